// Test helper (not product code): one f32 GEMM through launch_gemm_f32 as kind 2 (k_gemm_f32_split) and as kind 3 (k_gemm_f32_split_planes) on the same
// operands, with the weight plane that launch_split_weight_planes makes, for tests/test_gpu_gemm_f32_split_planes.py.
//   hipcc --offload-arch=gfx950 -O2 -shared -fPIC -I../../nemotron-asr.cpp_amd/csrc -o libgemm_planes_harness.so gemm_planes_harness.hip   (built by __graft_entry__.build())
// No kernel of its own: the launchers are the product's, resolved from libnemotron_asr_amd.so (loaded with RTLD_GLOBAL before this library).
#include "nasr_internal.h"
#include <stdio.h>
#include <string.h>
#include <vector>

static char g_err[256];
extern "C" const char *gemm_planes_error() { return g_err; }

// A: [M][lda] f32, W: [N][K] f32 (host).  force & 3: 0 = the launcher's tile rule, 1 .. 3 = bits 4-5 of f32_fma_tile; force & 4: kind 3 is launched before kind 2
// (tests/micro/f32_split_planes_cost.py alternates the order of its two arms).  Returns out2 / out3 [M][N] f32 (plain f32
// epilogue, every element NaN before the launch) and the plane's N K 4 bytes.  Shapes outside the split kernels' conditions are refused: there both kinds
// would run the FMA tile kernel and compare equal for nothing.
extern "C" int gemm_planes_run(int device, const float *A, const float *W, int M, int N, int K, int lda, int force, float *out2, float *out3, void *plane) {
    using namespace nasr;
    g_err[0] = 0;
    if (M <= 4 || N % 64 || K % 32 || lda % 4 || lda < K || force < 0 || force > 7) { snprintf(g_err, sizeof(g_err), "not a split-kernel shape"); return -1; }
    const size_t a_bytes = (size_t)M * lda * 4, w_bytes = (size_t)N * K * 4, o_bytes = (size_t)M * N * 4;
    char *dA = nullptr, *dW = nullptr, *dP = nullptr, *dO[2] = {nullptr, nullptr};
    hipError_t e = hipSetDevice(device);
    static bool attrs = false;
    if (e == hipSuccess && !attrs) { init_gemm_kernel_attributes(); attrs = true; }
    if (e == hipSuccess) e = hipMalloc((void **)&dA, a_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&dW, w_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&dP, w_bytes);
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipMalloc((void **)&dO[i], o_bytes);
    if (e == hipSuccess) e = hipMemcpy(dA, A, a_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dW, W, w_bytes, hipMemcpyHostToDevice);
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipMemset(dO[i], 0xff, o_bytes);
    if (e == hipSuccess) e = hipMemset(dP, 0xff, w_bytes);
    if (e == hipSuccess) {
        launch_split_weight_planes((const float *)dW, dP, N, K, 0);
        for (int n = 0; n < 2; n++) {
            const int i = n ^ (force >> 2);          // 0: kind 2, 1: kind 3
            GemmParams g;
            memset(&g, 0, sizeof(g));
            g.A = dA; g.W = dW; g.W_planes = i ? dP : nullptr; g.M = M; g.N = N; g.K = K; g.lda = lda; g.splits = 1;
            g.epi = EPI_PART_F32; g.out_f32 = (float *)dO[i]; g.ldo = N;
            g.f32_fma_tile = (i ? 3 : 2) + 16 * (force & 3);
            launch_gemm_f32(g, 0);
        }
        e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out2, dO[0], o_bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out3, dO[1], o_bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(plane, dP, w_bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) snprintf(g_err, sizeof(g_err), "%s", hipGetErrorString(e));
    for (char *p : {dA, dW, dP, dO[0], dO[1]}) if (p) (void)hipFree(p);
    return e == hipSuccess ? 0 : -1;
}
