// Test helper (not product code): ONE GEMM of kernels_gemm.hip through its launcher, on buffers with guard regions, for tests/test_gpu_gemm_kernels.py.
//   hipcc --offload-arch=gfx950 -O2 -shared -fPIC -I../../nemotron-asr.cpp_amd/csrc -o libgemm_harness.so gemm_harness.hip   (built by __graft_entry__.build())
//
// No kernel of its own: nasr::launch_gemm_bf16 / launch_gemm_f32, launch_pack_weight_bf16, launch_f32_to_bf16 and init_gemm_kernel_attributes are the
// product's, resolved from libnemotron_asr_amd.so (the test loads that library with RTLD_GLOBAL before this one), so the plan and the kernel are tested
// as the pair the engine uses.  Chained launches (ChainParams::head_wgs > 0) are not offered.
//
// Every device buffer is [guard | body | guard], and every byte that is not an input is filled with the 16-bit pattern SENTINEL, a NaN both as bf16 and,
// doubled, as f32: an output element the kernel did not write fails the test's finiteness check, and a byte it wrote outside its output shows in
// the copy the caller gets back whole, guards included.  The A operand gets the slack rows behind row M - 1 that the engine's workspaces have
// (nasr_engine.hip: w_rows = max(max_streams x TMAX, MAXNEW) rows whatever M a step runs), filled with NaN.
#include "nasr_internal.h"
#include "nasr_gemm_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace {

constexpr uint16_t SENTINEL = 0xFFC5;

struct Case {                     // mirrored field by field by tests/test_gpu_gemm_kernels.py (ctypes, native alignment); gemm_harness_case_bytes() checks the size
    int M, N, K, lda;
    int rows_per_batch, batch_stride, row_offset;
    int epi, splits, ldo, ldo_act;
    int dtype;                    // 0: bf16 activations and packed bf16 weights (launch_gemm_bf16), 1: f32 (launch_gemm_f32)
    float resid_scale;
    int T, n_batch_rows, n_slots; // EPI_QKV: rows m -> stream m / T; RowDesc per stream; K/V rings of n_slots slots
    int coresident, prio, no_persist, no_wide, wide_rows, tile_bands, t64_tiles_p1, wide_min_tiles, wide_min_rows, narrow_stores, f32_fma_tile;
    int resid_in_place;           // EPI_RESID_F32: resid == out_f32
    int guard_bytes;              // multiple of 256
    long long a_elems;            // floats of the caller's A image (every row the row map addresses; gaps are the caller's to poison)
    long long out_f32_elems, out_act_elems, q_elems;      // body sizes in elements; 0: the buffer does not exist (null pointer in GemmParams)
};

struct PlanOut { int inst, grid[3], block, lds, n_groups, m_chunks, splits; };

struct Buf {
    char *base = nullptr;
    size_t body = 0, guard = 0;
    void *ptr() const { return base ? base + guard : nullptr; }
    size_t total() const { return body + 2 * guard; }
};

char g_err[512];
int fail(const char *what, hipError_t e) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, e == hipSuccess ? "" : hipGetErrorString(e));
    return -1;
}

// [guard | body | guard], all of it SENTINEL
int alloc(Buf &b, size_t body_bytes, size_t guard, std::vector<Buf *> &all) {
    b.body = (body_bytes + 255) & ~(size_t)255;
    b.guard = guard;
    hipError_t e = hipMalloc((void **)&b.base, b.total());
    if (e != hipSuccess) return fail("hipMalloc", e);
    all.push_back(&b);
    std::vector<uint16_t> fill(b.total() / 2, SENTINEL);
    e = hipMemcpy(b.base, fill.data(), b.total(), hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : fail("hipMemcpy (sentinel fill)", e);
}
int put(const Buf &b, const void *src, size_t bytes) {
    hipError_t e = hipMemcpy(b.ptr(), src, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : fail("hipMemcpy (upload)", e);
}
// the whole buffer back, guards included: the caller's array holds total() bytes
int get(const Buf &b, void *dst) {
    if (!b.base || !dst) return 0;
    hipError_t e = hipMemcpy(dst, b.base, b.total(), hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : fail("hipMemcpy (download)", e);
}

// the case's GemmParams without its pointers: everything gemm_plan_bf16 reads
nasr::GemmParams params_of(const Case &c) {
    nasr::GemmParams g;
    memset(&g, 0, sizeof(g));
    g.M = c.M; g.N = c.N; g.K = c.K; g.lda = c.lda;
    g.rows_per_batch = c.rows_per_batch; g.batch_stride = c.batch_stride; g.row_offset = c.row_offset;
    g.splits = c.splits; g.epi = c.epi; g.ldo = c.ldo; g.ldo_act = c.ldo_act; g.resid_scale = c.resid_scale; g.T = c.T;
    g.coresident = c.coresident; g.prio = c.prio; g.f32_fma_tile = c.f32_fma_tile; g.no_persist = c.no_persist; g.no_wide = c.no_wide;
    g.wide_rows = c.wide_rows; g.tile_bands = c.tile_bands; g.t64_tiles_p1 = c.t64_tiles_p1; g.wide_min_tiles = c.wide_min_tiles;
    g.wide_min_rows = c.wide_min_rows; g.narrow_stores = c.narrow_stores;
    return g;
}
PlanOut plan_out(const nasr::GemmPlan &pl) {
    return PlanOut{(int)pl.inst, {(int)pl.grid[0], (int)pl.grid[1], (int)pl.grid[2]}, pl.block, pl.lds, pl.n_groups, pl.m_chunks, pl.splits};
}

}  // namespace

extern "C" const char *gemm_harness_error() { return g_err; }
extern "C" int gemm_harness_inst_count() { return (int)nasr::GI_COUNT; }
extern "C" const char *gemm_harness_inst_name(int i) { return i >= 0 && i < nasr::GI_COUNT ? nasr::GEMM_INST_NAME[i] : ""; }
extern "C" int gemm_harness_case_bytes() { return (int)sizeof(Case); }
extern "C" unsigned gemm_harness_sentinel() { return SENTINEL; }
// rows of the engine workspace a step of M rows runs in: the smallest engine that takes M rows has ceil(M / TMAX) streams
extern "C" int gemm_harness_workspace_rows(int M) {
    const int w = (M + nasr::TMAX - 1) / nasr::TMAX * nasr::TMAX;
    return w > nasr::MAXNEW ? w : nasr::MAXNEW;
}
// bytes of a buffer of `body_bytes` as the entry below returns it
extern "C" long long gemm_harness_total_bytes(long long body_bytes, int guard_bytes) { return ((body_bytes + 255) & ~255ll) + 2ll * guard_bytes; }

// the plan of a bf16 case on a chip of num_cus CUs: gemm_plan_bf16 is pure host code, no GPU is touched
extern "C" void gemm_harness_plan(const Case *c, int num_cus, PlanOut *plan) { *plan = plan_out(nasr::gemm_plan_bf16(params_of(*c), num_cus)); }
extern "C" int gemm_harness_num_cus(int device) {
    int cus = 0;
    return hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess ? cus : -1;
}

// Runs one GEMM.  Inputs are host arrays of f32 (A: c->a_elems, W: [N][K], bias: [N] or null, resid: c->out_f32_elems or null) and of int (slot,
// kv_head: c->n_batch_rows each, or null).  The four outputs are host arrays of gemm_harness_total_bytes(body) bytes, or null.
// Returns 0, or -1 with gemm_harness_error() set; plan->inst = -1 for f32 cases (launch_gemm_f32 has no plan).
extern "C" int gemm_harness_run(int device, const Case *c, const float *A, const float *W, const float *bias, const float *resid, const int *slot,
                                const int *kv_head, void *out_f32, void *out_act, void *q_out, void *kv_pool, PlanOut *plan, int *num_cus) {
    using namespace nasr;
    g_err[0] = 0;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail("hipSetDevice", e);
    if (hipDeviceGetAttribute(num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return fail("CU count", hipErrorUnknown);
    static bool attrs = false;
    if (!attrs) { init_gemm_kernel_attributes(); attrs = true; }
    const bool bf = c->dtype == 0;
    const size_t esz = bf ? 2 : 4, G = (size_t)c->guard_bytes;
    if (c->M < 1 || c->N % 16 || (bf && c->K % 32) || (G & 255)) return fail("bad case", hipSuccess);

    std::vector<Buf *> all;
    Buf dA32, dA, dW32, dW, dBias, dResid, dOut, dAct, dQ, dKV, dRows;
    int rc = 0;
    // ---- A: the caller's image + NaN slack rows, as f32; converted as a whole for the bf16 kernels
    const size_t slack = (size_t)(gemm_harness_workspace_rows(c->M) - c->M) * c->lda, a_all = (size_t)c->a_elems + slack;
    {
        std::vector<float> ha(a_all);
        memcpy(ha.data(), A, (size_t)c->a_elems * 4);
        const uint32_t qnan = 0x7fc00000u;
        for (size_t i = (size_t)c->a_elems; i < a_all; i++) memcpy(&ha[i], &qnan, 4);
        rc |= alloc(bf ? dA32 : dA, a_all * 4, G, all);
        if (!rc) rc |= put(bf ? dA32 : dA, ha.data(), a_all * 4);
    }
    if (!rc && bf) {
        rc |= alloc(dA, a_all * 2, G, all);
        if (!rc) launch_f32_to_bf16((const float *)dA32.ptr(), (bf16_t *)dA.ptr(), (int64_t)a_all, 0);
    }
    // ---- W: f32 [N][K]; packed into MFMA fragment tiles for the bf16 kernels
    const size_t w_elems = (size_t)c->N * c->K;
    if (!rc) rc |= alloc(bf ? dW32 : dW, w_elems * 4, G, all);
    if (!rc) rc |= put(bf ? dW32 : dW, W, w_elems * 4);
    if (!rc && bf) {
        rc |= alloc(dW, w_elems * 2, G, all);
        if (!rc) launch_pack_weight_bf16((const float *)dW32.ptr(), (bf16_t *)dW.ptr(), c->N, c->K, 0);
    }
    if (!rc && bias) { rc |= alloc(dBias, (size_t)c->N * 4, G, all); if (!rc) rc |= put(dBias, bias, (size_t)c->N * 4); }
    // ---- outputs
    if (!rc && c->out_f32_elems) rc |= alloc(dOut, (size_t)c->out_f32_elems * 4, G, all);
    if (!rc && c->out_act_elems) rc |= alloc(dAct, (size_t)c->out_act_elems * esz, G, all);
    if (!rc && c->q_elems) rc |= alloc(dQ, (size_t)c->q_elems * 4, G, all);
    const int64_t kv_slot_stride = (int64_t)2 * KVC * D;
    if (!rc && c->n_slots) rc |= alloc(dKV, (size_t)c->n_slots * kv_slot_stride * esz, G, all);
    if (!rc && resid) {
        if (c->resid_in_place) rc |= put(dOut, resid, (size_t)c->out_f32_elems * 4);
        else { rc |= alloc(dResid, (size_t)c->out_f32_elems * 4, G, all); if (!rc) rc |= put(dResid, resid, (size_t)c->out_f32_elems * 4); }
    }
    if (!rc && c->n_batch_rows) {
        std::vector<RowDesc> rd(c->n_batch_rows);
        memset(rd.data(), 0, rd.size() * sizeof(RowDesc));
        for (int b = 0; b < c->n_batch_rows; b++) { rd[b].slot = slot[b]; rd[b].kv_head = kv_head[b]; rd[b].prompt = -1; }
        rc |= alloc(dRows, rd.size() * sizeof(RowDesc), G, all);
        if (!rc) rc |= put(dRows, rd.data(), rd.size() * sizeof(RowDesc));
    }
    if (!rc) {
        GemmParams g = params_of(*c);
        g.A = dA.ptr(); g.W = dW.ptr();
        g.out_f32 = (float *)dOut.ptr(); g.out_act = dAct.ptr();
        g.bias = (const float *)dBias.ptr();
        g.resid = resid ? (const float *)(c->resid_in_place ? dOut.ptr() : dResid.ptr()) : nullptr;
        g.q_out = (float *)dQ.ptr(); g.kv_pool = dKV.ptr(); g.kv_slot_stride = kv_slot_stride;
        g.rows = (const RowDesc *)dRows.ptr();
        memset(plan, 0, sizeof(*plan));
        plan->inst = -1;
        if (bf) {
            const GemmPlan pl = gemm_plan_bf16(g, *num_cus);          // what launch_gemm_bf16 computes from the same params and CU count
            *plan = plan_out(pl);
            launch_gemm_bf16(g, 0);
        } else {
            launch_gemm_f32(g, 0);
        }
        e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = fail("hipDeviceSynchronize", e);
        else if ((e = hipGetLastError()) != hipSuccess) rc = fail("launch", e);
    }
    if (!rc) rc |= get(dOut, out_f32) | get(dAct, out_act) | get(dQ, q_out) | get(dKV, kv_pool);
    for (Buf *b : all) (void)hipFree(b->base);
    return rc ? -1 : 0;
}
