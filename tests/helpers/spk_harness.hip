// Test helper (not product code): ONE launcher call of the TitaNet-L side-car kernels on buffers with guard regions, for tests/test_gpu_spk_kernels.py.
//   hipcc --offload-arch=gfx950 -O2 -shared -fPIC -I../../nemotron-asr.cpp_amd/csrc -I../../include -o libspk_harness.so spk_harness.hip   (built by __graft_entry__.build())
//
// It has no kernel of its own.  The kernels are the product's, reached through its launchers: launch_spk_gemm, launch_spk_tile, launch_spk_front, launch_spk_fc,
// launch_gather_audio (kernels_spk.hip) and the eight launch_spk_* of kernels_diar.hip, resolved from libnemotron_asr_amd.so (the test loads that library with
// RTLD_GLOBAL before this one).  bf16 weights go through the product's launch_pack_weight_bf16, f32 MFMA weights through nasr_eng::pack_f32_mfma (as decode_harness.hip
// does); nasr_diar.hip's own pack_mfma_f32 documents the same layout and is not used here.
//
// The buffer plumbing is the other harnesses': buffers by handle, each [guard | body | guard] and all of it the 16-bit pattern SENTINEL; the test uploads its inputs
// into the bodies and gets every buffer back whole.  Before anything is launched every entry checks the shape against the launcher's own rule (spk_gemm_check for
// the GEMM), every buffer's body against the bytes the launch addresses -- all 160 rows per segment of every activation -- and every lens[s] against [1, 160] (the
// kernels divide by L; the product clamps to 1 .. 150): a case that fails a check is an error, never a launch.
// launch_spk_gemm / launch_spk_tile take a first segment `seg0` into buffers of `S_total` segments: the launch sees segments seg0 .. seg0 + S - 1, the segments
// in front of and behind them hold what the test put there (loud values the launch must neither read nor write).
#include "nasr_internal.h"
#include "nasr_engine_priv.h"
#include <stdio.h>
#include <string.h>
#include <vector>

namespace {

using namespace nasr;

constexpr uint16_t SENTINEL = 0xFFC5;

struct Buf {
    char *base = nullptr;
    size_t body = 0, guard = 0;
    void *ptr() const { return base ? base + guard : nullptr; }
    size_t total() const { return body + 2 * guard; }
};
std::vector<Buf> g_bufs;
bool g_attr = false;

char g_err[512];
int herr(const char *what, hipError_t e = hipSuccess) {
    snprintf(g_err, sizeof(g_err), "%s%s%s", what, e == hipSuccess ? "" : ": ", e == hipSuccess ? "" : hipGetErrorString(e));
    return -1;
}
const Buf *buf(int h) { return h >= 0 && h < (int)g_bufs.size() && g_bufs[h].base ? &g_bufs[h] : nullptr; }
template <typename T = void> T *ptr(int h) { const Buf *b = buf(h); return b ? (T *)b->ptr() : nullptr; }
bool need(int h, size_t bytes, const char *name) {
    const Buf *b = buf(h);
    if (b && b->body >= bytes) return true;
    snprintf(g_err, sizeof(g_err), "buffer %s: handle %d holds %zu bytes, the launch addresses %zu", name, h, b ? b->body : (size_t)0, bytes);
    return false;
}
int sync_check() {
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return herr("hipDeviceSynchronize", e);
    if ((e = hipGetLastError()) != hipSuccess) return herr("launch", e);
    return 0;
}
// lens [S_total] on the device: every entry in [1, SPK_T]
bool lens_ok(int h, int S) {
    if (S < 1 || S > 4096) { herr("S outside 1 .. 4096"); return false; }
    if (!need(h, (size_t)S * 4, "lens")) return false;
    std::vector<int> l(S);
    if (hipMemcpy(l.data(), ptr(h), (size_t)S * 4, hipMemcpyDeviceToHost) != hipSuccess) { herr("lens: download"); return false; }
    for (int v : l)
        if (v < 1 || v > SPK_T) { herr("lens: an entry outside 1 .. 160"); return false; }
    return true;
}
// bytes of a [rows][ld] matrix of which `cols` columns are addressed in every row
size_t mat(size_t rows, size_t ld, size_t cols, size_t elem) { return rows ? ((rows - 1) * ld + cols) * elem : 0; }

// every buffer of a SpkGemmParams by handle (-1 = null)
struct SgCase {
    int A, lda, W, S, N, K, mode, bias, lens, dw_w, dw_k, a_out, lda_out, y_out, colmean, y_in, z, x_out, x_in, bn_s, bn_b, pool, seg0, S_total;
};
struct StCase {
    int y_in, z, lens, S, C, mode, x_out, dw_w, dw_k, a_out, lda_out, mean, stdv, stat_ld, seg0, S_total;
};

}  // namespace

extern "C" const char *spk_harness_error() { return g_err; }
extern "C" unsigned spk_harness_sentinel() { return SENTINEL; }
extern "C" int spk_harness_struct_bytes(int which) {
    const int v[] = {(int)sizeof(SgCase), (int)sizeof(StCase), (int)sizeof(GatherDesc)};
    return which >= 0 && which < 3 ? v[which] : -1;
}
extern "C" int spk_harness_constant(int which) {
    const int v[] = {SPK_T, SPK_TVALID, DIAR_NMEL, SG_DW, SG_Y, SG_RES, SG_ASP, ST_DW, ST_STATS};
    return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : -1;
}

extern "C" int spk_harness_init(int device) {
    g_err[0] = 0;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return herr("hipSetDevice", e);
    if (!g_attr) { init_spk_kernel_attributes(); g_attr = true; }
    return 0;
}
extern "C" int spk_harness_alloc(long long body_bytes, int guard_bytes) {
    g_err[0] = 0;
    if (body_bytes < 0 || guard_bytes < 256 || (guard_bytes & 255)) return herr("alloc: sizes");
    Buf b;
    b.body = ((size_t)body_bytes + 255) & ~(size_t)255;
    b.guard = guard_bytes;
    hipError_t e = hipMalloc((void **)&b.base, b.total());
    if (e != hipSuccess) return herr("hipMalloc", e);
    std::vector<uint16_t> fill(b.total() / 2, SENTINEL);
    e = hipMemcpy(b.base, fill.data(), b.total(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(b.base); return herr("hipMemcpy (sentinel fill)", e); }
    g_bufs.push_back(b);
    return (int)g_bufs.size() - 1;
}
extern "C" long long spk_harness_total_bytes(int h) { const Buf *b = buf(h); return b ? (long long)b->total() : -1; }
extern "C" int spk_harness_put(int h, long long off, const void *src, long long bytes) {
    g_err[0] = 0;
    const Buf *b = buf(h);
    if (!b || off < 0 || bytes < 0 || (size_t)(off + bytes) > b->body) return herr("put: outside the body");
    if (bytes == 0) return 0;
    hipError_t e = hipMemcpy((char *)b->ptr() + off, src, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : herr("hipMemcpy (upload)", e);
}
extern "C" int spk_harness_get(int h, void *dst) {
    g_err[0] = 0;
    const Buf *b = buf(h);
    if (!b) return herr("get: handle");
    hipError_t e = hipMemcpy(dst, b->base, b->total(), hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : herr("hipMemcpy (download)", e);
}
extern "C" int spk_harness_count() { return (int)g_bufs.size(); }
extern "C" void spk_harness_free_from(int first) {
    if (first < 0) first = 0;
    for (size_t i = first; i < g_bufs.size(); i++)
        if (g_bufs[i].base) (void)hipFree(g_bufs[i].base);
    if ((size_t)first < g_bufs.size()) g_bufs.resize(first);
}
extern "C" void spk_harness_free_all() { spk_harness_free_from(0); }

// W [N][K] f32 row-major in src -> the bf16 16 x 32 tiles of launch_pack_weight_bf16 in dst
extern "C" int spk_harness_pack_bf16(int src, int dst, int N, int K) {
    g_err[0] = 0;
    if (N < 16 || N % 16 || K < 32 || K % 32) return herr("pack_bf16: N a multiple of 16, K a multiple of 32");
    if (!need(src, (size_t)N * K * 4, "pack src") || !need(dst, (size_t)N * K * 2, "pack dst")) return -1;
    launch_pack_weight_bf16(ptr<float>(src), ptr<bf16_t>(dst), N, K, 0);
    return sync_check();
}
// W [N][K] f32 row-major in src -> the f32 MFMA A-fragment order of nasr_eng::pack_f32_mfma in dst (on the host)
extern "C" int spk_harness_pack_f32(int src, int dst, int N, int K) {
    g_err[0] = 0;
    if (N < 16 || N % 16 || K < 16 || K % 16) return herr("pack_f32: N and K multiples of 16");
    if (!need(src, (size_t)N * K * 4, "pack src") || !need(dst, (size_t)N * K * 4, "pack dst")) return -1;
    std::vector<float> w((size_t)N * K), t;
    if (hipMemcpy(w.data(), ptr(src), w.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return herr("pack src: download");
    nasr_eng::pack_f32_mfma(w, N, K, false, t);
    if (t.size() != w.size()) return herr("pack_f32: the packer's output has another size than the kernel indexes");
    hipError_t e = hipMemcpy(ptr(dst), t.data(), t.size() * 4, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : herr("hipMemcpy (packed weights)", e);
}

extern "C" int spk_harness_gemm(const SgCase *c) {
    g_err[0] = 0;
    const int S = c->S, N = c->N, K = c->K, St = c->S_total, s0 = c->seg0;
    if (S < 1 || s0 < 0 || St < s0 + S || N < 1 || N > 8192 || K < 1 || K > 8192 || c->lda < 1 || c->lda > 16384) return herr("gemm: S, seg0, N, K or lda outside the harness's range");
    if (!lens_ok(c->lens, St)) return -1;
    const size_t R = (size_t)St * SPK_T;
    if (!need(c->A, mat(R, c->lda, K, 2), "A") || !need(c->W, (size_t)N * K * 2, "W") || !need(c->bias, (size_t)N * 4, "bias")) return -1;
    const bool taps = c->mode == SG_DW || (c->mode == SG_RES && c->dw_k > 1);
    if (taps) {
        if (c->dw_k < 1 || c->dw_k > 15 || c->lda_out < N || c->lda_out > 16384) return herr("gemm: dw_k or lda_out");
        if (!need(c->dw_w, (size_t)c->dw_k * N * 4, "dw_w") || !need(c->a_out, mat(R, c->lda_out, N, 2), "a_out")) return -1;
    }
    if (c->mode == SG_Y && (!need(c->y_out, R * N * 4, "y_out") || !need(c->colmean, (size_t)St * N * 4, "colmean"))) return -1;
    if (c->mode == SG_RES && (!need(c->y_in, R * N * 4, "y_in") || !need(c->z, (size_t)St * N * 4, "z") || !need(c->x_out, R * N * 2, "x_out"))) return -1;
    if (c->mode == SG_ASP && (!need(c->x_in, R * N * 2, "x_in") || !need(c->bn_s, (size_t)2 * N * 4, "bn_s") || !need(c->bn_b, (size_t)2 * N * 4, "bn_b") ||
                              !need(c->pool, (size_t)St * 2 * N * 4, "pool")))
        return -1;
    const size_t r0 = (size_t)s0 * SPK_T;
    SpkGemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = ptr<bf16_t>(c->A) + r0 * c->lda; p.lda = c->lda; p.W = ptr<bf16_t>(c->W);
    p.S = S; p.N = N; p.K = K; p.mode = c->mode;
    p.bias = ptr<float>(c->bias); p.lens = ptr<int>(c->lens) + s0;
    p.dw_w = ptr<float>(c->dw_w); p.dw_k = c->dw_k; p.lda_out = c->lda_out;
    if (buf(c->a_out)) p.a_out = ptr<bf16_t>(c->a_out) + r0 * c->lda_out;
    if (buf(c->y_out)) p.y_out = ptr<float>(c->y_out) + r0 * N;
    if (buf(c->colmean)) p.colmean = ptr<float>(c->colmean) + (size_t)s0 * N;
    if (buf(c->y_in)) p.y_in = ptr<float>(c->y_in) + r0 * N;
    if (buf(c->z)) p.z = ptr<float>(c->z) + (size_t)s0 * N;
    if (buf(c->x_out)) p.x_out = ptr<bf16_t>(c->x_out) + r0 * N;
    if (buf(c->x_in)) p.x_in = ptr<bf16_t>(c->x_in) + r0 * N;
    p.bn_s = ptr<float>(c->bn_s); p.bn_b = ptr<float>(c->bn_b);
    if (buf(c->pool)) p.pool = ptr<float>(c->pool) + (size_t)s0 * 2 * N;
    if (const char *why = spk_gemm_check(p)) { snprintf(g_err, sizeof(g_err), "spk_gemm_check: %s", why); return -1; }
    if (launch_spk_gemm(p, 0) != 0) return herr("launch_spk_gemm refused the case");
    return sync_check();
}

extern "C" int spk_harness_tile(const StCase *c) {
    g_err[0] = 0;
    const int S = c->S, C = c->C, St = c->S_total, s0 = c->seg0;
    if (S < 1 || s0 < 0 || St < s0 + S || C < 64 || C % 64 || C > 8192) return herr("tile: S, seg0 or C (a multiple of 64)");
    if (!lens_ok(c->lens, St)) return -1;
    const size_t R = (size_t)St * SPK_T, r0 = (size_t)s0 * SPK_T;
    if (!need(c->y_in, R * C * 4, "y_in") || !need(c->z, (size_t)St * C * 4, "z") || !need(c->x_out, R * C * 2, "x_out")) return -1;
    SpkTileParams p;
    memset(&p, 0, sizeof(p));
    p.y_in = ptr<float>(c->y_in) + r0 * C; p.z = ptr<float>(c->z) + (size_t)s0 * C; p.lens = ptr<int>(c->lens) + s0;
    p.S = S; p.C = C; p.mode = c->mode; p.x_out = ptr<bf16_t>(c->x_out) + r0 * C;
    if (c->mode == ST_DW) {
        if ((c->dw_k != 3 && c->dw_k != 7 && c->dw_k != 11 && c->dw_k != 15) || c->lda_out < C || c->lda_out > 16384) return herr("tile: dw_k or lda_out");
        if (!need(c->dw_w, (size_t)c->dw_k * C * 4, "dw_w") || !need(c->a_out, mat(R, c->lda_out, C, 2), "a_out")) return -1;
        p.dw_w = ptr<float>(c->dw_w); p.dw_k = c->dw_k; p.a_out = ptr<bf16_t>(c->a_out) + r0 * c->lda_out; p.lda_out = c->lda_out;
    } else if (c->mode == ST_STATS) {
        const bool halves = c->mean == c->stdv;          // one [S][stat_ld >= 2 C] buffer: mean in columns 0 .. C - 1, std in C .. 2 C - 1 (the product's pooling input)
        if (c->stat_ld < (halves ? 2 * C : C) || c->stat_ld > 16384) return herr("tile: stat_ld");
        if (!need(c->mean, mat(St, c->stat_ld, halves ? 2 * C : C, 4), "mean") || !need(c->stdv, mat(St, c->stat_ld, halves ? 2 * C : C, 4), "stdv")) return -1;
        p.mean = ptr<float>(c->mean) + (size_t)s0 * c->stat_ld; p.stdv = ptr<float>(c->stdv) + (size_t)s0 * c->stat_ld + (halves ? C : 0); p.stat_ld = c->stat_ld;
    } else return herr("tile: mode");
    if (launch_spk_tile(p, 0) != 0) return herr("launch_spk_tile refused the case");
    return sync_check();
}

extern "C" int spk_harness_front(int mel, int cpitch, int dw_w, int lens, int a_out, int lda_out, int S) {
    g_err[0] = 0;
    if (cpitch < DIAR_NMEL || cpitch > 4096 || lda_out < 128 || lda_out > 4096) return herr("front: cpitch >= 80, lda_out >= 128");
    if (!lens_ok(lens, S)) return -1;
    const size_t R = (size_t)S * SPK_T;
    if (!need(mel, mat(R, cpitch, DIAR_NMEL, 4), "mel") || !need(dw_w, 3 * DIAR_NMEL * 4, "dw_w") || !need(a_out, mat(R, lda_out, 128, 2), "a_out")) return -1;
    if (launch_spk_front(ptr<float>(mel), cpitch, ptr<float>(dw_w), ptr<int>(lens), ptr<bf16_t>(a_out), lda_out, S, 0) != 0) return herr("launch_spk_front refused the case");
    return sync_check();
}

extern "C" int spk_harness_fc_slices(int M, int K, int N) { return spk_fc_slices(M, K, N); }
extern "C" int spk_harness_fc(int x, int ldx, int wpk, int bias, int out, int part, int M, int K, int N, int relu) {
    g_err[0] = 0;
    if (M < 1 || M > 65535 * 64 || N < 16 || N % 16 || N > 65535 * 16 || K < 64 || K % 64 || K > (1 << 20) || ldx < K || ldx % 4 || ldx > (1 << 20))
        return herr("fc: M >= 1, N a multiple of 16, K a multiple of 64, ldx >= K and a multiple of 4");
    const int Z = spk_fc_slices(M, K, N);
    if (Z < 1 || Z > 16 || (K / 16) % (4 * Z)) return herr("fc: spk_fc_slices gives a split the kernel's K walk does not cover");
    if (!need(x, mat(M, ldx, K, 4), "x") || !need(wpk, (size_t)N * K * 4, "wpk") || !need(bias, (size_t)N * 4, "bias") || !need(out, (size_t)M * N * 4, "out")) return -1;
    if (Z > 1 && !need(part, (size_t)Z * M * N * 4, "part")) return -1;
    if (launch_spk_fc(ptr<float>(x), ldx, ptr<float>(wpk), ptr<float>(bias), ptr<float>(out), ptr<float>(part), M, K, N, relu, 0) != 0) return herr("launch_spk_fc refused the case");
    return sync_check();
}

// desc [B][3] = (offset into src, dst_off, bytes); the table is built here from the source buffer's address
extern "C" int spk_harness_gather(int src, int dst, int tab, const long long *desc, int B, long long max_bytes) {
    g_err[0] = 0;
    const Buf *sb = buf(src), *db = buf(dst);
    if (!sb || !db || B < 1 || B > 65535 || max_bytes < 1) return herr("gather: handles, B or max_bytes");
    if (!need(tab, (size_t)B * sizeof(GatherDesc), "tab")) return -1;
    std::vector<GatherDesc> t(B);
    for (int b = 0; b < B; b++) {
        const long long so = desc[3 * b], dof = desc[3 * b + 1], n = desc[3 * b + 2];
        if (so < 0 || dof < 0 || n < 0 || (so & 1) || (dof & 1) || (n & 1) || (size_t)(so + n) > sb->body || (size_t)(dof + n) > db->body)
            return herr("gather: a descriptor outside its buffers, or odd");
        t[b].src = (const char *)sb->ptr() + so; t[b].dst_off = dof; t[b].bytes = n;
    }
    if (hipMemcpy(ptr(tab), t.data(), t.size() * sizeof(GatherDesc), hipMemcpyHostToDevice) != hipSuccess) return herr("gather: table upload");
    launch_gather_audio(ptr<GatherDesc>(tab), B, max_bytes, ptr<char>(dst), 0);
    return sync_check();
}

// ---- the f32 engine's layer-by-layer kernels (kernels_diar.hip) ----
static bool sc_ok(int S, int C, int lo = 1) {
    if (S < 1 || S > 4096 || C < lo || C > 8192) { herr("S or C outside the harness's range"); return false; }
    return true;
}
extern "C" int spk_harness_depthwise(int x, int x_pitch, int w, int kernel, int C, int Cpad, int lens, int a_out, int S) {
    g_err[0] = 0;
    if (!sc_ok(S, C) || kernel < 1 || kernel > 15 || !(kernel & 1) || Cpad < C || Cpad > 8192 || x_pitch < C || x_pitch > 16384) return g_err[0] ? -1 : herr("depthwise: kernel odd 1 .. 15, Cpad >= C, x_pitch >= C");
    if (!lens_ok(lens, S)) return -1;
    const size_t R = (size_t)S * SPK_T;
    if (!need(x, mat(R, x_pitch, C, 4), "x") || !need(w, (size_t)kernel * C * 4, "w") || !need(a_out, R * Cpad * 4, "a_out")) return -1;
    launch_spk_depthwise(ptr<float>(x), x_pitch, ptr<float>(w), kernel, C, Cpad, ptr<int>(lens), ptr<float>(a_out), S, 0);
    return sync_check();
}
extern "C" int spk_harness_mask_cvt(int x, int C, int lens, int a_out, int S) {
    g_err[0] = 0;
    if (!sc_ok(S, C) || !lens_ok(lens, S)) return -1;
    const size_t n = (size_t)S * SPK_T * C * 4;
    if (!need(x, n, "x") || !need(a_out, n, "a_out")) return -1;
    launch_spk_mask_cvt(ptr<float>(x), C, ptr<int>(lens), ptr<float>(a_out), S, 0);
    return sync_check();
}
extern "C" int spk_harness_colmean(int y, int C, int lens, int mean, int S) {
    g_err[0] = 0;
    if (!sc_ok(S, C) || !lens_ok(lens, S)) return -1;
    if (!need(y, (size_t)S * SPK_T * C * 4, "y") || !need(mean, (size_t)S * C * 4, "mean")) return -1;
    launch_spk_colmean(ptr<float>(y), C, ptr<int>(lens), ptr<float>(mean), S, 0);
    return sync_check();
}
extern "C" int spk_harness_combine(int y, int z, int r, int C, int lens, int out, int S) {
    g_err[0] = 0;
    if (!sc_ok(S, C) || !lens_ok(lens, S)) return -1;
    const size_t n = (size_t)S * SPK_T * C * 4;
    if (!need(y, n, "y") || !need(z, (size_t)S * C * 4, "z") || (r >= 0 && !need(r, n, "r")) || !need(out, n, "out")) return -1;
    launch_spk_combine(ptr<float>(y), ptr<float>(z), ptr<float>(r), C, ptr<int>(lens), ptr<float>(out), S, 0);
    return sync_check();
}
extern "C" int spk_harness_stats(int x, int C, int lens, int mean, int stdv, int S) {
    g_err[0] = 0;
    if (!sc_ok(S, C) || !lens_ok(lens, S)) return -1;
    if (!need(x, (size_t)S * SPK_T * C * 4, "x") || !need(mean, (size_t)S * C * 4, "mean") || !need(stdv, (size_t)S * C * 4, "stdv")) return -1;
    launch_spk_stats(ptr<float>(x), C, ptr<int>(lens), ptr<float>(mean), ptr<float>(stdv), S, 0);
    return sync_check();
}
extern "C" int spk_harness_att_const(int mean, int stdv, int w1, int b1, int cst, int C, int A, int S) {
    g_err[0] = 0;
    if (!sc_ok(S, C) || A < 1 || A > 4096) return g_err[0] ? -1 : herr("att_const: A");
    if (!need(mean, (size_t)S * C * 4, "mean") || !need(stdv, (size_t)S * C * 4, "stdv") || !need(w1, (size_t)A * 3 * C * 4, "w1") || !need(b1, (size_t)A * 4, "b1") ||
        !need(cst, (size_t)S * A * 4, "cst"))
        return -1;
    launch_spk_att_const(ptr<float>(mean), ptr<float>(stdv), ptr<float>(w1), ptr<float>(b1), ptr<float>(cst), C, A, S, 0);
    return sync_check();
}
extern "C" int spk_harness_att_post(int g, int cst, int sc, int bi, int a_out, int out_bf16, int A, int S) {
    g_err[0] = 0;
    if (S < 1 || S > 4096 || A < 1 || A > 128) return herr("att_post: S, or A outside 1 .. 128 (one thread per a, 128 threads)");
    const size_t n = (size_t)S * SPK_T * A;
    if (!need(g, n * 4, "g") || !need(cst, (size_t)S * A * 4, "cst") || !need(sc, (size_t)A * 4, "sc") || !need(bi, (size_t)A * 4, "bi") || !need(a_out, n * (out_bf16 ? 2 : 4), "a_out")) return -1;
    launch_spk_att_post(ptr<float>(g), ptr<float>(cst), ptr<float>(sc), ptr<float>(bi), ptr(a_out), out_bf16 ? 1 : 0, A, S, 0);
    return sync_check();
}
extern "C" int spk_harness_asp(int x, int logits, int C, int lens, int sc, int bi, int pool, int S) {
    g_err[0] = 0;
    if (!sc_ok(S, C) || !lens_ok(lens, S)) return -1;
    const size_t n = (size_t)S * SPK_T * C * 4;
    if (!need(x, n, "x") || !need(logits, n, "logits") || !need(sc, (size_t)2 * C * 4, "sc") || !need(bi, (size_t)2 * C * 4, "bi") || !need(pool, (size_t)S * 2 * C * 4, "pool")) return -1;
    launch_spk_asp(ptr<float>(x), ptr<float>(logits), C, ptr<int>(lens), ptr<float>(sc), ptr<float>(bi), ptr<float>(pool), S, 0);
    return sync_check();
}
