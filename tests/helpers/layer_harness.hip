// Test helper (not product code): ONE launch of kernels_layer.hip / kernels_fused.hip through its launcher, on buffers with guard regions, for
// tests/test_gpu_layer_kernels.py.
//   hipcc --offload-arch=gfx950 -O2 -shared -fPIC -I../../nemotron-asr.cpp_amd/csrc -o liblayer_harness.so layer_harness.hip   (built by __graft_entry__.build())
//
// No kernel of its own: nasr::launch_post / launch_attention / launch_dwconv / launch_fused_skinny / launch_fused_skinny_group,
// launch_pack_weight_bf16, launch_f32_to_bf16 and init_fused_kernel_attributes are the product's, resolved from libnemotron_asr_amd.so (the test
// loads that library with RTLD_GLOBAL before this one).
//
// The test owns the layout: it allocates device buffers by handle, each [guard | body | guard] and all of it the 16-bit pattern SENTINEL (a NaN as
// bf16 and, doubled, as f32), uploads its inputs into the bodies -- poison rows included -- and gets every buffer back whole, guards included.
// The launch entries take handles.  Before anything is launched they check the shapes against the kernels' limits, every buffer's body against
// the bytes the launch addresses, and every row descriptor against the pools (slot, kv_head, cc_par): a case the kernels' indexing does not
// cover is an error, never a launch.
#include "nasr_internal.h"
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

char g_err[512];
int fail(const char *what, hipError_t e = hipSuccess) {
    snprintf(g_err, sizeof(g_err), "%s%s%s", what, e == hipSuccess ? "" : ": ", e == hipSuccess ? "" : hipGetErrorString(e));
    return -1;
}
const Buf *buf(int h) { return h >= 0 && h < (int)g_bufs.size() && g_bufs[h].base ? &g_bufs[h] : nullptr; }
void *ptr(int h) { const Buf *b = buf(h); return b ? b->ptr() : nullptr; }
// handle h holds at least `bytes` in its body (optional = true: h < 0 is "no such buffer")
bool need(int h, size_t bytes, const char *name, bool optional = false) {
    if (h < 0 && optional) return true;
    const Buf *b = buf(h);
    if (b && b->body >= bytes) return true;
    snprintf(g_err, sizeof(g_err), "buffer %s: handle %d holds %zu bytes, the launch addresses %zu", name, h, b ? b->body : (size_t)0, bytes);
    return false;
}
int sync_check() {
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail("hipDeviceSynchronize", e);
    if ((e = hipGetLastError()) != hipSuccess) return fail("launch", e);
    return 0;
}
// the B row descriptors of handle h, checked against the pools they index
bool rows_ok(int h, int B, int kv_slots, int cc_slots) {
    if (B < 1 || !need(h, (size_t)B * sizeof(RowDesc), "rows")) { if (B < 1) fail("rows: B < 1"); return false; }
    std::vector<RowDesc> rd(B);
    if (hipMemcpy(rd.data(), ptr(h), rd.size() * sizeof(RowDesc), hipMemcpyDeviceToHost) != hipSuccess) { fail("rows: download"); return false; }
    for (const RowDesc &r : rd) {
        if (r.slot < 0 || (kv_slots >= 0 && r.slot >= kv_slots) || (cc_slots >= 0 && r.slot >= cc_slots)) { fail("rows: slot outside the pool"); return false; }
        if (r.kv_head < 0 || r.kv_head >= KVC) { fail("rows: kv_head outside the ring"); return false; }
        if (r.valid_len < 0 || (r.cc_par != 0 && r.cc_par != 1)) { fail("rows: valid_len < 0 or cc_par not 0 / 1"); return false; }
    }
    return true;
}

struct PostCase { int x, M, part, splits; float scale; int ln1_w, ln1_b, ln_out, ln2_w, ln2_b, a_out, act_bf16, copy_out; };
struct AttnCase { int q, kv_pool, n_slots, act_bf16, posproj, bias_u, bias_v, rows, B, T, TS, ctx_out; };
struct ConvCase { int glu, cc_pool, n_slots, dw, ln_w, ln_b, rows, B, T, ks, c_out, act_bf16, stream_form; };
struct FusedCase {
    int pro, M, N, K, splits, epi, ldo, ldo_act, T;
    int A, lda, W, out_f32, out_act, q_out, kv_pool, n_slots, rows;
    int x_in, x_out, part, part_splits; float scale; int lno_w, lno_b, ln_w, ln_b;
    AttnCase at;
    ConvCase cv;
};

bool attn_params(const AttnCase &c, AttnParams &a, int max_rows) {
    const int TS = c.TS > 0 ? c.TS : c.T, esz = c.act_bf16 ? 2 : 4;
    if (c.T < 1 || c.T > TMAX || TS > MAXNEW || TS % c.T || c.B < 1 || c.B * TS > max_rows) { fail("attention: T, TS or B outside the kernels' range"); return false; }
    const size_t M = (size_t)c.B * TS;
    if (!rows_ok(c.rows, c.B, c.n_slots, -1)) return false;
    if (!need(c.q, M * D * 4, "q") || !need(c.kv_pool, (size_t)c.n_slots * 2 * KVC * D * esz, "kv_pool") ||
        !need(c.posproj, (size_t)(LCTX + 2 * c.T - 1) * D * esz, "posproj") || !need(c.bias_u, D * 4, "bias_u") || !need(c.bias_v, D * 4, "bias_v") ||
        !need(c.ctx_out, M * D * esz, "ctx_out", true))
        return false;
    memset(&a, 0, sizeof(a));
    a.q = (const float *)ptr(c.q); a.kv_pool = ptr(c.kv_pool); a.kv_slot_stride = (int64_t)2 * KVC * D; a.act_bf16 = c.act_bf16;
    a.posproj = ptr(c.posproj); a.bias_u = (const float *)ptr(c.bias_u); a.bias_v = (const float *)ptr(c.bias_v);
    a.rows = (const RowDesc *)ptr(c.rows); a.B = c.B; a.T = c.T; a.TS = c.TS; a.ctx_out = ptr(c.ctx_out);
    return true;
}
bool conv_params(const ConvCase &c, ConvParams &p, int max_rows) {
    const int esz = c.act_bf16 ? 2 : 4;
    if (c.ks < 2 || c.ks > MAX_KS || c.T < 1 || c.T > MAXNEW || c.B < 1 || (long long)c.B * c.T > max_rows) { fail("dwconv: ks, T or B outside the kernels' range"); return false; }
    const size_t M = (size_t)c.B * c.T;
    if (!rows_ok(c.rows, c.B, -1, c.n_slots)) return false;
    if (!need(c.glu, M * D * 4, "glu") || !need(c.cc_pool, (size_t)c.n_slots * 2 * (c.ks - 1) * D * 4, "cc_pool") || !need(c.dw, (size_t)c.ks * D * 4, "dw") ||
        !need(c.ln_w, D * 4, "ln_w") || !need(c.ln_b, D * 4, "ln_b") || !need(c.c_out, M * D * esz, "c_out", true))
        return false;
    memset(&p, 0, sizeof(p));
    p.glu = (const float *)ptr(c.glu); p.cc_pool = (float *)ptr(c.cc_pool); p.cc_slot_stride = (int64_t)2 * (c.ks - 1) * D; p.dw = (const float *)ptr(c.dw);
    p.ln_w = (const float *)ptr(c.ln_w); p.ln_b = (const float *)ptr(c.ln_b); p.rows = (const RowDesc *)ptr(c.rows); p.B = c.B; p.T = c.T; p.ks = c.ks;
    p.c_out = ptr(c.c_out); p.act_bf16 = c.act_bf16; p.stream_form = c.stream_form;
    return true;
}
bool fused_params(const FusedCase &c, FusedParams &f, int max_m) {
    if (c.M < 1 || c.M > max_m || c.N < 16 || c.N % 16 || c.K < 32 || c.splits < 1 || c.splits > 8 || c.K % (32 * c.splits) || c.K / c.splits > 1024) {
        fail("fused: M, N, K or splits outside the kernel's range (M <= 16, N % 16, K % (32 splits), K / splits <= 1024)");
        return false;
    }
    if (c.pro != PRO_PLAIN && c.K != D) { fail("fused: the prologues produce 1024 columns"); return false; }
    if (c.pro == PRO_ATTN && (c.splits != NH || c.N % 128 || c.M > FUSE_MAX_M)) { fail("fused attention: splits = 8 heads, N % 128, M <= 2"); return false; }
    memset(&f, 0, sizeof(f));
    GemmParams &g = f.g;
    const size_t M = c.M;
    g.M = c.M; g.N = c.N; g.K = c.K; g.lda = c.lda; g.splits = c.splits; g.epi = c.epi; g.ldo = c.ldo; g.ldo_act = c.ldo_act; g.T = c.T;
    if (!need(c.W, (size_t)c.N * c.K * 2, "W")) return false;
    g.W = ptr(c.W);
    switch (c.epi) {
    case EPI_PART_F32:
        if (c.ldo < c.N || c.ldo % 4 || !need(c.out_f32, (size_t)c.splits * M * c.ldo * 4, "out_f32")) { if (c.ldo < c.N || c.ldo % 4) fail("fused: ldo"); return false; }
        break;
    case EPI_SILU_ACT:
        if (c.splits != 1 || c.ldo_act < c.N || c.ldo_act % 4 || !need(c.out_act, M * c.ldo_act * 2, "out_act")) { if (!g_err[0]) fail("fused: SILU needs splits = 1 and ldo_act >= N"); return false; }
        break;
    case EPI_GLU:
        if (c.splits != 1 || c.ldo < c.N / 2 || c.ldo % 2 || !need(c.out_f32, M * c.ldo * 4, "out_f32")) { if (!g_err[0]) fail("fused: GLU needs splits = 1 and ldo >= N / 2"); return false; }
        break;
    case EPI_QKV:
        if (c.splits != 1 || c.N != 3 * D || c.T < 1 || c.M % c.T) { fail("fused: QKV needs splits = 1, N = 3072, M % T = 0"); return false; }
        if (!rows_ok(c.rows, c.M / c.T, c.n_slots, -1)) return false;
        if (!need(c.q_out, M * D * 4, "q_out") || !need(c.kv_pool, (size_t)c.n_slots * 2 * KVC * D * 2, "kv_pool")) return false;
        if (c.T > MAXNEW) { fail("fused: T"); return false; }
        break;
    default:
        fail("fused: epilogue not offered by the harness");
        return false;
    }
    g.out_f32 = (float *)ptr(c.out_f32); g.out_act = ptr(c.out_act); g.q_out = (float *)ptr(c.q_out); g.kv_pool = ptr(c.kv_pool);
    g.kv_slot_stride = (int64_t)2 * KVC * D; g.rows = (const RowDesc *)ptr(c.rows);
    f.pro = c.pro;
    switch (c.pro) {
    case PRO_PLAIN:
        if (c.lda < c.K || c.lda % 8 || !need(c.A, M * c.lda * 2, "A")) { if (!g_err[0]) fail("fused: lda"); return false; }
        g.A = ptr(c.A);
        break;
    case PRO_LN:
        if (c.part_splits < 0 || c.part_splits > 8) { fail("fused: part_splits"); return false; }
        if (!need(c.x_in, M * D * 4, "x_in") || !need(c.x_out, M * D * 4, "x_out", true) || !need(c.part, (size_t)c.part_splits * M * D * 4, "part", c.part_splits == 0) ||
            !need(c.ln_w, D * 4, "ln_w") || !need(c.ln_b, D * 4, "ln_b") || !need(c.lno_w, D * 4, "lno_w", true) || !need(c.lno_b, D * 4, "lno_b", c.lno_w < 0))
            return false;
        f.x_in = (const float *)ptr(c.x_in); f.x_out = (float *)ptr(c.x_out); f.part = (const float *)ptr(c.part); f.part_splits = c.part_splits; f.scale = c.scale;
        f.lno_w = (const float *)ptr(c.lno_w); f.lno_b = (const float *)ptr(c.lno_b); f.ln_w = (const float *)ptr(c.ln_w); f.ln_b = (const float *)ptr(c.ln_b);
        break;
    case PRO_ATTN: {
        const int TS = c.at.TS > 0 ? c.at.TS : c.at.T;
        if (!c.at.act_bf16 || c.at.B * TS != c.M) { fail("fused attention: bf16 caches, B x TS = M"); return false; }
        if (!attn_params(c.at, f.at, FUSE_MAX_M)) return false;
    } break;
    case PRO_DWCONV:
        if (c.cv.B * c.cv.T != c.M) { fail("fused dwconv: B x T = M"); return false; }
        if (!conv_params(c.cv, f.cv, 16)) return false;
        break;
    default:
        fail("fused: prologue");
        return false;
    }
    return true;
}

}  // namespace

extern "C" const char *layer_harness_error() { return g_err; }
extern "C" unsigned layer_harness_sentinel() { return SENTINEL; }
extern "C" int layer_harness_struct_bytes(int which) {
    return which == 0 ? (int)sizeof(PostCase) : which == 1 ? (int)sizeof(AttnCase) : which == 2 ? (int)sizeof(ConvCase) : which == 3 ? (int)sizeof(FusedCase) : (int)sizeof(RowDesc);
}
extern "C" int layer_harness_constant(int which) {
    const int v[] = {D, NH, DH, LCTX, TMAX, MAXNEW, KVC, MAX_KS, FUSE_MAX_M, FUSED_GROUP};
    return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : -1;
}

extern "C" int layer_harness_init(int device) {
    g_err[0] = 0;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail("hipSetDevice", e);
    static bool attrs = false;
    if (!attrs) { init_fused_kernel_attributes(); attrs = true; }
    return 0;
}
// a new buffer [guard | body | guard], all of it SENTINEL; returns its handle or -1
extern "C" int layer_harness_alloc(long long body_bytes, int guard_bytes) {
    g_err[0] = 0;
    if (body_bytes < 0 || guard_bytes < 0 || (guard_bytes & 255)) return fail("alloc: sizes");
    Buf b;
    b.body = ((size_t)body_bytes + 255) & ~(size_t)255;
    b.guard = guard_bytes;
    hipError_t e = hipMalloc((void **)&b.base, b.total());
    if (e != hipSuccess) return fail("hipMalloc", e);
    std::vector<uint16_t> fill(b.total() / 2, SENTINEL);
    e = hipMemcpy(b.base, fill.data(), b.total(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(b.base); return fail("hipMemcpy (sentinel fill)", e); }
    g_bufs.push_back(b);
    return (int)g_bufs.size() - 1;
}
extern "C" long long layer_harness_total_bytes(int h) { const Buf *b = buf(h); return b ? (long long)b->total() : -1; }
extern "C" int layer_harness_put(int h, long long off, const void *src, long long bytes) {
    g_err[0] = 0;
    const Buf *b = buf(h);
    if (!b || off < 0 || bytes < 0 || (size_t)(off + bytes) > b->body) return fail("put: outside the body");
    hipError_t e = hipMemcpy((char *)b->ptr() + off, src, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : fail("hipMemcpy (upload)", e);
}
// the whole buffer, guards included: dst holds layer_harness_total_bytes(h)
extern "C" int layer_harness_get(int h, void *dst) {
    g_err[0] = 0;
    const Buf *b = buf(h);
    if (!b) return fail("get: handle");
    hipError_t e = hipMemcpy(dst, b->base, b->total(), hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : fail("hipMemcpy (download)", e);
}
extern "C" void layer_harness_free_all() {
    for (Buf &b : g_bufs)
        if (b.base) (void)hipFree(b.base);
    g_bufs.clear();
}
extern "C" int layer_harness_to_bf16(int src, int dst, long long n) {
    g_err[0] = 0;
    if (n < 1 || !need(src, (size_t)n * 4, "to_bf16 src") || !need(dst, (size_t)n * 2, "to_bf16 dst")) return -1;
    launch_f32_to_bf16((const float *)ptr(src), (bf16_t *)ptr(dst), (int64_t)n, 0);
    return sync_check();
}
extern "C" int layer_harness_pack_weight(int src, int dst, int N, int K) {
    g_err[0] = 0;
    if (N < 16 || N % 16 || K < 32 || K % 32) return fail("pack_weight: N % 16, K % 32");
    if (!need(src, (size_t)N * K * 4, "pack src") || !need(dst, (size_t)N * K * 2, "pack dst")) return -1;
    launch_pack_weight_bf16((const float *)ptr(src), (bf16_t *)ptr(dst), N, K, 0);
    return sync_check();
}

extern "C" int layer_harness_post(const PostCase *c) {
    g_err[0] = 0;
    const size_t M = c->M;
    if (c->M < 1 || c->M > 4096 || c->splits < 0 || c->splits > 8) return fail("post: M or splits outside the kernel's range");
    const int esz = c->act_bf16 ? 2 : 4;
    const bool ln2 = c->ln2_w >= 0;
    if (!need(c->x, M * D * 4, "x") || !need(c->part, (size_t)c->splits * M * D * 4, "part", c->splits == 0) || !need(c->ln1_w, D * 4, "ln1_w", !c->ln_out) ||
        !need(c->ln1_b, D * 4, "ln1_b", !c->ln_out) || !need(c->ln2_w, D * 4, "ln2_w", true) || !need(c->ln2_b, D * 4, "ln2_b", !ln2) ||
        !need(c->a_out, M * D * esz, "a_out", !ln2) || !need(c->copy_out, M * D * 4, "copy_out", true))
        return -1;
    PostParams p;
    memset(&p, 0, sizeof(p));
    p.x = (float *)ptr(c->x); p.M = c->M; p.part = (const float *)ptr(c->part); p.splits = c->splits; p.scale = c->scale;
    p.ln1_w = (const float *)ptr(c->ln1_w); p.ln1_b = (const float *)ptr(c->ln1_b); p.ln_out = c->ln_out;
    p.ln2_w = (const float *)ptr(c->ln2_w); p.ln2_b = (const float *)ptr(c->ln2_b); p.a_out = ptr(c->a_out); p.act_bf16 = c->act_bf16;
    p.copy_out = (float *)ptr(c->copy_out);
    launch_post(p, 0);
    return sync_check();
}
extern "C" int layer_harness_attention(const AttnCase *c) {
    g_err[0] = 0;
    AttnParams a;
    if (c->ctx_out < 0) return fail("attention: ctx_out");
    if (!attn_params(*c, a, 1 << 20)) return -1;
    launch_attention(a, 0);
    return sync_check();
}
extern "C" int layer_harness_dwconv(const ConvCase *c) {
    g_err[0] = 0;
    ConvParams p;
    if (c->c_out < 0) return fail("dwconv: c_out");
    if (!conv_params(*c, p, 1 << 20)) return -1;
    launch_dwconv(p, 0);
    return sync_check();
}
// n = 1, grouped = 0: launch_fused_skinny.  grouped = 1: launch_fused_skinny_group of n <= FUSED_GROUP problems of one kind (M <= 2); a case with M = 0 is a skipped
// problem: its FusedParams hold its buffers all the same, so that a kernel that did not skip it would show in them
extern "C" int layer_harness_fused(const FusedCase *cs, int n, int grouped) {
    g_err[0] = 0;
    if (n < 1 || n > FUSED_GROUP || (!grouped && n != 1)) return fail("fused: n");
    FusedParamsGroup *pp = new FusedParamsGroup;
    memset(pp, 0, sizeof(*pp));
    int first = -1, rc = 0;
    for (int i = 0; i < n && !rc; i++) {
        FusedCase c = cs[i];
        const bool skipped = grouped && c.M == 0;
        if (skipped) {
            if (first < 0) { rc = fail("fused group: the first problem must be live"); break; }
            c.M = cs[first].M;
            if (c.pro == PRO_ATTN) { c.at.B = cs[first].at.B; c.at.T = cs[first].at.T; c.at.TS = cs[first].at.TS; }
            if (c.pro == PRO_DWCONV) { c.cv.B = cs[first].cv.B; c.cv.T = cs[first].cv.T; }
        }
        if (!fused_params(c, pp->p[i], grouped ? FUSE_MAX_M : 16)) { rc = -1; break; }
        if (skipped) { pp->p[i].g.M = 0; continue; }
        if (first < 0) first = i;
        const FusedCase &f = cs[first];
        if (c.pro != f.pro || c.M != f.M || c.N != f.N || c.K != f.K || c.splits != f.splits || c.epi != f.epi) rc = fail("fused group: problems of different kinds");
    }
    if (!rc) {
        if (grouped) launch_fused_skinny_group(*pp, n, 0);
        else launch_fused_skinny(pp->p[0], 0);
        rc = sync_check();
    }
    delete pp;
    return rc;
}
