// Test helper (not product code): ONE launch of kernels_offline.hip through its launcher, on buffers with guard regions, for
// tests/test_gpu_offline_kernels.py.
//   hipcc --offload-arch=gfx950 -O2 -shared -fPIC -I../../nemotron-asr.cpp_amd/csrc -o liboffline_harness.so offline_harness.hip   (built by __graft_entry__.build())
//
// No kernel of its own: nasr::launch_off_attention / launch_off_dwconv / launch_off_conv0_dw / launch_off_window / launch_off_dec_reset,
// off_attn_qb and launch_f32_to_bf16 are the product's, resolved from libnemotron_asr_amd.so (the test loads that library with RTLD_GLOBAL
// before this one).
//
// The buffer plumbing is layer_harness.hip's: the test allocates device buffers by handle, each [guard | body | guard] and all of it the
// 16-bit pattern SENTINEL, uploads its inputs into the bodies -- poison included -- and gets every buffer back whole.  The launch entries
// take handles.  Before anything is launched they check the shapes against the kernels' limits (T <= OFFLINE_MAX_T, ks <= MAX_KS,
// off + T <= M), every buffer's body against the bytes the launch addresses, and every descriptor against the buffers it indexes (the
// attention items, tpos, OffSubDesc, the window int4): a case the kernels' indexing does not cover is an error, never a launch.
#include "nasr_offline.h"
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
// handle h holds at least `bytes` in its body
bool need(int h, size_t bytes, const char *name) {
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
// the n descriptors of handle h (its body holds them: checked by the caller)
template <typename T>
bool fetch(int h, int n, std::vector<T> &out, const char *name) {
    out.resize(n);
    if (n > 0 && hipMemcpy(out.data(), ptr(h), (size_t)n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: download", name);
        return false;
    }
    return true;
}

struct AttnCase { int qkv, pos, bias_u, bias_v, items, n_items, ctx, M, act_bf16; };
struct ConvCase { int glu, tpos, M, dw, ks, ln_w, ln_b, out, act_bf16; };
struct SubCase { int desc, B, max_h2, mel, mel_rows, w0t, b0, w2t, b2, out, out_rows, out_bf16; };
struct WinCase { int encproj, rows, win, B, W, out; };
struct ResetCase { int B, h, c, ctrl; };

}  // namespace

extern "C" const char *offline_harness_error() { return g_err; }
extern "C" unsigned offline_harness_sentinel() { return SENTINEL; }
extern "C" int offline_harness_struct_bytes(int which) {
    const int v[] = {(int)sizeof(AttnCase), (int)sizeof(ConvCase), (int)sizeof(SubCase), (int)sizeof(WinCase), (int)sizeof(ResetCase),
                     (int)sizeof(OffSubDesc), (int)sizeof(DecCtrl), (int)sizeof(int4)};
    return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : -1;
}
extern "C" int offline_harness_constant(int which) {
    const int v[] = {D, NH, DH, OFFLINE_MAX_T, OFFLINE_NREL, OFF_QKV_LD, MAX_KS, SUBC, NMEL, JNT, HID, BLANK, OFF_DEC_WIN};
    return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : -1;
}
// query rows per attention workgroup: the driver's item stride
extern "C" int offline_harness_attn_qb(int act_bf16) { return off_attn_qb(act_bf16); }

extern "C" int offline_harness_init(int device) {
    g_err[0] = 0;
    hipError_t e = hipSetDevice(device);
    return e == hipSuccess ? 0 : fail("hipSetDevice", e);
}
// a new buffer [guard | body | guard], all of it SENTINEL; returns its handle or -1
extern "C" int offline_harness_alloc(long long body_bytes, int guard_bytes) {
    g_err[0] = 0;
    if (body_bytes < 0 || guard_bytes < 256 || (guard_bytes & 255)) return fail("alloc: sizes");
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
extern "C" long long offline_harness_total_bytes(int h) { const Buf *b = buf(h); return b ? (long long)b->total() : -1; }
extern "C" int offline_harness_put(int h, long long off, const void *src, long long bytes) {
    g_err[0] = 0;
    const Buf *b = buf(h);
    if (!b || off < 0 || bytes < 0 || (size_t)(off + bytes) > b->body) return fail("put: outside the body");
    if (bytes == 0) return 0;
    hipError_t e = hipMemcpy((char *)b->ptr() + off, src, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : fail("hipMemcpy (upload)", e);
}
// the whole buffer, guards included: dst holds offline_harness_total_bytes(h)
extern "C" int offline_harness_get(int h, void *dst) {
    g_err[0] = 0;
    const Buf *b = buf(h);
    if (!b) return fail("get: handle");
    hipError_t e = hipMemcpy(dst, b->base, b->total(), hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : fail("hipMemcpy (download)", e);
}
extern "C" void offline_harness_free_all() {
    for (Buf &b : g_bufs)
        if (b.base) (void)hipFree(b.base);
    g_bufs.clear();
}
extern "C" int offline_harness_to_bf16(int src, int dst, long long n) {
    g_err[0] = 0;
    if (n < 1 || !need(src, (size_t)n * 4, "to_bf16 src") || !need(dst, (size_t)n * 2, "to_bf16 dst")) return n < 1 ? fail("to_bf16: n") : -1;
    launch_f32_to_bf16((const float *)ptr(src), (bf16_t *)ptr(dst), (int64_t)n, 0);
    return sync_check();
}

// k_off_attn_bf16 / k_off_attn_f32.  An item (off, T, q0, -) addresses rows off .. off + T - 1 of qkv (the kernels clamp their query and key rows
// to T - 1) and writes ctx rows off + q0 .. below off + T; with q0 a multiple of the workgroup's query rows and below T <= 2048, every
// position-table row either kernel forms lies in [0, 4094] (the bf16 kernel clamps band row 79 to 4094).
extern "C" int offline_harness_attention(const AttnCase *c) {
    g_err[0] = 0;
    const size_t esz = c->act_bf16 ? 2 : 4;
    if (c->M < 1 || c->n_items < 1 || c->n_items > 65535) return fail("attention: M or n_items outside the launch's range");
    if (!need(c->qkv, (size_t)c->M * OFF_QKV_LD * esz, "qkv") || !need(c->pos, (size_t)OFFLINE_NREL * D * esz, "pos") || !need(c->bias_u, D * 4, "bias_u") ||
        !need(c->bias_v, D * 4, "bias_v") || !need(c->items, (size_t)c->n_items * sizeof(int4), "items") || !need(c->ctx, (size_t)c->M * D * esz, "ctx"))
        return -1;
    std::vector<int4> items;
    if (!fetch(c->items, c->n_items, items, "attention items")) return -1;
    const int qb = off_attn_qb(c->act_bf16);
    for (const int4 &it : items) {
        if (it.y < 1 || it.y > OFFLINE_MAX_T) return fail("attention item: T outside 1 .. OFFLINE_MAX_T");
        if (it.x < 0 || (long long)it.x + it.y > c->M) return fail("attention item: off + T > M");
        if (it.z < 0 || it.z >= it.y || it.z % qb) return fail("attention item: first query row not a multiple of the workgroup's rows below T");
    }
    OffAttnParams p;
    p.qkv = ptr(c->qkv); p.pos = ptr(c->pos); p.bias_u = (const float *)ptr(c->bias_u); p.bias_v = (const float *)ptr(c->bias_v);
    p.items = (const int4 *)ptr(c->items); p.ctx = ptr(c->ctx);
    launch_off_attention(p, c->n_items, c->act_bf16, 0);
    return sync_check();
}

// k_off_dwconv: row m reads rows m - min(tpos[m], ks - 1) .. m of glu
extern "C" int offline_harness_dwconv(const ConvCase *c) {
    g_err[0] = 0;
    if (c->M < 1 || c->ks < 1 || c->ks > MAX_KS) return fail("dwconv: M or ks outside the kernel's range (1 <= ks <= MAX_KS)");
    const size_t M = c->M;
    if (!need(c->glu, M * D * 4, "glu") || !need(c->tpos, M * 4, "tpos") || !need(c->dw, (size_t)c->ks * D * 4, "dw") || !need(c->ln_w, D * 4, "ln_w") ||
        !need(c->ln_b, D * 4, "ln_b") || !need(c->out, M * D * (c->act_bf16 ? 2 : 4), "out"))
        return -1;
    std::vector<int> tpos;
    if (!fetch(c->tpos, c->M, tpos, "dwconv tpos")) return -1;
    for (int m = 0; m < c->M; m++)
        if (tpos[m] < 0 || tpos[m] > m || tpos[m] >= OFFLINE_MAX_T) return fail("dwconv tpos: a frame index outside 0 .. min(m, OFFLINE_MAX_T - 1)");
    launch_off_dwconv((const float *)ptr(c->glu), (const int *)ptr(c->tpos), c->M, (const float *)ptr(c->dw), c->ks, (const float *)ptr(c->ln_w),
                      (const float *)ptr(c->ln_b), ptr(c->out), c->act_bf16, 0);
    return sync_check();
}

// k_off_conv0_dw<OUT_BF16>: utterance b reads mel rows mel_off .. mel_off + n_mel - 1 and writes out rows out_row .. out_row + min(H2, max_h2) - 1
extern "C" int offline_harness_conv0_dw(const SubCase *c) {
    g_err[0] = 0;
    if (c->B < 1 || c->B > 65535 || c->max_h2 < 0 || c->max_h2 > 65535 || c->mel_rows < 0 || c->out_rows < 0) return fail("conv0_dw: B, max_h2 or rows outside the launch's range");
    if (!need(c->desc, (size_t)c->B * sizeof(OffSubDesc), "desc") || !need(c->mel, (size_t)c->mel_rows * NMEL * 4, "mel") || !need(c->w0t, 9 * SUBC * 4, "w0t") ||
        !need(c->b0, SUBC * 4, "b0") || !need(c->w2t, 9 * SUBC * 4, "w2t") || !need(c->b2, SUBC * 4, "b2") ||
        !need(c->out, (size_t)c->out_rows * 33 * SUBC * (c->out_bf16 ? 2 : 4), "out"))
        return -1;
    std::vector<OffSubDesc> sd;
    if (!fetch(c->desc, c->B, sd, "conv0_dw desc")) return -1;
    for (const OffSubDesc &d : sd) {
        if (d.n_mel <= 0) continue;                                // the kernel returns before it forms an address
        if (d.n_mel > 8 * OFFLINE_MAX_T) return fail("conv0_dw desc: n_mel above the offline limit");
        if (d.mel_off < 0 || (long long)d.mel_off + d.n_mel > c->mel_rows) return fail("conv0_dw desc: mel rows outside the buffer");
        const int h2 = nasr_plan::sub_h2(d.n_mel), rows = h2 < c->max_h2 ? h2 : c->max_h2;
        if (d.out_row < 0 || (long long)d.out_row + rows > c->out_rows) return fail("conv0_dw desc: output rows outside the buffer");
    }
    launch_off_conv0_dw((const OffSubDesc *)ptr(c->desc), c->B, c->max_h2, (const float *)ptr(c->mel), (const float *)ptr(c->w0t), (const float *)ptr(c->b0),
                        (const float *)ptr(c->w2t), (const float *)ptr(c->b2), ptr(c->out), c->out_bf16, 0);
    return sync_check();
}

// k_off_window: utterance b copies rows win.x .. win.x + min(win.y, W) - 1 of encproj [rows][640] into out [b][W][640]
extern "C" int offline_harness_window(const WinCase *c) {
    g_err[0] = 0;
    if (c->B < 1 || c->B > 65535 || c->W < 1 || c->W > 65535 || c->rows < 0) return fail("window: B, W or rows outside the launch's range");
    if (!need(c->encproj, (size_t)c->rows * JNT * 4, "encproj") || !need(c->win, (size_t)c->B * sizeof(int4), "win") || !need(c->out, (size_t)c->B * c->W * JNT * 4, "out"))
        return -1;
    std::vector<int4> win;
    if (!fetch(c->win, c->B, win, "window int4")) return -1;
    for (const int4 &w : win) {
        const int n = w.y < c->W ? w.y : c->W;
        if (n > 0 && (w.x < 0 || (long long)w.x + n > c->rows)) return fail("window int4: source rows outside encproj");
    }
    launch_off_window((const float *)ptr(c->encproj), (const int4 *)ptr(c->win), c->B, c->W, (float *)ptr(c->out), 0);
    return sync_check();
}

// k_off_dec_reset: slots 0 .. B - 1 of h, c [slot][4 x 640] and of ctrl
extern "C" int offline_harness_dec_reset(const ResetCase *c) {
    g_err[0] = 0;
    if (c->B < 1 || c->B > 65535) return fail("dec_reset: B outside the launch's range");
    if (!need(c->h, (size_t)c->B * 4 * HID * 4, "h") || !need(c->c, (size_t)c->B * 4 * HID * 4, "c") || !need(c->ctrl, (size_t)c->B * sizeof(DecCtrl), "ctrl")) return -1;
    launch_off_dec_reset(c->B, (float *)ptr(c->h), (float *)ptr(c->c), (DecCtrl *)ptr(c->ctrl), 0);
    return sync_check();
}
