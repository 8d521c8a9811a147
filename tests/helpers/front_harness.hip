// Test helper (not product code): ONE launcher call of the front-end kernels (kernels_front.hip) on buffers with guard regions, for tests/test_gpu_front_kernels.py.
//   hipcc --offload-arch=gfx950 -O2 -shared -fPIC -I../../nemotron-asr.cpp_amd/csrc -I../../include -o libfront_harness.so front_harness.hip   (built by __graft_entry__.build())
//
// The kernels are the product's, reached through its launchers -- launch_mel, launch_mel_put, launch_mel_zero, launch_stream_reset, launch_stream_fork,
// launch_stream_pack, launch_stream_unpack, launch_sub_conv0_dw, launch_sub_dw, launch_diar_logmel, launch_diar_frames -- resolved from libnemotron_asr_amd.so (the
// test loads that library with RTLD_GLOBAL before this one).  The one kernel of its own, k_libm, applies the device logf to an array; it serves only to measure
// logf against float64 (as decode_harness.hip's k_libm does for expf and tanhf).
//
// The buffer plumbing is the other harnesses': buffers by handle, each [guard | body | guard] and all of it the 16-bit pattern SENTINEL; the test uploads its inputs
// into the bodies and gets every buffer back whole.  Descriptor tables that hold device addresses (PcmDesc, StreamForkPiece, the pool pointer arrays of a reset) are
// built here from handles and offsets and uploaded into a buffer of the test's.  Before anything is launched every entry checks the case against the bytes the
// launch addresses: every buffer's body, every slot, ring position, count and offset a kernel indexes with, the band table's entries, the pieces of a copy plan
// (inside their buffers, destinations disjoint).  A case that fails a check is an error (-1 and a reason), never a launch.
#include "nasr_internal.h"
#include "nasr_constants.h"
#include "nasr_conv0_dw.h"
#include "nasr_decode_set.h"
#include "nasr_fork_plan.h"
#include "nasr_snapshot.h"
#include "nasr_lm.h"
#include "nasr_resample.h"
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
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
template <typename T> bool upload(int h, const std::vector<T> &v, const char *name) {
    if (!need(h, v.size() * sizeof(T), name)) return false;
    if (!v.empty() && hipMemcpy(ptr(h), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { herr("descriptor table: upload"); return false; }
    return true;
}
// the band table [n_mel][2] on the device: 0 <= lo <= hi <= NBINS for every filter
bool band_ok(int h, int n_mel) {
    if (!need(h, (size_t)n_mel * 8, "fb_band")) return false;
    std::vector<int> b(2 * n_mel);
    if (hipMemcpy(b.data(), ptr(h), b.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { herr("fb_band: download"); return false; }
    for (int m = 0; m < n_mel; m++)
        if (b[2 * m] < 0 || b[2 * m] > b[2 * m + 1] || b[2 * m + 1] > NBINS) { herr("fb_band: an entry outside 0 <= lo <= hi <= 257"); return false; }
    return true;
}
bool mel_tables_ok(int window, int fbT, int band, int cos_t, int sin_t, int n_mel) {
    return need(window, NFFT * 4, "window") && need(fbT, (size_t)NBINS * n_mel * 4, "fbT") && band_ok(band, n_mel) && need(cos_t, NFFT * 4, "cos_t") && need(sin_t, NFFT * 4, "sin_t");
}

__global__ void k_libm(const float *x, float *y, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = logf(x[i]);
}

}  // namespace

extern "C" const char *front_harness_error() { return g_err; }
extern "C" unsigned front_harness_sentinel() { return SENTINEL; }
extern "C" int front_harness_constant(int which) {
    const int v[] = {NMEL, NBINS, NFFT, HOP, MEL_RING, ABUF_CAP, KVC, LCTX, D, HID, PRE_CACHE, SUBC, DIAR_NMEL, nasr_rs::HIST_MAX, BLANK,
                     (int)sizeof(PcmDesc), (int)sizeof(RowDesc), (int)sizeof(StreamForkPiece), (int)sizeof(DecCtrl), (int)sizeof(DiarFrameDesc),
                     (int)sizeof(nasr_lm::Greedy), (int)offsetof(nasr_lm::Greedy, attached), (int)(offsetof(nasr_lm::Greedy, lm) + offsetof(nasr_lm::View, start))};
    return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : -1;
}

extern "C" int front_harness_init(int device) {
    g_err[0] = 0;
    hipError_t e = hipSetDevice(device);
    return e == hipSuccess ? 0 : herr("hipSetDevice", e);
}
extern "C" int front_harness_alloc(long long body_bytes, int guard_bytes) {
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
extern "C" long long front_harness_total_bytes(int h) { const Buf *b = buf(h); return b ? (long long)b->total() : -1; }
extern "C" int front_harness_put(int h, long long off, const void *src, long long bytes) {
    g_err[0] = 0;
    const Buf *b = buf(h);
    if (!b || off < 0 || bytes < 0 || (size_t)(off + bytes) > b->body) return herr("put: outside the body");
    if (bytes == 0) return 0;
    hipError_t e = hipMemcpy((char *)b->ptr() + off, src, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : herr("hipMemcpy (upload)", e);
}
extern "C" int front_harness_get(int h, void *dst) {
    g_err[0] = 0;
    const Buf *b = buf(h);
    if (!b) return herr("get: handle");
    hipError_t e = hipMemcpy(dst, b->base, b->total(), hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : herr("hipMemcpy (download)", e);
}
extern "C" void front_harness_free_all() {
    for (Buf &b : g_bufs)
        if (b.base) (void)hipFree(b.base);
    g_bufs.clear();
}

// ---- launch_mel: k_preemph, k_melframes, k_abuf_shift ----------------------------------------------------------------------------------------------------
// a: desc table, pcm, B, max_frames, abuf, last_sample, mel_ring, window, fbT, fb_band, cos_t, sin_t, tap (-1: null), tap_cap, max_n, n_slots;
// d [B][8]: offset into pcm (samples), slot, n, cnt, par, n_frames, mel_wpos, consumed
extern "C" int front_harness_mel(const int *a, const int *d) {
    g_err[0] = 0;
    const int B = a[2], max_frames = a[3], tap = a[12], tap_cap = a[13], max_n = a[14], n_slots = a[15];
    if (B < 1 || B > 1024 || max_frames < 0 || max_frames > 4096 || n_slots < 1 || n_slots > 64 || max_n < 1) return herr("mel: B, max_frames, n_slots or max_n outside the harness's range");
    if (!need(a[4], (size_t)n_slots * 2 * ABUF_CAP * 4, "abuf") || !need(a[5], (size_t)n_slots * 4, "last_sample") || !need(a[6], (size_t)n_slots * MEL_RING * NMEL * 4, "mel_ring") ||
        !mel_tables_ok(a[7], a[8], a[9], a[10], a[11], NMEL))
        return -1;
    if (tap >= 0 && (tap_cap < 1 || !need(tap, (size_t)B * tap_cap * NMEL * 4, "tap"))) return g_err[0] ? -1 : herr("mel: tap_cap < 1");
    const Buf *pb = buf(a[1]);
    if (!pb) return herr("mel: pcm handle");
    std::vector<PcmDesc> t(B);
    std::vector<char> seen(n_slots, 0);
    for (int b = 0; b < B; b++) {
        const int *x = d + 8 * b;
        const int off = x[0], slot = x[1], n = x[2], cnt = x[3], par = x[4], nf = x[5], wpos = x[6], consumed = x[7];
        if (slot < 0 || slot >= n_slots || seen[slot]) return herr("mel: a slot outside the pool, or named twice");
        seen[slot] = 1;
        if (n < 0 || cnt < 0 || (par != 0 && par != 1)) return herr("mel: n, cnt or par");
        if ((long long)cnt + n > ABUF_CAP) return herr("mel: cnt + n > ABUF_CAP");
        if (off < 0 || ((size_t)off + n) * 2 > pb->body) return herr("mel: the samples of a descriptor leave the pcm buffer");
        if (nf < 0 || nf > max_frames) return herr("mel: n_frames outside 0 .. max_frames");
        if (nf > 0 && (long long)(nf - 1) * HOP + NFFT > (long long)cnt + n) return herr("mel: n_frames larger than the samples allow");
        if (consumed != nf * HOP) return herr("mel: consumed != n_frames * HOP");
        if (wpos < 0 || wpos >= MEL_RING) return herr("mel: mel_wpos outside the ring");
        memset(&t[b], 0, sizeof(PcmDesc));
        t[b].pcm = (const int16_t *)pb->ptr() + off; t[b].slot = slot; t[b].n = n; t[b].cnt = cnt; t[b].par = par;
        t[b].n_frames = nf; t[b].mel_wpos = wpos; t[b].consumed = consumed;
    }
    if (!upload(a[0], t, "desc")) return -1;
    MelParams p;
    memset(&p, 0, sizeof(p));
    p.desc = ptr<PcmDesc>(a[0]); p.B = B; p.max_frames = max_frames;
    p.abuf = ptr<float>(a[4]); p.last_sample = ptr<float>(a[5]); p.mel_ring = ptr<float>(a[6]);
    p.window = ptr<float>(a[7]); p.fbT = ptr<float>(a[8]); p.fb_band = ptr<int>(a[9]); p.cos_t = ptr<float>(a[10]); p.sin_t = ptr<float>(a[11]);
    p.tap = tap >= 0 ? ptr<float>(tap) : nullptr; p.tap_cap = tap_cap;
    launch_mel(p, max_n, 0);
    return sync_check();
}

// which 0: launch_mel_put, 1: launch_mel_zero.  d [B][3]: slot, n_frames, mel_wpos
extern "C" int front_harness_mel_ring(int which, int staged, int desc, int mel_ring, int B, int max_frames, int n_slots, const int *d) {
    g_err[0] = 0;
    if (B < 1 || B > 1024 || max_frames < 0 || max_frames > 4096 || n_slots < 1 || n_slots > 64) return herr("mel_ring: B, max_frames or n_slots outside the harness's range");
    if (!need(mel_ring, (size_t)n_slots * MEL_RING * NMEL * 4, "mel_ring")) return -1;
    if (which == 0 && !need(staged, (size_t)B * max_frames * NMEL * 4, "staged")) return -1;
    std::vector<PcmDesc> t(B);
    std::vector<char> seen(n_slots, 0);
    for (int b = 0; b < B; b++) {
        const int slot = d[3 * b], nf = d[3 * b + 1], wpos = d[3 * b + 2];
        if (slot < 0 || slot >= n_slots || seen[slot]) return herr("mel_ring: a slot outside the pool, or named twice");
        seen[slot] = 1;
        if (nf < 0 || nf > max_frames) return herr("mel_ring: n_frames outside 0 .. max_frames");
        if (wpos < 0 || wpos >= MEL_RING) return herr("mel_ring: mel_wpos outside the ring");
        memset(&t[b], 0, sizeof(PcmDesc));
        t[b].slot = slot; t[b].n_frames = nf; t[b].mel_wpos = wpos;
    }
    if (!upload(desc, t, "desc")) return -1;
    if (which == 0) launch_mel_put(ptr<float>(staged), ptr<PcmDesc>(desc), B, max_frames, ptr<float>(mel_ring), 0);
    else launch_mel_zero(ptr<PcmDesc>(desc), B, max_frames, ptr<float>(mel_ring), 0);
    return sync_check();
}

// ---- launch_stream_fork (which 0), launch_stream_pack (1), launch_stream_unpack (2) ------------------------------------------------------------------------
// pc [n][4]: offset into src, offset into dst, bytes, pad (the section index of the piece's first word; fork ignores it).  A piece moves as words when an address
// or its length is no multiple of 16; pack then writes, and unpack then reads, the piece padded to 16 bytes.
extern "C" int front_harness_pieces(int which, int tab, int src, int dst, int sums, const long long *pc, int n) {
    g_err[0] = 0;
    const Buf *sb = buf(src), *db = buf(dst);
    if (which < 0 || which > 2 || n < 0 || n > 4096) return herr("pieces: which or n");
    if (!sb || !db || src == dst) return herr("pieces: src and dst are two buffers");
    if (which != 0 && !need(sums, (size_t)n * 8, "sums")) return -1;
    std::vector<StreamForkPiece> t(n);
    std::vector<std::pair<long long, long long>> wr;
    for (int i = 0; i < n; i++) {
        const long long so = pc[4 * i], dof = pc[4 * i + 1], bytes = pc[4 * i + 2], pad = pc[4 * i + 3];
        if (so < 0 || dof < 0 || bytes < 4 || bytes > (1ll << 30) || (so & 3) || (dof & 3) || (bytes & 3) || pad < 0 || pad > 0x7fffffffll) return herr("pieces: offsets and lengths are multiples of 4, lengths positive");
        const bool words = ((so | dof | bytes) & 15) != 0;          // the buffers' bodies start on 256-byte boundaries
        const long long padded = (bytes + 15) / 16 * 16;
        const long long rd = words && which == 2 ? padded : bytes, wrn = words && which == 1 ? padded : bytes;
        if ((size_t)(so + rd) > sb->body || (size_t)(dof + wrn) > db->body) return herr("pieces: a piece leaves its buffer");
        wr.push_back({dof, dof + wrn});
        t[i].src = (const char *)sb->ptr() + so; t[i].dst = (char *)db->ptr() + dof; t[i].bytes = (uint32_t)bytes; t[i].pad = (uint32_t)pad;
    }
    std::sort(wr.begin(), wr.end());
    for (size_t i = 1; i < wr.size(); i++)
        if (wr[i].first < wr[i - 1].second) return herr("pieces: two pieces overlap in the destination");
    if (n > 0 && !upload(tab, t, "pieces")) return -1;
    if (which == 0) {
        StreamForkParams p{ptr<StreamForkPiece>(tab), n};
        launch_stream_fork(p, 0);
    } else {
        StreamPackParams p{ptr<StreamForkPiece>(tab), n, ptr<unsigned long long>(sums)};
        if (which == 1) launch_stream_pack(p, 0);
        else launch_stream_unpack(p, 0);
    }
    return sync_check();
}

// ---- launch_stream_reset -------------------------------------------------------------------------------------------------------------------------------------
// a: pointer table, kv [n_layers][n_slots][2][KVC][1024] esz, cc [n_layers][n_slots][cc_slot_floats], esz, kv_head, n_layers, slot, n_slots, cc_slot_floats,
// keep_reference_state, abuf, last_sample, mel_ring, dec_h, dec_c, ctrl, boost_state (-1), boost_init, lm_state (-1), lm_blk (-1), lm_enabled, aud_hist (-1)
extern "C" int front_harness_reset(const int *a) {
    g_err[0] = 0;
    const int esz = a[3], kv_head = a[4], nl = a[5], slot = a[6], ns = a[7], ccf = a[8];
    if ((esz != 2 && esz != 4) || kv_head < 0 || kv_head >= KVC || nl < 1 || nl > 64 || ns < 1 || ns > 64 || slot < 0 || slot >= ns || ccf < 4 || (ccf & 3) || ccf > (1 << 24))
        return herr("reset: esz 2 or 4, kv_head inside the ring, slot inside the pool, cc_slot_floats a multiple of 4");
    const size_t kv_layer = (size_t)ns * 2 * KVC * D * esz, cc_layer = (size_t)ns * ccf * 4;
    if (!need(a[1], nl * kv_layer, "kv") || !need(a[2], nl * cc_layer, "cc") || !need(a[10], (size_t)ns * 2 * ABUF_CAP * 4, "abuf") || !need(a[11], (size_t)ns * 4, "last_sample") ||
        !need(a[12], (size_t)ns * MEL_RING * NMEL * 4, "mel_ring") || !need(a[13], (size_t)ns * 4 * HID * 4, "dec_h") || !need(a[14], (size_t)ns * 4 * HID * 4, "dec_c") ||
        !need(a[15], (size_t)ns * sizeof(DecCtrl), "ctrl"))
        return -1;
    if (a[16] >= 0 && !need(a[16], (size_t)ns * 4, "boost_state")) return -1;
    if (a[18] >= 0 && (!need(a[18], (size_t)ns * 4, "lm_state") || !need(a[19], sizeof(nasr_lm::Greedy), "lm_blk"))) return -1;
    if (a[21] >= 0 && !need(a[21], (size_t)ns * 2 * nasr_rs::HIST_MAX * 4, "aud_hist")) return -1;
    std::vector<void *> tab(2 * nl);
    for (int l = 0; l < nl; l++) { tab[l] = ptr<char>(a[2]) + l * cc_layer; tab[nl + l] = ptr<char>(a[1]) + l * kv_layer; }
    if (!upload(a[0], tab, "pointer table")) return -1;
    StreamResetParams p;
    memset(&p, 0, sizeof(p));
    p.cc_pools = ptr<float *>(a[0]); p.kv_pools = ptr<void *>(a[0]) + nl;
    p.esz = esz; p.kv_head = kv_head; p.n_layers = nl; p.slot = slot; p.cc_slot_floats = ccf; p.keep_reference_state = a[9];
    p.abuf = ptr<float>(a[10]); p.last_sample = ptr<float>(a[11]); p.mel_ring = ptr<float>(a[12]); p.dec_h = ptr<float>(a[13]); p.dec_c = ptr<float>(a[14]);
    p.ctrl = ptr<DecCtrl>(a[15]);
    p.boost_state = a[16] >= 0 ? ptr<int>(a[16]) : nullptr; p.boost_init = a[17];
    p.lm_state = a[18] >= 0 ? ptr<int32_t>(a[18]) : nullptr; p.lm_blk = a[18] >= 0 ? ptr<nasr_lm::Greedy>(a[19]) : nullptr; p.lm_enabled = a[20];
    p.aud_hist = a[21] >= 0 ? ptr<float>(a[21]) : nullptr;
    launch_stream_reset(p, 0);
    return sync_check();
}

// ---- launch_sub_conv0_dw: rows [B][2] = slot, mel_start ------------------------------------------------------------------------------------------------------
extern "C" int front_harness_conv0(int rows_tab, int mel_ring, int w0t, int b0, int w2t, int b2, int out, int out_bf16, int B, int chunk_mel, int H1, int W1, int n_slots,
                                   const int *rows) {
    g_err[0] = 0;
    if (W1 != 65) return herr("conv0: W1 != 65 (the staged rows hold 4 * 33 + 12 columns)");
    if (B < 1 || B > 65535 || chunk_mel < 1 || chunk_mel > MEL_RING || H1 != chunk_mel / 2 + 1 || n_slots < 1 || n_slots > 64) return herr("conv0: B, chunk_mel, H1 = chunk_mel / 2 + 1 or n_slots");
    const int H2 = H1 / 2 + 1;
    if (!need(mel_ring, (size_t)n_slots * MEL_RING * NMEL * 4, "mel_ring") || !need(w0t, 9 * SUBC * 4, "w0t") || !need(b0, SUBC * 4, "b0") || !need(w2t, 9 * SUBC * 4, "w2t") ||
        !need(b2, SUBC * 4, "b2") || !need(out, (size_t)B * H2 * 33 * SUBC * (out_bf16 ? 2 : 4), "out"))
        return -1;
    std::vector<RowDesc> t(B);
    for (int b = 0; b < B; b++) {
        const int slot = rows[2 * b], ms = rows[2 * b + 1];
        if (slot < 0 || slot >= n_slots || ms < 0 || ms >= MEL_RING) return herr("conv0: a slot outside the pool or a mel_start outside the ring");
        memset(&t[b], 0, sizeof(RowDesc));
        t[b].slot = slot; t[b].mel_start = ms; t[b].prompt = -1;
    }
    if (!upload(rows_tab, t, "rows")) return -1;
    launch_sub_conv0_dw(ptr<RowDesc>(rows_tab), B, chunk_mel, ptr<float>(mel_ring), ptr<float>(w0t), ptr<float>(b0), ptr<float>(w2t), ptr<float>(b2), ptr(out), out_bf16 ? 1 : 0,
                        H1, W1, 0);
    return sync_check();
}

// ---- launch_sub_dw -----------------------------------------------------------------------------------------------------------------------------------------
extern "C" int front_harness_dw(int in, int wt, int bias, int out, int out_bf16, int B, int Hin, int Win) {
    g_err[0] = 0;
    if (B < 1 || B > 65535 || Hin < 1 || Hin > 4096 || Win < 1 || Win > 4096) return herr("dw: B, Hin or Win outside the harness's range");
    const int Hout = Hin / 2 + 1, Wout = Win / 2 + 1;
    if (!need(in, (size_t)B * Hin * Win * SUBC * 4, "in") || !need(wt, 9 * SUBC * 4, "wt") || !need(bias, SUBC * 4, "bias") ||
        !need(out, (size_t)B * Hout * Wout * SUBC * (out_bf16 ? 2 : 4), "out"))
        return -1;
    launch_sub_dw(ptr<float>(in), B, Hin, Win, ptr<float>(wt), ptr<float>(bias), ptr(out), out_bf16 ? 1 : 0, 0);
    return sync_check();
}

// ---- launch_diar_logmel / launch_diar_frames -------------------------------------------------------------------------------------------------------------------
// a: audio, s16 (0 / 1), window, fbT, fb_band, cos_t, sin_t
static bool diar_params(const int *a, DiarMelParams &p, size_t &samples) {
    const Buf *ab = buf(a[0]);
    if (!ab) { herr("diar: audio handle"); return false; }
    if (!mel_tables_ok(a[2], a[3], a[4], a[5], a[6], DIAR_NMEL)) return false;
    memset(&p, 0, sizeof(p));
    samples = ab->body / (a[1] ? 2 : 4);
    if (a[1]) p.audio_s16 = (const int16_t *)ab->ptr();
    else p.audio = (const float *)ab->ptr();
    p.window = ptr<float>(a[2]); p.fbT = ptr<float>(a[3]); p.fb_band = ptr<int>(a[4]); p.cos_t = ptr<float>(a[5]); p.sin_t = ptr<float>(a[6]);
    return true;
}
extern "C" int front_harness_diar_logmel(const int *a, int win_off, int mel, int W, int n_win, int T_pad, int t_valid, int cpitch, int normalize) {
    g_err[0] = 0;
    DiarMelParams p;
    size_t samples;
    if (!diar_params(a, p, samples)) return -1;
    if (W < 1 || W > 4096 || n_win < 1 || n_win > (1 << 24) || T_pad < 1 || T_pad > 4096) return herr("diar_logmel: W, n_win or T_pad outside the harness's range");
    if (t_valid > T_pad) return herr("diar_logmel: t_valid > T_pad");
    if (t_valid < 1) return herr("diar_logmel: t_valid < 1 (k_diar_featnorm divides by it)");
    if (cpitch < DIAR_NMEL || cpitch > 256) return herr("diar_logmel: cpitch outside 80 .. 256 (one thread per column, 256 threads)");
    if (!need(win_off, (size_t)W * 8, "win_off") || !need(mel, (size_t)W * T_pad * cpitch * 4, "mel")) return -1;
    std::vector<long long> off(W);
    if (hipMemcpy(off.data(), ptr(win_off), (size_t)W * 8, hipMemcpyDeviceToHost) != hipSuccess) return herr("win_off: download");
    for (long long o : off)
        if (o < 0 || (size_t)o + n_win > samples) return herr("diar_logmel: a window leaves the audio buffer");
    p.win_off = ptr<long long>(win_off); p.n_win = n_win; p.T_pad = T_pad; p.t_valid = t_valid; p.cpitch = cpitch; p.mel = ptr<float>(mel);
    launch_diar_logmel(p, W, normalize != 0, 0);
    return sync_check();
}
// fr [n][3]: base, n, t
extern "C" int front_harness_diar_frames(const int *a, int tab, int out, const long long *fr, int n) {
    g_err[0] = 0;
    DiarMelParams p;
    size_t samples;
    if (!diar_params(a, p, samples)) return -1;
    if (n < 1 || n > 65535) return herr("diar_frames: n");
    if (!need(out, (size_t)n * DIAR_NMEL * 4, "out")) return -1;
    std::vector<DiarFrameDesc> t(n);
    for (int i = 0; i < n; i++) {
        const long long base = fr[3 * i], len = fr[3 * i + 1], tt = fr[3 * i + 2];
        if (base < 0 || len < 1 || len > (1 << 24) || (size_t)(base + len) > samples) return herr("diar_frames: a window leaves the audio buffer");
        if (tt < 0 || tt > (1 << 20)) return herr("diar_frames: t");
        t[i].base = base; t[i].n = (int)len; t[i].t = (int)tt;
    }
    if (!upload(tab, t, "frames")) return -1;
    launch_diar_frames(p, ptr<DiarFrameDesc>(tab), n, ptr<float>(out), 0);
    return sync_check();
}

// y[i] = logf(x[i]): the device libm as kernels_front.hip calls it
extern "C" int front_harness_libm(int x, int y, int n) {
    g_err[0] = 0;
    if (n < 1) return herr("libm: n");
    if (!need(x, (size_t)n * 4, "libm x") || !need(y, (size_t)n * 4, "libm y")) return -1;
    hipLaunchKernelGGL(k_libm, dim3((n + 255) / 256), dim3(256), 0, 0, ptr<float>(x), ptr<float>(y), n);
    return sync_check();
}
