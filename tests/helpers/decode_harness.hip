// Test helper (not product code): ONE launcher call of kernels_decode.hip on buffers with guard regions, for tests/test_gpu_decode_kernels.py.
//   hipcc --offload-arch=gfx950 -O2 -shared -fPIC -I../../nemotron-asr.cpp_amd/csrc -I../../include -o libdecode_harness.so decode_harness.hip   (built by __graft_entry__.build())
//
// The decode kernels are the product's: nasr::launch_encproj, launch_decode_begin, launch_decode_candidates, launch_decode_iter, launch_decode_rows,
// launch_decode_rows_boost and launch_lm_rows, resolved from libnemotron_asr_amd.so (the test loads that library with RTLD_GLOBAL before this one),
// and so is the weight packer nasr_eng::pack_f32_mfma (nasr_engine_priv.h): packer and kernel are tested as a pair against the row-major matrix.
// The one kernel of its own, k_libm, applies the three device libm functions the decode's cell update and softmax parts use to an array; it
// serves only to measure them against float64.
//
// The buffer plumbing is layer_harness.hip's: buffers by handle, each [guard | body | guard] and all of it the 16-bit pattern SENTINEL; the test
// uploads its inputs into the bodies -- poison included -- and gets every buffer back whole.  A DecCase names every buffer of a DecParams by
// handle, -1 = null.  Before anything is launched the entry checks every buffer's body against the bytes the launch may address and every INDEX a
// kernel may read -- rows[b].slot, dlist, rowmap, the three counters, and per slot prev_token, cur, t, n_frames, the automaton and LM states --
// against the buffers it indexes, the entries only the clamped lanes read included: a case the kernels' indexing does not cover is an error,
// never a launch.
#include "nasr_internal.h"
#include "nasr_lm.h"
#include "nasr_step_plan.h"
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

char g_err[512];
int herr(const char *what, hipError_t e = hipSuccess) {
    snprintf(g_err, sizeof(g_err), "%s%s%s", what, e == hipSuccess ? "" : ": ", e == hipSuccess ? "" : hipGetErrorString(e));
    return -1;
}
const Buf *buf(int h) { return h >= 0 && h < (int)g_bufs.size() && g_bufs[h].base ? &g_bufs[h] : nullptr; }
template <typename T = void> T *ptr(int h) { const Buf *b = buf(h); return b ? (T *)b->ptr() : nullptr; }
// handle h holds at least `bytes` in its body
bool need(int h, size_t bytes, const char *name) {
    const Buf *b = buf(h);
    if (b && b->body >= bytes) return true;
    snprintf(g_err, sizeof(g_err), "buffer %s: handle %d holds %zu bytes, the launch addresses %zu", name, h, b ? b->body : (size_t)0, bytes);
    return false;
}
// a buffer that may be null (-1)
bool need_opt(int h, size_t bytes, const char *name) { return h < 0 || need(h, bytes, name); }
int sync_check() {
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return herr("hipDeviceSynchronize", e);
    if ((e = hipGetLastError()) != hipSuccess) return herr("launch", e);
    return 0;
}
template <typename T>
bool fetch(int h, size_t n, std::vector<T> &out, const char *name) {
    out.resize(n);
    if (n > 0 && hipMemcpy(out.data(), ptr(h), n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: download", name);
        return false;
    }
    return true;
}

// every buffer of a DecParams by handle (-1 = null); counters = {n_active, n_dirty, n_rows}
struct DecCase {
    int rows, B, T, n_slots, ctrl, h, c, encproj, embed;
    int w_ih[2], w_hh[2], b_ih[2], b_hh[2];
    int pred_w, pred_b, out_w, out_b, predg, key, counters, dlist, rowmap, tok_ring, tok_frame;
    int lp_part, tok_logprob;
    int boost_bonus, boost_next, boost_state, n_states, boost_raw, raw_logits;
    int alt_key, alt_id, alt_lp, alt_k;
    int fb_row, frame_blank;
    int lm_blk, lm_state, lm_row, lm_next, lm_fold, lm_relook, lm_states;
    int ent_part, tok_entropy;
    float ent_alpha;
};
// the fixed block of "lm_fusion" from its tables' handles
struct LmCase { int blk, states, uni, arcs, n_arcs, n_states, order, max_probe, start, attached; float weight, token_bonus; };

enum { CALL_BEGIN = 0, CALL_CANDIDATES, CALL_ITER, CALL_ROWS, CALL_ROWS_BOOST };

__global__ void k_libm(const float *x, float *y, int n, int which) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    y[i] = which == 0 ? 1.0f / (1.0f + expf(-v)) : which == 1 ? tanhf(v) : expf(v);
}

// sizes and indices of a DecCase: everything any kernel of the call may address
bool check_case(const DecCase &c, int call) {
    const int B = c.B, T = c.T, S = c.n_slots;
    if (B < 1 || B > 65535 || T < 1 || T > 65535 || S < 1 || (long long)B * T > (1 << 20)) { herr("B, T or n_slots outside the harness's range"); return false; }
    const size_t BT = (size_t)B * T;
    const int np = nasr_lp::n_parts(B * T);
    const bool beam = call == CALL_ROWS || call == CALL_ROWS_BOOST;
    const int parts = beam ? nasr_lp::WG_PARTS : np;
    if (!need(c.rows, (size_t)B * sizeof(RowDesc), "rows") || !need(c.ctrl, (size_t)S * sizeof(DecCtrl), "ctrl") || !need(c.h, (size_t)S * 4 * HID * 4, "h") ||
        !need(c.c, (size_t)S * 4 * HID * 4, "c") || !need(c.encproj, BT * JNT * 4, "encproj") || !need(c.embed, (size_t)VOCAB * HID * 4, "embed") ||
        !need(c.pred_w, (size_t)JNT * HID * 4, "pred_w") || !need(c.pred_b, JNT * 4, "pred_b") || !need(c.out_w, (size_t)65 * 16 * JNT * 4, "out_w") ||
        !need(c.out_b, VOCAB * 4, "out_b") || !need(c.predg, (size_t)S * JNT * 4, "predg") || !need(c.key, BT * 8, "key") || !need(c.counters, 12, "counters") ||
        !need(c.dlist, (size_t)B * 4, "dlist") || !need(c.rowmap, BT * 4, "rowmap") || !need(c.tok_ring, (size_t)S * TOK_CAP * 4, "tok_ring") ||
        !need(c.tok_frame, (size_t)S * TOK_CAP * 4, "tok_frame"))
        return false;
    for (int l = 0; l < 2; l++)
        if (!need(c.w_ih[l], (size_t)4 * HID * HID * 4, "w_ih") || !need(c.w_hh[l], (size_t)4 * HID * HID * 4, "w_hh") || !need(c.b_ih[l], 4 * HID * 4, "b_ih") ||
            !need(c.b_hh[l], 4 * HID * 4, "b_hh"))
            return false;
    if (!nasr_topk::valid_k(c.alt_k) || (c.alt_key >= 0 && c.alt_k < 1)) { herr("alt_k"); return false; }
    if (!need_opt(c.lp_part, BT * parts * sizeof(nasr_lp::Part), "lp_part") || !need_opt(c.tok_logprob, (size_t)S * TOK_CAP * 4, "tok_logprob") ||
        !need_opt(c.boost_bonus, nasr_boost::table_elems(c.n_states) * 4, "boost_bonus") || !need_opt(c.boost_next, nasr_boost::table_elems(c.n_states) * 4, "boost_next") ||
        !need_opt(c.boost_state, (size_t)S * 4, "boost_state") || !need_opt(c.boost_raw, BT * parts * 4, "boost_raw") ||
        !need_opt(c.raw_logits, BT * nasr_boost::COLS * 4, "raw_logits") || !need_opt(c.alt_key, BT * parts * c.alt_k * 8, "alt_key") ||
        !need_opt(c.alt_id, (size_t)S * TOK_CAP * c.alt_k * 4, "alt_id") || !need_opt(c.alt_lp, (size_t)S * TOK_CAP * c.alt_k * 4, "alt_lp") ||
        !need_opt(c.fb_row, BT * 4, "fb_row") || !need_opt(c.frame_blank, (size_t)S * FRAME_CAP * 4, "frame_blank") ||
        !need_opt(c.lm_blk, sizeof(nasr_lm::Greedy), "lm_blk") || !need_opt(c.lm_state, (size_t)S * 4, "lm_state") ||
        !need_opt(c.lm_row, (size_t)S * nasr_lm::ROW_COLS * 4, "lm_row") || !need_opt(c.lm_next, (size_t)S * nasr_lm::ROW_COLS * 4, "lm_next") ||
        !need_opt(c.ent_part, BT * parts * 4, "ent_part") || !need_opt(c.tok_entropy, (size_t)S * TOK_CAP * 4, "tok_entropy"))
        return false;
    // the options come in the sets the launchers' rules assume
    const bool lp = c.lp_part >= 0;
    if (lp != (c.tok_logprob >= 0) || (c.alt_key >= 0 && (!lp || c.alt_id < 0 || c.alt_lp < 0)) || ((c.fb_row >= 0) != (c.frame_blank >= 0)) || (c.fb_row >= 0 && !lp) ||
        ((c.ent_part >= 0) != (c.tok_entropy >= 0)) || (c.ent_part >= 0 && !lp)) { herr("options: lp_part / alt / frame_blank / entropy buffers do not come as a set"); return false; }
    if (c.boost_bonus >= 0 && (c.boost_state < 0 || c.n_states < 1 || (!beam && c.boost_next < 0) || (lp && !beam && c.boost_raw < 0))) { herr("options: phrase_boost buffers do not come as a set"); return false; }
    if (c.lm_row >= 0 && (c.lm_blk < 0 || c.lm_state < 0 || c.lm_next < 0 || (lp && c.boost_raw < 0))) { herr("options: lm_fusion buffers do not come as a set"); return false; }
    if (c.lm_row < 0 && c.boost_bonus < 0 && c.boost_next >= 0) { herr("options: boost_next without boost_bonus"); return false; }
    if (call == CALL_ROWS && (!lp || c.alt_key < 0)) { herr("launch_decode_rows needs lp_part and alt_key"); return false; }
    if (call == CALL_ROWS_BOOST && (!lp || c.alt_key < 0 || c.boost_bonus < 0 || c.raw_logits < 0)) { herr("launch_decode_rows_boost needs lp_part, alt_key, boost_bonus and raw_logits"); return false; }
    // indices
    std::vector<RowDesc> rows;
    std::vector<DecCtrl> ctrl;
    std::vector<int> cnt, dlist, bstate, lstate;
    std::vector<unsigned> rowmap;
    if (!fetch(c.rows, B, rows, "rows") || !fetch(c.ctrl, S, ctrl, "ctrl") || !fetch(c.counters, 3, cnt, "counters") || !fetch(c.dlist, B, dlist, "dlist") ||
        !fetch(c.rowmap, BT, rowmap, "rowmap"))
        return false;
    std::vector<char> seen((size_t)S, 0);
    for (int b = 0; b < B; b++) {
        const int s = rows[b].slot;
        if (s < 0 || s >= S || seen[s]) { herr("rows: a slot outside the pool or used twice"); return false; }
        seen[s] = 1;
        if (rows[b].n_dec < 0 || rows[b].n_dec > T) { herr("rows: n_dec outside 0 .. T"); return false; }
        const DecCtrl &ct = ctrl[s];
        if (ct.prev_token < 0 || ct.prev_token >= VOCAB || (ct.cur != 0 && ct.cur != 1)) { herr("ctrl: prev_token or cur outside its range"); return false; }
        if (call != CALL_BEGIN && (ct.t < 0 || ct.n_frames < ct.t || ct.n_frames > T || ct.n_tok < 0)) { herr("ctrl: t, n_frames or n_tok outside 0 <= t <= n_frames <= T"); return false; }
    }
    if (call != CALL_BEGIN) {
        if (cnt[0] < 0 || cnt[0] > B || cnt[1] < 0 || cnt[1] > B || cnt[2] < 0 || (size_t)cnt[2] > BT) { herr("counters outside their lists"); return false; }
        for (int i = 0; i < B; i++)
            if (dlist[i] < 0 || dlist[i] >= B) { herr("dlist: a batch row outside 0 .. B - 1"); return false; }
        for (size_t i = 0; i < BT; i++)
            if ((int)(rowmap[i] & 0xffffu) >= B || (int)(rowmap[i] >> 16) >= T) { herr("rowmap: a (frame, batch row) outside the step"); return false; }
    }
    if (c.boost_state >= 0) {
        if (!fetch(c.boost_state, S, bstate, "boost_state")) return false;
        for (int s = 0; s < S; s++)
            if (c.boost_bonus >= 0 || c.boost_next >= 0)
                if (bstate[s] < 0 || bstate[s] >= c.n_states) { herr("boost_state: a state outside the tables"); return false; }
        if (c.boost_next >= 0) {
            std::vector<int> nx;
            if (!fetch(c.boost_next, nasr_boost::table_elems(c.n_states), nx, "boost_next")) return false;
            for (int v : nx)
                if (v < 0 || v >= c.n_states) { herr("boost_next: a state outside the tables"); return false; }
        }
    }
    if (c.lm_state >= 0) {
        if (!fetch(c.lm_state, S, lstate, "lm_state")) return false;
        for (int s = 0; s < S; s++)
            if (lstate[s] < -1 || lstate[s] >= (c.lm_states > 0 ? c.lm_states : 1)) { herr("lm_state: a state outside the model"); return false; }
        if (c.lm_next >= 0) {                          // k_dec_commit moves lm_state to an entry of the slot's row: rows[b].slot's rows hold states or the sentinel's bits nowhere
            std::vector<int> nx;
            if (!fetch(c.lm_next, (size_t)S * nasr_lm::ROW_COLS, nx, "lm_next")) return false;
            for (int b = 0; b < B; b++)
                for (int v = 0; v < nasr_lm::ROW_COLS; v++) {
                    const int x = nx[(size_t)rows[b].slot * nasr_lm::ROW_COLS + v];
                    if (x < -1 || x >= (c.lm_states > 0 ? c.lm_states : 1)) { herr("lm_next: a state outside the model in a row of the batch"); return false; }
                }
        }
    }
    return true;
}

void fill_params(const DecCase &c, DecParams &p) {
    memset(&p, 0, sizeof(p));
    p.rows = ptr<RowDesc>(c.rows); p.B = c.B; p.T = c.T;
    p.ctrl = ptr<DecCtrl>(c.ctrl); p.h = ptr<float>(c.h); p.c = ptr<float>(c.c);
    p.encproj = ptr<float>(c.encproj); p.embed = ptr<float>(c.embed);
    for (int l = 0; l < 2; l++) { p.w_ih[l] = ptr<float>(c.w_ih[l]); p.w_hh[l] = ptr<float>(c.w_hh[l]); p.b_ih[l] = ptr<float>(c.b_ih[l]); p.b_hh[l] = ptr<float>(c.b_hh[l]); }
    p.pred_w = ptr<float>(c.pred_w); p.pred_b = ptr<float>(c.pred_b); p.out_w = ptr<float>(c.out_w); p.out_b = ptr<float>(c.out_b);
    p.predg = ptr<float>(c.predg); p.key = ptr<unsigned long long>(c.key);
    int *cnt = ptr<int>(c.counters);
    p.n_active = cnt; p.n_dirty = cnt + 1; p.n_rows = cnt + 2;
    p.dlist = ptr<int>(c.dlist); p.rowmap = ptr<unsigned>(c.rowmap); p.tok_ring = ptr<int>(c.tok_ring); p.tok_frame = ptr<int>(c.tok_frame);
    p.lp_part = ptr<nasr_lp::Part>(c.lp_part); p.tok_logprob = ptr<float>(c.tok_logprob);
    p.boost_bonus = ptr<float>(c.boost_bonus); p.boost_next = ptr<int32_t>(c.boost_next); p.boost_state = ptr<int>(c.boost_state);
    p.boost_raw = ptr<float>(c.boost_raw); p.raw_logits = ptr<float>(c.raw_logits);
    p.alt_key = ptr<unsigned long long>(c.alt_key); p.alt_id = ptr<int32_t>(c.alt_id); p.alt_lp = ptr<float>(c.alt_lp); p.alt_k = c.alt_k;
    p.fb_row = ptr<float>(c.fb_row); p.frame_blank = ptr<float>(c.frame_blank);
    p.lm_blk = ptr<nasr_lm::Greedy>(c.lm_blk); p.lm_state = ptr<int32_t>(c.lm_state); p.lm_row = ptr<float>(c.lm_row); p.lm_next = ptr<int32_t>(c.lm_next);
    p.lm_fold = c.lm_fold; p.lm_relook = c.lm_relook;
    p.ent_part = ptr<float>(c.ent_part); p.tok_entropy = ptr<float>(c.tok_entropy); p.ent_alpha = c.ent_alpha;
}

}  // namespace

extern "C" const char *decode_harness_error() { return g_err; }
extern "C" unsigned decode_harness_sentinel() { return SENTINEL; }
extern "C" int decode_harness_struct_bytes(int which) {
    const int v[] = {(int)sizeof(DecCase), (int)sizeof(LmCase), (int)sizeof(DecCtrl), (int)sizeof(RowDesc), (int)sizeof(nasr_lp::Part), (int)sizeof(nasr_lm::Greedy),
                     (int)sizeof(nasr_lm::State), (int)sizeof(nasr_lm::Uni), (int)sizeof(nasr_lm::Arc)};
    return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : -1;
}
extern "C" int decode_harness_constant(int which) {
    const int v[] = {D, HID, JNT, VOCAB, BLANK, TOK_CAP, FRAME_CAP, MAX_SYMBOLS, nasr_lp::SMALL_ROWS, nasr_lp::TILE_PARTS, nasr_lp::WG_PARTS, nasr_boost::COLS, nasr_lm::ROW_COLS,
                     nasr_topk::KMAX};
    return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : -1;
}

extern "C" int decode_harness_init(int device) {
    g_err[0] = 0;
    hipError_t e = hipSetDevice(device);
    return e == hipSuccess ? 0 : herr("hipSetDevice", e);
}
// a new buffer [guard | body | guard], all of it SENTINEL; returns its handle or -1
extern "C" int decode_harness_alloc(long long body_bytes, int guard_bytes) {
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
extern "C" long long decode_harness_total_bytes(int h) { const Buf *b = buf(h); return b ? (long long)b->total() : -1; }
extern "C" int decode_harness_put(int h, long long off, const void *src, long long bytes) {
    g_err[0] = 0;
    const Buf *b = buf(h);
    if (!b || off < 0 || bytes < 0 || (size_t)(off + bytes) > b->body) return herr("put: outside the body");
    if (bytes == 0) return 0;
    hipError_t e = hipMemcpy((char *)b->ptr() + off, src, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : herr("hipMemcpy (upload)", e);
}
// the whole buffer, guards included: dst holds decode_harness_total_bytes(h)
extern "C" int decode_harness_get(int h, void *dst) {
    g_err[0] = 0;
    const Buf *b = buf(h);
    if (!b) return herr("get: handle");
    hipError_t e = hipMemcpy(dst, b->base, b->total(), hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : herr("hipMemcpy (download)", e);
}
// the number of handles given out so far: free_from(count()) later frees what was allocated in between (the weights of a module stay)
extern "C" int decode_harness_count() { return (int)g_bufs.size(); }
extern "C" void decode_harness_free_from(int first) {
    if (first < 0) first = 0;
    for (size_t i = first; i < g_bufs.size(); i++)
        if (g_bufs[i].base) (void)hipFree(g_bufs[i].base);
    if ((size_t)first < g_bufs.size()) g_bufs.resize(first);
}
extern "C" void decode_harness_free_all() { decode_harness_free_from(0); }

// W [N][K] row-major in src -> the product's MFMA A-fragment order in dst (nasr_eng::pack_f32_mfma, on the host)
extern "C" int decode_harness_pack(int src, int dst, int N, int K, int lstm_order) {
    g_err[0] = 0;
    if (N < 1 || K < 16 || K % 16 || (lstm_order && (N != 4 * HID || K != HID))) return herr("pack: shape");
    const size_t out_elems = (size_t)((N + 15) / 16) * 16 * K;
    if (!need(src, (size_t)N * K * 4, "pack src") || !need(dst, out_elems * 4, "pack dst")) return -1;
    std::vector<float> w, t;
    if (!fetch(src, (size_t)N * K, w, "pack src")) return -1;
    nasr_eng::pack_f32_mfma(w, N, K, lstm_order != 0, t);
    if (t.size() != out_elems) return herr("pack: the packer's output has another size than the kernels index");
    hipError_t e = hipMemcpy(ptr(dst), t.data(), t.size() * 4, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : herr("hipMemcpy (packed weights)", e);
}

// k_encproj: out [M][N] = x [M][K] . W^T + bias.  grid = (N / 16, ceil(M / 64)); the four waves take K / 64 k-groups each, so K a multiple of 64
// is what the kernel covers -- any other K is refused here (the product's call sites pass 1024, 512, 192: asserted by the CPU tests)
extern "C" int decode_harness_encproj(int x, int wpk, int bias, int out, int M, int K, int N) {
    g_err[0] = 0;
    if (M < 1 || M > (1 << 20) || K < 64 || K % 64 || N < 16 || N % 16 || N > 65535 * 16) return herr("encproj: M, K (a multiple of 64) or N (a multiple of 16) outside the kernel's range");
    if (!need(x, (size_t)M * K * 4, "x") || !need(wpk, (size_t)N * K * 4, "wpk") || !need(bias, (size_t)N * 4, "bias") || !need(out, (size_t)M * N * 4, "out")) return -1;
    launch_encproj(ptr<float>(x), ptr<float>(wpk), ptr<float>(bias), ptr<float>(out), M, K, N, 0);
    return sync_check();
}

// one launcher call on the case's buffers: CALL_BEGIN .. CALL_ROWS_BOOST
extern "C" int decode_harness_call(const DecCase *c, int call) {
    g_err[0] = 0;
    if (call < CALL_BEGIN || call > CALL_ROWS_BOOST) return herr("call: which");
    if (!check_case(*c, call)) return -1;
    DecParams p;
    fill_params(*c, p);
    switch (call) {
    case CALL_BEGIN: launch_decode_begin(p, 0); break;
    case CALL_CANDIDATES: launch_decode_candidates(p, 0); break;
    case CALL_ITER: launch_decode_iter(p, 0); break;
    case CALL_ROWS: launch_decode_rows(p, 0); break;
    default: launch_decode_rows_boost(p, 0); break;
    }
    return sync_check();
}

// the fixed block nasr_lm::Greedy in `blk`, its view pointing at the tables of the handles (states [n_states], uni [UNI], arcs [n_arcs], n_arcs a power of two)
extern "C" int decode_harness_lm_block(const LmCase *c) {
    g_err[0] = 0;
    if (c->n_states < 1 || c->n_arcs < 1 || (c->n_arcs & (c->n_arcs - 1)) || c->order < 0 || c->order > nasr_lm::MAX_ORDER || c->max_probe < 0 || c->max_probe > c->n_arcs ||
        c->start < 0 || c->start >= c->n_states)
        return herr("lm_block: shape");
    if (!need(c->blk, sizeof(nasr_lm::Greedy), "lm_blk") || !need(c->states, (size_t)c->n_states * sizeof(nasr_lm::State), "lm states") ||
        !need(c->uni, (size_t)nasr_lm::UNI * sizeof(nasr_lm::Uni), "lm uni") || !need(c->arcs, (size_t)c->n_arcs * sizeof(nasr_lm::Arc), "lm arcs"))
        return -1;
    std::vector<nasr_lm::State> st;
    std::vector<nasr_lm::Uni> un;
    std::vector<nasr_lm::Arc> ar;
    if (!fetch(c->states, c->n_states, st, "lm states") || !fetch(c->uni, nasr_lm::UNI, un, "lm uni") || !fetch(c->arcs, c->n_arcs, ar, "lm arcs")) return -1;
    for (const auto &s : st) if (s.back < 0 || s.back >= c->n_states) return herr("lm states: a back-off state outside the model");
    for (const auto &u : un) if (u.next < 0 || u.next >= c->n_states) return herr("lm uni: a next state outside the model");
    for (const auto &a : ar) if (a.key != nasr_lm::EMPTY && (a.next < 0 || a.next >= c->n_states)) return herr("lm arcs: a next state outside the model");
    nasr_lm::Greedy g;
    memset(&g, 0, sizeof(g));
    if (c->attached) {
        g.lm.states = ptr<nasr_lm::State>(c->states); g.lm.uni = ptr<nasr_lm::Uni>(c->uni); g.lm.arcs = ptr<nasr_lm::Arc>(c->arcs);
        g.lm.mask = (unsigned long long)c->n_arcs - 1; g.lm.order = c->order; g.lm.max_probe = c->max_probe; g.lm.n_states = c->n_states; g.lm.start = c->start;
    }
    g.weight = c->weight; g.token_bonus = c->token_bonus; g.attached = c->attached ? 1 : 0;
    hipError_t e = hipMemcpy(ptr(c->blk), &g, sizeof(g), hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : herr("hipMemcpy (lm block)", e);
}

// k_lm_rows_slots: the bias rows of slots slot0 .. slot0 + n - 1 (boost_bonus / boost_state -1 without "phrase_boost")
extern "C" int decode_harness_lm_rows(const DecCase *c, int slot0, int n) {
    g_err[0] = 0;
    const int S = c->n_slots;
    if (S < 1 || slot0 < 0 || n < 0 || slot0 + n > S) return herr("lm_rows: slots outside the pool");
    if (!need(c->lm_blk, sizeof(nasr_lm::Greedy), "lm_blk") || !need(c->lm_state, (size_t)S * 4, "lm_state") || !need(c->lm_row, (size_t)S * nasr_lm::ROW_COLS * 4, "lm_row") ||
        !need(c->lm_next, (size_t)S * nasr_lm::ROW_COLS * 4, "lm_next") || (c->boost_bonus >= 0) != (c->boost_state >= 0) ||
        !need_opt(c->boost_bonus, nasr_boost::table_elems(c->n_states) * 4, "boost_bonus") || !need_opt(c->boost_state, (size_t)S * 4, "boost_state"))
        return g_err[0] ? -1 : herr("lm_rows: boost_bonus and boost_state come together");
    std::vector<int> st;
    if (!fetch(c->lm_state, S, st, "lm_state")) return -1;
    for (int s : st) if (s < -1 || s >= (c->lm_states > 0 ? c->lm_states : 1)) return herr("lm_state: a state outside the model");
    if (c->boost_state >= 0) {
        if (!fetch(c->boost_state, S, st, "boost_state")) return -1;
        for (int s : st) if (s < 0 || s >= c->n_states) return herr("boost_state: a state outside the tables");
    }
    launch_lm_rows(ptr<nasr_lm::Greedy>(c->lm_blk), ptr<int32_t>(c->lm_state), ptr<float>(c->lm_row), ptr<int32_t>(c->lm_next), ptr<float>(c->boost_bonus),
                   ptr<int>(c->boost_state), slot0, n, 0);
    return sync_check();
}

// y[i] = sigm(x[i]) (which 0), tanhf (1), expf (2): the device libm as kernels_decode.hip calls it
extern "C" int decode_harness_libm(int x, int y, int n, int which) {
    g_err[0] = 0;
    if (n < 1 || which < 0 || which > 2) return herr("libm: n or which");
    if (!need(x, (size_t)n * 4, "libm x") || !need(y, (size_t)n * 4, "libm y")) return -1;
    hipLaunchKernelGGL(k_libm, dim3((n + 255) / 256), dim3(256), 0, 0, ptr<float>(x), ptr<float>(y), n, which);
    return sync_check();
}
