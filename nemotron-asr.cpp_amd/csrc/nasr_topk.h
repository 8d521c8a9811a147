// nasr_topk.h -- the selection arithmetic and the index maps of the per-token alternatives (engine option "token_alternatives" = K,
// 1 .. 8), pure code without HIP so that the CPU suite compiles it with g++ under sanitizers (tests/test_topk_math.py), like
// nasr_logprob.h / nasr_boost.h.  kernels_decode.hip includes it and runs the same functions on the device.
//
// For every emitted token the decode keeps the K largest packed keys nasr_lp::pack_key(raw logit, id) of the row's 1025 joint outputs, in
// descending order (= descending logit, among equal logit bits the lower id first: the tie rule of the arg-max), and for each
//   ln P(id) = (logit[id] - m) - log s     with m, s the row's softmax parts merged as nasr_lp::finish merges them.
// A key names one vocabulary entry, so keys are unique and the K largest of a row are one fixed list whatever the order of the merges.
// A list is KMAX = 8 keys in registers, sorted descending, 0 (below every real key) where it has fewer entries:
//   lane     the lane's four keys sorted by a 5-comparator network                                              (lane_keys)
//   tile     16 entries = the four lane groups of a wave: merge8 over the xor-16 / xor-32 butterfly              (tile_keys)
//   k_dec_joint (up to 64 rows a step)       one list per 16-entry tile: 65 slices, slice = blockIdx.x
//   k_dec_joint_tiled (more rows)            one list per workgroup = 64 entries, its four waves' lists merged     (wg_keys)
// The kernels store the first K keys of every slice into a scratch [key index][slice][K] with plain stores, one writer per element (the
// writer threads are those of the softmax parts: nasr_lp::joint_store_row / tiled_store_row).  k_dec_commit merges the slices of the one
// frame it commits (RowTop) and writes K ids and K values into the rings alt_id / alt_lp [slot][4096][K].  The K largest of a union of
// slices are among the K largest of each slice, so storing K per slice loses nothing, and K = 4 is a prefix of K = 8.
#pragma once
#include "nasr_logprob.h"

#if defined(__HIPCC__)
#define NASR_TOPK_UNROLL _Pragma("unroll")
#else
#define NASR_TOPK_UNROLL
#endif

namespace nasr_topk {

typedef unsigned long long tkey;
constexpr int KMAX = 8;

NASR_LP_HD tkey kmax2(tkey a, tkey b) { return a > b ? a : b; }
NASR_LP_HD tkey kmin2(tkey a, tkey b) { return a > b ? b : a; }
NASR_LP_HD void cex(tkey &hi, tkey &lo) { const tkey a = kmax2(hi, lo), b = kmin2(hi, lo); hi = a; lo = b; }   // compare-exchange, descending

// the lane's entries v0 .. v0 + 3 of a row (those below the vocabulary's end) as a sorted list
NASR_LP_HD void lane_keys(float x0, float x1, float x2, float x3, int v0, tkey *out) {
    const int n = nasr_lp::lane_valid(v0);
    tkey a = n > 0 ? nasr_lp::pack_key(x0, v0) : 0ull, b = n > 1 ? nasr_lp::pack_key(x1, v0 + 1) : 0ull;
    tkey c = n > 2 ? nasr_lp::pack_key(x2, v0 + 2) : 0ull, d = n > 3 ? nasr_lp::pack_key(x3, v0 + 3) : 0ull;
    cex(a, b); cex(c, d); cex(a, c); cex(b, d); cex(b, c);
    out[0] = a; out[1] = b; out[2] = c; out[3] = d;
    out[4] = out[5] = out[6] = out[7] = 0ull;
}
// a = the 8 largest of two sorted lists, sorted: max(a[i], b[7 - i]) holds them as a bitonic sequence, three half-cleaner stages
// sort it.  Symmetric in its arguments as a set operation on unique keys (both lanes of a butterfly step get the same list)
NASR_LP_HD void merge8(tkey *a, const tkey *b) {
    tkey c[KMAX];
    for (int i = 0; i < KMAX; i++) c[i] = kmax2(a[i], b[KMAX - 1 - i]);
    for (int i = 0; i < 4; i++) cex(c[i], c[i + 4]);
    for (int i = 0; i < 2; i++) { cex(c[i], c[i + 2]); cex(c[i + 4], c[i + 6]); }
    for (int i = 0; i < KMAX; i += 2) cex(c[i], c[i + 1]);
    for (int i = 0; i < KMAX; i++) a[i] = c[i];
}

// host restatement of what a kernel leaves for one slice: the 16-entry tile nt of a row's 1025 logits, butterfly order (q0, q1), (q2, q3)
NASR_LP_HD void tile_keys(const float *logits, int nt, tkey *out) {
    tkey q[4][KMAX];
    for (int k = 0; k < 4; k++) {
        const int v0 = nt * nasr_lp::TILE_W + k * 4, n = nasr_lp::lane_valid(v0);
        lane_keys(n > 0 ? logits[v0] : 0.0f, n > 1 ? logits[v0 + 1] : 0.0f, n > 2 ? logits[v0 + 2] : 0.0f, n > 3 ? logits[v0 + 3] : 0.0f, v0, q[k]);
    }
    merge8(q[0], q[1]); merge8(q[2], q[3]); merge8(q[0], q[2]);
    for (int i = 0; i < KMAX; i++) out[i] = q[0][i];
}
// the 64 entries of workgroup x = tiles 4x .. 4x + 3, its waves merged in wave order
NASR_LP_HD void wg_keys(const float *logits, int x, tkey *out) {
    tkey w[KMAX];
    tile_keys(logits, 4 * x, out);
    for (int u = 1; u < 4; u++) { tile_keys(logits, 4 * x + u, w); merge8(out, w); }
}

// ---- the row: the K largest of its slices' lists --------------------------------------------------------------------------------
struct RowTop { tkey top[KMAX]; tkey last; };                        // top[0 .. K) sorted descending, last = top[K - 1]
NASR_LP_HD void row_begin(RowTop &t) { for (int i = 0; i < KMAX; i++) t.top[i] = 0ull; t.last = 0ull; }
// a bubble pass without data-dependent indexing (the list stays in registers): key sinks to its place, the smallest of the K drops out
NASR_LP_HD void row_insert(RowTop &t, int K, tkey key) {
    tkey x = key;
    NASR_TOPK_UNROLL
    for (int i = 0; i < KMAX; i++)
        if (i < K) { cex(t.top[i], x); if (i == K - 1) t.last = t.top[i]; }
}
// the row's K largest from its slices' stored lists keys[slices][K].  A list is descending, so the first key that does not beat the K-th so
// far ends its slice: most slices cost their head alone.  The heads of HEAD_GROUP slices are loaded together -- independent loads in
// flight at once; read one by one behind each slice's test they would be a chain of `slices` memory latencies in the committing thread
constexpr int HEAD_GROUP = 8;
NASR_LP_HD void row_merge(RowTop &t, int K, const tkey *keys, int slices) {
    for (int s0 = 0; s0 < slices; s0 += HEAD_GROUP) {
        tkey head[HEAD_GROUP];
        NASR_TOPK_UNROLL
        for (int u = 0; u < HEAD_GROUP; u++) head[u] = s0 + u < slices ? keys[(size_t)(s0 + u) * K] : 0ull;
        NASR_TOPK_UNROLL
        for (int u = 0; u < HEAD_GROUP; u++) {
            if (head[u] <= t.last) continue;
            row_insert(t, K, head[u]);
            const tkey *rest = keys + (size_t)(s0 + u) * K;
            for (int j = 1; j < K; j++) {
                const tkey k = rest[j];
                if (k <= t.last) break;
                row_insert(t, K, k);
            }
        }
    }
}

// ---- from keys and parts to (id, ln P) ------------------------------------------------------------------------------------------------
// the row's softmax parts merged in ascending part index, the loops of nasr_lp::finish: m = max, log_s = log(sum exp(x - m))
NASR_LP_HD void row_softmax(const nasr_lp::Part *parts, int n_parts, float *m_out, float *log_s_out) {
    float m = nasr_lp::neg_inf();
    for (int i = 0; i < n_parts; i++) m = fmaxf(m, parts[i].m);
    float s = 0.0f;
    for (int i = 0; i < n_parts; i++) s += parts[i].s * expf(parts[i].m - m);
    *m_out = m;
    *log_s_out = logf(s);
}
NASR_LP_HD float lp_of(float logit, float m, float log_s) { return (logit - m) - log_s; }                    // = nasr_lp::finish(logit, parts)
NASR_LP_HD int alt_id(tkey key) { return nasr_lp::key_index_of(key); }
NASR_LP_HD float alt_lp(tkey key, float m, float log_s) { return lp_of(nasr_lp::key_logit(key), m, log_s); }  // the logit's own bits, from the key

// ---- where the lists live -------------------------------------------------------------------------------------------------------------
NASR_LP_HD bool valid_k(int K) { return K >= 0 && K <= KMAX; }
NASR_LP_HD size_t scratch_keys(int max_step_rows, int K) { return nasr_lp::scratch_parts(max_step_rows) * (size_t)K; }       // keys to allocate
NASR_LP_HD size_t scratch_index(int key_idx, int slice, int slices, int K) { return nasr_lp::scratch_index(key_idx, slice, slices) * (size_t)K; }   // of the slice's key 0
NASR_LP_HD size_t ring_index(int slot, int n_tok, int ring_cap, int K) { return ((size_t)slot * ring_cap + (size_t)(n_tok & (ring_cap - 1))) * (size_t)K; }

}  // namespace nasr_topk
