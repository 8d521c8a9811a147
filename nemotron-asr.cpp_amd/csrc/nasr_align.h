// nasr_align.h -- the index maps and the recursions of forced alignment / transcript scoring on the RNN-T lattice
// (nasr_engine_align*), pure code without HIP so that the CPU suite compiles it with g++ under sanitizers
// (tests/test_align_math.py), like nasr_logprob.h / nasr_topk.h.  kernels_align.hip includes it and runs the same functions on
// the device.
//
// Lattice of an utterance with T encoder frames and a transcript y of U tokens: cells (t, u), 0 <= t < T, 0 <= u <= U, row-major
// [T][U + 1].  lb(t, u) = ln P(blank | t, u), ly(t, u) = ln P(y_u | t, u) for u < U (column U of ly holds -inf).
//   alpha(0, 0) = 0
//   alpha(t, u) = logaddexp(alpha(t - 1, u) + lb(t - 1, u), alpha(t, u - 1) + ly(t, u - 1))          loglik = alpha(T - 1, U) + lb(T - 1, U)
//   delta = the same with max (Viterbi); the token move (t, u - 1) -> (t, u) is taken only when its score is STRICTLY greater than the
//   blank move's (t - 1, u) -> (t, u); one back-pointer bit per cell; best = delta(T - 1, U) + lb(T - 1, U).
// The recursions run in double: their error is far below that of the f32 cells they sum.
//
// The joint kernel (k_align_lattice) cuts every lattice into tiles of TILE_T frames x TILE_U label positions, one workgroup each; a
// launch covers consecutive tiles up to "align_cells" cells (engine option).  Every cell is one fixed-order accumulation whatever tile
// or launch it falls into, so the results do not depend on that option or on what else is in the batch.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "nasr_logprob.h"
#include <vector>

namespace nasr_align {

constexpr int TILE_T = 16, TILE_U = 8, TILE_CELLS = TILE_T * TILE_U;     // a workgroup's cells: 8 MFMA column tiles of 16 frames
constexpr int MAX_TOKENS = 1024;                                          // NASR_ALIGN_MAX_TOKENS
constexpr int MIN_CELLS = 64, DEFAULT_CELLS = 1 << 20;                    // engine option "align_cells"
constexpr int ALIGN_VOCAB = nasr_lp::LP_VOCAB, ALIGN_BLANK = ALIGN_VOCAB - 1;

// an utterance of a sub-batch as the kernels see it
struct Utt {
    int enc_row;              // first of its T packed encproj rows
    int g_row;                // first of its U + 1 prediction-network rows g[0 .. U]
    int T, U;
    long long cell0;          // first of its T * (U + 1) cells in lp_blank / lp_token / the back-pointers
    int tok0;                 // first of its U tokens (and of its U frames / token log-probabilities)
    int pad;
};
struct Tile { int utt, t0, u0, pad; };

NASR_LP_HD int tiles_t(int T) { return (T + TILE_T - 1) / TILE_T; }
NASR_LP_HD int tiles_u(int U) { return (U + 1 + TILE_U - 1) / TILE_U; }
NASR_LP_HD int n_tiles(int T, int U) { return T > 0 ? tiles_t(T) * tiles_u(U) : 0; }
NASR_LP_HD long long n_cells(int T, int U) { return (long long)T * (U + 1); }
NASR_LP_HD long long cell_index(int U, int t, int u) { return (long long)t * (U + 1) + u; }
// tile i of an utterance: label positions fastest
NASR_LP_HD Tile tile_of(int utt, int U, int i) {
    Tile td;
    td.utt = utt; td.t0 = (i / tiles_u(U)) * TILE_T; td.u0 = (i % tiles_u(U)) * TILE_U; td.pad = 0;
    return td;
}
NASR_LP_HD int tile_cells(int T, int U, int t0, int u0) {                // cells of the tile that exist
    const int nt = T - t0 < TILE_T ? T - t0 : TILE_T, nu = U + 1 - u0 < TILE_U ? U + 1 - u0 : TILE_U;
    return nt > 0 && nu > 0 ? nt * nu : 0;
}
// the workgroup's thread c < 128 finishes cell c of its tile: label position u0 + c / 16 (= the MFMA column tile), frame t0 + c % 16 (= the
// column inside it).  Returns the cell's index in the lattice arrays, or -1 for a thread without a cell (edge tiles, threads 128 ..)
NASR_LP_HD long long store_cell(const Utt &ud, const Tile &td, int thread, int *t_out = nullptr, int *u_out = nullptr) {
    if (thread < 0 || thread >= TILE_CELLS) return -1;
    const int u = td.u0 + (thread >> 4), t = td.t0 + (thread & 15);
    if (t >= ud.T || u > ud.U) return -1;
    if (t_out) *t_out = t;
    if (u_out) *u_out = u;
    return ud.cell0 + cell_index(ud.U, t, u);
}

// (host) the tiles of a sub-batch in utterance order and the first tile of every launch (+ the end): a launch takes tiles while the cells that
// exist in them stay within align_cells, and at least one
inline void plan_launches(const Utt *utt, int n, long long align_cells, std::vector<Tile> &tiles, std::vector<int> &first) {
    tiles.clear(); first.clear();
    long long in_launch = 0;
    for (int k = 0; k < n; k++)
        for (int i = 0; i < n_tiles(utt[k].T, utt[k].U); i++) {
            const Tile td = tile_of(k, utt[k].U, i);
            const int c = tile_cells(utt[k].T, utt[k].U, td.t0, td.u0);
            if (first.empty() || in_launch + c > align_cells) { first.push_back((int)tiles.size()); in_launch = 0; }
            tiles.push_back(td);
            in_launch += c;
        }
    first.push_back((int)tiles.size());
}

// ---- the recursions ------------------------------------------------------------------------------------------------------------
NASR_LP_HD double neg_inf_d() { return -(double)__builtin_inff(); }
NASR_LP_HD double logaddexp(double a, double b) {
    if (a == neg_inf_d()) return b;
    if (b == neg_inf_d()) return a;
    const double m = a > b ? a : b, d = a > b ? b - a : a - b;
    return m + log1p(exp(d));
}
struct Cell { double alpha, delta; unsigned char token_move; };
// cell (t, u) from its two predecessors: up = (t - 1, u) with lb(t - 1, u), left = (t, u - 1) with ly(t, u - 1); (0, 0) has neither
NASR_LP_HD Cell step(bool has_up, double a_up, double d_up, float lb_up, bool has_left, double a_left, double d_left, float ly_left) {
    Cell c;
    if (!has_up && !has_left) { c.alpha = 0.0; c.delta = 0.0; c.token_move = 0; return c; }
    const double ab = has_up ? a_up + (double)lb_up : neg_inf_d(), at = has_left ? a_left + (double)ly_left : neg_inf_d();
    const double sb = has_up ? d_up + (double)lb_up : neg_inf_d(), st = has_left ? d_left + (double)ly_left : neg_inf_d();
    c.alpha = logaddexp(ab, at);
    c.token_move = (has_left && (!has_up || st > sb)) ? 1 : 0;            // the tie rule: strictly greater
    c.delta = c.token_move ? st : sb;
    return c;
}
// label positions of anti-diagonal d = t + u
NASR_LP_HD void diag_range(int d, int T, int U, int *u_lo, int *u_hi) {
    *u_lo = d - (T - 1) > 0 ? d - (T - 1) : 0;
    *u_hi = d < U ? d : U;
}
// best path from the back-pointers: frames[i] = the frame at which y_i is emitted, lps[i] = ly(frames[i], i); at most T + U steps
NASR_LP_HD void backtrace(const unsigned char *bp, const float *ly, int T, int U, int32_t *frames, float *lps) {
    int t = T - 1, u = U;
    while (u > 0 && t >= 0) {
        if (bp[cell_index(U, t, u)]) {
            u--;
            frames[u] = t;
            lps[u] = ly[cell_index(U, t, u)];
        } else t--;
    }
}

// host restatement of k_align_recursion: the same march over anti-diagonals with two diagonals kept, one label position after the other
inline void run_lattice(const float *lb, const float *ly, int T, int U, double *loglik, double *best, unsigned char *bp, int32_t *frames, float *lps) {
    if (T <= 0) {
        *loglik = *best = U == 0 ? 0.0 : neg_inf_d();
        for (int i = 0; i < U; i++) { frames[i] = -1; lps[i] = nasr_lp::neg_inf(); }
        return;
    }
    std::vector<double> a[2], dl[2];
    for (int i = 0; i < 2; i++) { a[i].assign((size_t)U + 1, neg_inf_d()); dl[i].assign((size_t)U + 1, neg_inf_d()); }
    for (int d = 0; d <= T - 1 + U; d++) {
        int lo, hi;
        diag_range(d, T, U, &lo, &hi);
        const int cur = d & 1, prev = cur ^ 1;
        for (int u = lo; u <= hi; u++) {
            const int t = d - u;
            const bool up = t > 0, left = u > 0;
            const Cell c = step(up, up ? a[prev][(size_t)u] : 0.0, up ? dl[prev][(size_t)u] : 0.0, up ? lb[cell_index(U, t - 1, u)] : 0.0f,
                                left, left ? a[prev][(size_t)u - 1] : 0.0, left ? dl[prev][(size_t)u - 1] : 0.0, left ? ly[cell_index(U, t, u - 1)] : 0.0f);
            a[cur][(size_t)u] = c.alpha; dl[cur][(size_t)u] = c.delta;
            bp[cell_index(U, t, u)] = c.token_move;
        }
    }
    const int last = (T - 1 + U) & 1;
    *loglik = a[last][(size_t)U] + (double)lb[cell_index(U, T - 1, U)];
    *best = dl[last][(size_t)U] + (double)lb[cell_index(U, T - 1, U)];
    backtrace(bp, ly, T, U, frames, lps);
}

}  // namespace nasr_align
