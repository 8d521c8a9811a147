// kernels_align.hip -- forced alignment / transcript scoring on the RNN-T lattice (nasr_engine_align*; index maps, recursion step,
// tie rule and backtrace in nasr_align.h).
//   k_align_pred_step   teacher forcing: between two runs of the decode's own LSTM / joint.pred launches (launch_decode_candidates,
//                       kernels_decode.hip) it stores g[u - 1] of every utterance and commits token y[u - 1] into the decoder slots
//   k_align_lattice     the joint over a tile of 16 frames x 8 label positions of one utterance: lb, ly of its 128 cells
//   k_align_recursion   forward (sum) and Viterbi (max) recursions in double over anti-diagonals, one workgroup per utterance, and
//                       the backtrace of the best path
#include "nasr_internal.h"

namespace nasr {

typedef __attribute__((ext_vector_type(4))) float f32x4;
using nasr_align::TILE_T;
using nasr_align::TILE_U;
using nasr_align::TILE_CELLS;

// ---- teacher forcing: one workgroup between the steps of the prediction network ---------------------------------------------------
// step u evaluates the LSTM candidate of every utterance with U >= u from the state after blank, y_0 .. y_{u-1} (u = 0: the fresh state,
// prev_token = blank); this launch first keeps the g rows step u - 1 left in predg, then commits y_{u-1} the way k_dec_commit does
// (prev_token, cur ^= 1) and lists the utterances of step u
__global__ __launch_bounds__(256) void k_align_pred_step(AlignPredParams p) {
    if (p.u > 0)
        for (int i = threadIdx.x; i < p.n * (JNT / 4); i += 256) {
            const int k = i / (JNT / 4), c = i % (JNT / 4);
            const nasr_align::Utt ud = p.utt[k];
            if (ud.U >= p.u - 1) ((float4 *)(p.g + (size_t)(ud.g_row + p.u - 1) * JNT))[c] = ((const float4 *)(p.predg + (size_t)k * JNT))[c];
        }
    // one thread per utterance; the list's order is that of shared-memory tickets, as in build_lists (kernels_decode.hip): every row of the
    // LSTM / joint.pred launches is an independent accumulation chain, so the order cannot change a result
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < p.n; k += 256) {
        const nasr_align::Utt ud = p.utt[k];
        if (p.u > ud.U) continue;
        if (p.u > 0) {
            p.ctrl[k].prev_token = p.tok[ud.tok0 + p.u - 1];
            p.ctrl[k].cur ^= 1;
        }
        p.dlist[atomicAdd(&cnt, 1)] = k;
    }
    __syncthreads();
    if (threadIdx.x == 0) *p.n_dirty = cnt;
}
void launch_align_pred_step(const AlignPredParams &p, hipStream_t st) {
    hipLaunchKernelGGL(k_align_pred_step, dim3(1), dim3(256), 0, st, p);
}

// ---- the lattice joint -----------------------------------------------------------------------------------------------------------
// A workgroup owns TILE_T x TILE_U cells of one utterance.  Its 16 encproj rows and 8 g rows sit in LDS (row stride ES: 16-byte reads of
// 16 rows at one column spread over the banks); relu(e + g) is formed on the fly as the MFMA's B operand, so a cell reads no row from HBM.
// Column tile mt of the MFMA = label position u0 + mt, column r inside it = frame t0 + r; wave w runs the vocabulary tiles w, w + 4, ..
// of the packed out_w (the decode's A fragments, kernels_decode.hip) against all eight column tiles: 32 MFMAs per 1 KiB of weights.
// Per cell the 640 products are summed in one accumulator in one fixed order (k-group after k-group, within a group the MFMA's own order over
// its four k of every component): the sum does not depend on the tile or the launch.
// No logits are written: after each vocabulary tile the wave merges its 16 entries into the running softmax part of every cell
// (nasr_logprob.h: tile_part_wave = lane4 + the xor-16 / xor-32 butterfly, merge in ascending tile order), and the lanes that hold the blank's and y_u's
// logits leave them in LDS.  The four waves' parts meet in LDS and thread c < 128 finishes cell c (nasr_lp::finish over the four parts in
// wave order) and stores its two values.
constexpr int ES = JNT + 4;
constexpr int KG_J = JNT / 16;

__global__ __launch_bounds__(256) void k_align_lattice(AlignParams p) {
    __shared__ __attribute__((aligned(16))) float rows[(TILE_T + TILE_U) * ES];
    __shared__ float blank_lg[TILE_CELLS], tok_lg[TILE_CELLS];
    static_assert(sizeof(nasr_lp::Part) * 4 * TILE_CELLS <= sizeof(float) * (TILE_T + TILE_U) * ES, "the waves' parts fit the row staging");
    float *es = rows, *gs = rows + TILE_T * ES;
    const nasr_align::Tile td = p.tiles[blockIdx.x];
    const nasr_align::Utt ud = p.utt[td.utt];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
    // rows past the lattice's edge repeat its last row: valid memory, their cells are never stored
    for (int i = threadIdx.x; i < (TILE_T + TILE_U) * (JNT / 4); i += 256) {
        const int row = i / (JNT / 4), c = i % (JNT / 4);
        const float *src;
        if (row < TILE_T) { const int t = td.t0 + row < ud.T ? td.t0 + row : ud.T - 1; src = p.encproj + (size_t)(ud.enc_row + t) * JNT; }
        else { const int u = td.u0 + row - TILE_T <= ud.U ? td.u0 + row - TILE_T : ud.U; src = p.g + (size_t)(ud.g_row + u) * JNT; }
        *(float4 *)(rows + row * ES + c * 4) = ((const float4 *)src)[c];
    }
    if (threadIdx.x < TILE_CELLS) { blank_lg[threadIdx.x] = 0.f; tok_lg[threadIdx.x] = 0.f; }
    // the token of every label position of the tile (-1: none, u >= U)
    int tokv[TILE_U];
#pragma unroll
    for (int mt = 0; mt < TILE_U; mt++) tokv[mt] = td.u0 + mt < ud.U ? p.tok[ud.tok0 + td.u0 + mt] : -1;
    __syncthreads();
    nasr_lp::Part run[TILE_U];
#pragma unroll
    for (int mt = 0; mt < TILE_U; mt++) run[mt] = nasr_lp::empty_part();
    const float *er = es + r * ES + q * 4, *gr = gs + q * 4;
    for (int nt = wave; nt < nasr_lp::TILE_PARTS; nt += 4) {
        const float4 *w = (const float4 *)p.out_w + (size_t)nt * KG_J * 64 + lane;
        f32x4 acc[TILE_U];
#pragma unroll
        for (int mt = 0; mt < TILE_U; mt++) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        float4 wn = w[0];
        for (int kg = 0; kg < KG_J; kg++) {
            const float4 wv = wn;
            if (kg + 1 < KG_J) wn = w[(size_t)(kg + 1) * 64];
            const float4 e4 = *(const float4 *)(er + kg * 16);
#pragma unroll
            for (int mt = 0; mt < TILE_U; mt++) {
                const float4 g4 = *(const float4 *)(gr + mt * ES + kg * 16);
                const float x0 = fmaxf(e4.x + g4.x, 0.0f), x1 = fmaxf(e4.y + g4.y, 0.0f), x2 = fmaxf(e4.z + g4.z, 0.0f), x3 = fmaxf(e4.w + g4.w, 0.0f);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.x, x0, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.y, x1, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.z, x2, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.w, x3, acc[mt], 0, 0, 0);
            }
        }
        // lane (q, r) holds the logits of entries v0 .. v0 + 3 of cell (t0 + r, u0 + mt)
        const int v0 = nt * 16 + q * 4;
        float bias[4];
#pragma unroll
        for (int j = 0; j < 4; j++) bias[j] = v0 + j < VOCAB ? p.out_b[v0 + j] : 0.0f;
#pragma unroll
        for (int mt = 0; mt < TILE_U; mt++) {
            float lg[4];
#pragma unroll
            for (int j = 0; j < 4; j++) lg[j] = acc[mt][j] + bias[j];
            run[mt] = nasr_lp::merge(run[mt], nasr_lp::tile_part_wave(lg[0], lg[1], lg[2], lg[3], v0));
            // one lane holds a given entry of a cell: one writer per element
            if (v0 == BLANK) blank_lg[mt * 16 + r] = lg[0];
            const int jt = tokv[mt] - v0;
            if (jt >= 0 && jt < 4) tok_lg[mt * 16 + r] = jt == 0 ? lg[0] : jt == 1 ? lg[1] : jt == 2 ? lg[2] : lg[3];
        }
    }
    __syncthreads();                                   // every wave is done with the rows: the parts take their place
    nasr_lp::Part (*parts)[TILE_CELLS] = (nasr_lp::Part (*)[TILE_CELLS])rows;
    if (q == 0) {
#pragma unroll
        for (int mt = 0; mt < TILE_U; mt++) parts[wave][mt * 16 + r] = run[mt];
    }
    __syncthreads();
    int t, u;
    const long long cell = nasr_align::store_cell(ud, td, threadIdx.x, &t, &u);
    if (cell >= 0) {
        nasr_lp::Part p4[4];
#pragma unroll
        for (int wv = 0; wv < 4; wv++) p4[wv] = parts[wv][threadIdx.x];
        p.lp_blank[cell] = nasr_lp::finish(blank_lg[threadIdx.x], p4, 4);
        p.lp_token[cell] = u < ud.U ? nasr_lp::finish(tok_lg[threadIdx.x], p4, 4) : nasr_lp::neg_inf();
    }
}
void launch_align_lattice(const AlignParams &p, int n_tiles, hipStream_t st) {
    if (n_tiles > 0) hipLaunchKernelGGL(k_align_lattice, dim3(n_tiles), dim3(256), 0, st, p);
}

// ---- recursions + backtrace: one workgroup per utterance ---------------------------------------------------------------------------
// threads run over the label positions of an anti-diagonal t + u = d; the two diagonals d - 1 and d of alpha and delta live in LDS.
// One back-pointer byte per cell goes to global memory; thread 0 walks it back (at most T + U steps).
__global__ __launch_bounds__(256) void k_align_recursion(AlignRecParams p) {
    __shared__ double al[2][nasr_align::MAX_TOKENS + 1], dl[2][nasr_align::MAX_TOKENS + 1];
    const nasr_align::Utt ud = p.utt[blockIdx.x];
    const int T = ud.T, U = ud.U;
    if (T <= 0 || U > nasr_align::MAX_TOKENS) return;
    const float *lb = p.lp_blank + ud.cell0, *ly = p.lp_token + ud.cell0;
    unsigned char *bp = p.bp + ud.cell0;
    for (int d = 0; d <= T - 1 + U; d++) {
        int lo, hi;
        nasr_align::diag_range(d, T, U, &lo, &hi);
        const int cur = d & 1, prev = cur ^ 1;
        for (int u = lo + (int)threadIdx.x; u <= hi; u += 256) {
            const int t = d - u;
            const bool up = t > 0, left = u > 0;
            const nasr_align::Cell c = nasr_align::step(up, up ? al[prev][u] : 0.0, up ? dl[prev][u] : 0.0, up ? lb[nasr_align::cell_index(U, t - 1, u)] : 0.0f,
                                                        left, left ? al[prev][u - 1] : 0.0, left ? dl[prev][u - 1] : 0.0, left ? ly[nasr_align::cell_index(U, t, u - 1)] : 0.0f);
            al[cur][u] = c.alpha; dl[cur][u] = c.delta;
            bp[nasr_align::cell_index(U, t, u)] = c.token_move;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int last = (T - 1 + U) & 1;
        const double end = (double)lb[nasr_align::cell_index(U, T - 1, U)];
        p.scores[2 * blockIdx.x] = al[last][U] + end;
        p.scores[2 * blockIdx.x + 1] = dl[last][U] + end;
        nasr_align::backtrace(bp, ly, T, U, p.frames + ud.tok0, p.tok_lp + ud.tok0);
    }
}
void launch_align_recursion(const AlignRecParams &p, int n, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_align_recursion, dim3(n), dim3(256), 0, st, p);
}

}  // namespace nasr
