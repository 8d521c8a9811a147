// kernels_decode.hip -- device-resident batched RNN-T greedy decode (stage a-12..a-14).
//
// Reference: src/nemo-stream.cpp:840-930 runs, per symbol, 4 host->device copies, one graph
// launch and 1-3 device->host copies for ONE stream, and evaluates LSTMx2 + joint once per
// (frame, symbol).  Here the loop lives on the device for all B streams of a step and is
// re-scheduled around one fact of the reference's rules: a blank leaves the decoder state
// untouched (:908-911), so the prediction network's output only changes when a symbol is emitted.
//   * per stream the LSTM candidate (h', c') and g = joint.pred(h1') + b_pred are CACHED (they persist
//     across steps) and recomputed only for streams whose committed state changed ("dirty");
//   * one iteration evaluates the joint for EVERY frame a stream still has to decode against that
//     cached g -- all (stream, frame) rows of the batch in one f32-MFMA GEMM with the arg-max in the
//     epilogue -- and the commit kernel walks each stream's frames in order up to its first
//     non-blank: the blanks before it are final (state unchanged), the symbol is emitted there
//     (prev_token = best, commit h'/c' :921-926, at most 10 symbols per frame :849), and the frames
//     after it are re-evaluated in the next iteration with the new g.
// A step therefore needs (max symbols emitted by one stream) + 1 iterations instead of
// (frames + symbols); every (frame, state) pair the reference evaluates is evaluated with the same
// inputs, so tokens, the iteration statistic and the committed state are identical.  Arg-max
// keeps the first maximum (:899-906).
//
// All arithmetic is f32 (the reference keeps decoder/joint weights F32 in every GGUF flavour):
// the mat-vec stages are batched over rows and run on the f32-input MFMA
// (v_mfma_f32_16x16x4_f32, bit-exact fmaf chains).  Weights are pre-packed at upload into
// MFMA A-fragment order -- tile (nt, kg) = 16 rows x 16 k is 1 KiB, lane l = q*16 + r holds
// W[row(nt, r)][kg*16 + 4q .. +4) as one float4 = its operand for 4 consecutive MFMAs -- so a
// wave-load is one contiguous 1 KiB read.  The row vectors are the B operand: lane (q, j)
// loads x[row j][kg*16 + 4q .. +4), contiguous as well.  For the LSTM the 16 rows of a tile
// are ordered (unit u, gate g) = (r/4, r%4), which lands the four gates i,f,g,o of one hidden
// unit in the four accumulator registers of one lane: the cell update needs no data movement.
#include "nasr_internal.h"
#include "nasr_step_plan.h"

namespace nasr {

typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

constexpr int KG640 = HID / 16;     // 40 k-groups of 16
constexpr int MT_MAX = 4;           // m-tiles (16 rows each) per pass

// ---- work lists: streams to recompute, (stream, frame) rows to evaluate ---------------------------
// One 256-thread block.  Order inside the lists is arbitrary (shared-memory tickets); every output
// element is an independent accumulation chain, so the order cannot change a result.
__device__ __forceinline__ void build_lists(const DecParams &p, int *sh) {
    __syncthreads();
    if (threadIdx.x < 3) sh[threadIdx.x] = 0;
    __syncthreads();
    for (int b = threadIdx.x; b < p.B; b += 256) {
        const DecCtrl ct = p.ctrl[p.rows[b].slot];
        if (!ct.active) continue;
        atomicAdd(&sh[0], 1);
        if (ct.dirty) p.dlist[atomicAdd(&sh[1], 1)] = b;
        const int n = ct.n_frames - ct.t;
        const int base = atomicAdd(&sh[2], n);
        for (int i = 0; i < n; i++) p.rowmap[base + i] = ((unsigned)(ct.t + i) << 16) | (unsigned)b;
    }
    __syncthreads();
    if (threadIdx.x == 0) { *p.n_active = sh[0]; *p.n_dirty = sh[1]; *p.n_rows = sh[2]; }
}

__global__ __launch_bounds__(256) void k_dec_begin(DecParams p) {
    __shared__ int sh[4];
    for (int b = threadIdx.x; b < p.B; b += 256) {
        const RowDesc rd = p.rows[b];
        DecCtrl *ct = &p.ctrl[rd.slot];
        ct->t = 0;
        ct->n_frames = rd.n_dec;
        ct->symbols = 0;
        ct->row = b;
        ct->active = rd.n_dec > 0 ? 1 : 0;
        ct->frame0 = ct->frame_next;
        ct->frame_next += rd.n_dec;
    }
    for (int i = threadIdx.x; i < p.B * p.T; i += 256) p.key[i] = 0ull;
    __threadfence_block();
    build_lists(p, sh);
}

// acc[mt] += W_tile(nt, kg range) . X   for MT m-tiles; xrow[mt] = this lane's row vector.
// JOINT: the operand is relu(xrow + grow) formed on the fly (src/nemo-ggml.cpp:1210-1217).
// The k-groups are processed in blocks of 5 with every load of the block (weights + row vectors)
// issued before its MFMAs, so a wave has ~25 independent 16-byte loads in flight instead of one.
template <int MT, bool JOINT>
__device__ __forceinline__ void mfma_range(const float4 *wt, int kg0, int kg1, const float *const *xrow,
                                           const float *const *grow, int q, f32x4 *acc) {
    constexpr int KB = JOINT ? (MT > 2 ? 2 : 5) : 5;
    auto fetch = [&](int mt, int kg) -> float4 {
        float4 x = *(const float4 *)(xrow[mt] + kg * 16 + q * 4);
        if (JOINT) {
            const float4 g = *(const float4 *)(grow[mt] + kg * 16 + q * 4);
            x = make_float4(fmaxf(x.x + g.x, 0.0f), fmaxf(x.y + g.y, 0.0f), fmaxf(x.z + g.z, 0.0f), fmaxf(x.w + g.w, 0.0f));
        }
        return x;
    };
    int kg = kg0;
    for (; kg + KB <= kg1; kg += KB) {
        float4 w[KB], x[KB][MT];
#pragma unroll
        for (int u = 0; u < KB; u++) {
            w[u] = wt[(size_t)(kg + u) * 64];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) x[u][mt] = fetch(mt, kg + u);
        }
#pragma unroll
        for (int u = 0; u < KB; u++)
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u].x, x[u][mt].x, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u].y, x[u][mt].y, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u].z, x[u][mt].z, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u].w, x[u][mt].w, acc[mt], 0, 0, 0);
            }
    }
    for (; kg < kg1; kg++) {
        const float4 w = wt[(size_t)kg * 64];
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const float4 x = fetch(mt, kg);
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, x.x, acc[mt], 0, 0, 0);
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, x.y, acc[mt], 0, 0, 0);
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, x.z, acc[mt], 0, 0, 0);
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, x.w, acc[mt], 0, 0, 0);
        }
    }
}

// ---- LSTM layer L over the dirty rows: grid = 160 (4 hidden units per workgroup), 4 waves split K ----
template <int L, int MT>
__device__ __forceinline__ void lstm_pass(const DecParams &p, int i0, int nd, float (*red)[2][MT_MAX][64][4]) {
    const int nt = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = lane >> 4, r = lane & 15;
    const float4 *w_ih = (const float4 *)p.w_ih[L] + (size_t)nt * KG640 * 64 + lane;
    const float4 *w_hh = (const float4 *)p.w_hh[L] + (size_t)nt * KG640 * 64 + lane;
    const int kg0 = wave * (KG640 / 4), kg1 = kg0 + KG640 / 4;
    const float *xr[MT], *hr[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        int i = i0 + mt * 16 + r;
        if (i >= nd) i = i0;                                       // valid memory, result discarded
        const int slot = p.rows[p.dlist[i]].slot;
        const DecCtrl ct = p.ctrl[slot];
        const float *hcom = p.h + (((size_t)slot * 2 + ct.cur) * 2) * HID;
        const float *hnew = p.h + (((size_t)slot * 2 + (ct.cur ^ 1)) * 2) * HID;
        xr[mt] = L == 0 ? p.embed + (size_t)ct.prev_token * HID : hnew;   // layer 1 input = h0'
        hr[mt] = hcom + L * HID;
    }
    f32x4 ai[MT], ah[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) { ai[mt] = (f32x4){0.f, 0.f, 0.f, 0.f}; ah[mt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    mfma_range<MT, false>(w_ih, kg0, kg1, xr, nullptr, q, ai);     // src/nemo-ggml.cpp:595
    mfma_range<MT, false>(w_hh, kg0, kg1, hr, nullptr, q, ah);     // :596
    __syncthreads();                                               // previous pass done with `red`
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int j = 0; j < 4; j++) { red[wave][0][mt][lane][j] = ai[mt][j]; red[wave][1][mt][lane][j] = ah[mt][j]; }
    __syncthreads();
    // wave mt finishes m-tile mt: lane (q, r) holds gates i,f,g,o of unit nt*4+q for its row
    const int mt = wave;
    const int i = i0 + mt * 16 + r;
    if (mt < MT && i < nd) {
        const int slot = p.rows[p.dlist[i]].slot;
        const DecCtrl ct = p.ctrl[slot];
        const int unit = nt * 4 + q;
        float g[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float gi = ((red[0][0][mt][lane][j] + red[1][0][mt][lane][j]) + red[2][0][mt][lane][j]) + red[3][0][mt][lane][j];
            const float gh = ((red[0][1][mt][lane][j] + red[1][1][mt][lane][j]) + red[2][1][mt][lane][j]) + red[3][1][mt][lane][j];
            const int row = j * HID + unit;
            g[j] = ((gi + gh) + p.b_ih[L][row]) + p.b_hh[L][row];     // :597-599
        }
        const float cprev = p.c[(((size_t)slot * 2 + ct.cur) * 2 + L) * HID + unit];
        const float cnew = sigm(g[1]) * cprev + sigm(g[0]) * tanhf(g[2]);   // :615
        p.c[(((size_t)slot * 2 + (ct.cur ^ 1)) * 2 + L) * HID + unit] = cnew;
        p.h[(((size_t)slot * 2 + (ct.cur ^ 1)) * 2 + L) * HID + unit] = sigm(g[3]) * tanhf(cnew);   // :618
    }
}

template <int L>
__global__ __launch_bounds__(256) void k_dec_lstm(DecParams p) {
    const int nd = *p.n_dirty;
    if (nd == 0) return;
    __shared__ float red[4][2][MT_MAX][64][4];
    for (int i0 = 0; i0 < nd; i0 += 16 * MT_MAX) {
        const int left = nd - i0;
        if (left <= 16) lstm_pass<L, 1>(p, i0, nd, red);
        else if (left <= 32) lstm_pass<L, 2>(p, i0, nd, red);
        else lstm_pass<L, 4>(p, i0, nd, red);
    }
}

// ---- g = W_pred . h1' + b_pred for the dirty rows, grid = 40 (src/nemo-ggml.cpp:1207-1208) ---------
template <int MT>
__device__ __forceinline__ void pred_pass(const DecParams &p, int i0, int nd, float (*red)[MT_MAX][64][4]) {
    const int nt = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = lane >> 4, r = lane & 15;
    const float4 *w = (const float4 *)p.pred_w + (size_t)nt * KG640 * 64 + lane;
    const int kg0 = wave * (KG640 / 4), kg1 = kg0 + KG640 / 4;
    const float *xr[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        int i = i0 + mt * 16 + r;
        if (i >= nd) i = i0;
        const int slot = p.rows[p.dlist[i]].slot;
        xr[mt] = p.h + (((size_t)slot * 2 + (p.ctrl[slot].cur ^ 1)) * 2 + 1) * HID;   // h1'
    }
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    mfma_range<MT, false>(w, kg0, kg1, xr, nullptr, q, acc);
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int j = 0; j < 4; j++) red[wave][mt][lane][j] = acc[mt][j];
    __syncthreads();
    const int mt = wave;
    const int i = i0 + mt * 16 + r;
    if (mt < MT && i < nd) {
        const int slot = p.rows[p.dlist[i]].slot;
        float4 o;
        float *op = (float *)&o;
#pragma unroll
        for (int j = 0; j < 4; j++)
            op[j] = (((red[0][mt][lane][j] + red[1][mt][lane][j]) + red[2][mt][lane][j]) + red[3][mt][lane][j]) + p.pred_b[nt * 16 + q * 4 + j];
        *(float4 *)(p.predg + (size_t)slot * JNT + nt * 16 + q * 4) = o;
    }
}

// ---- engine option "lm_fusion" (nasr_lm.h): the bias row of a slot = phrase bonus + lmbias of every vocabulary entry in the slot's
// states, and beside it the LM state after emitting that entry.  One thread per entry runs the lookup against the tables in device memory.  Both
// states move only in k_dec_commit, which marks the stream dirty, so refreshing the rows of the streams in dlist keeps every row current; a
// slot that did not emit is not touched.  boost_bonus / boost_state are null when "phrase_boost" is off
__device__ __forceinline__ void lm_refresh_entry(const nasr_lm::Greedy *blk, const int32_t *lm_state, float *lm_row, int32_t *lm_next, const float *boost_bonus,
                                                 const int *boost_state, int slot, int v) {
    int32_t next;
    const float lb = nasr_lm::lmbias(*blk, lm_state[slot], v, &next);
    const float bb = boost_bonus ? nasr_boost::bonus_of(boost_bonus, boost_state[slot], v) : 0.0f;
    lm_row[(size_t)slot * nasr_lm::ROW_COLS + v] = bb + lb;
    lm_next[(size_t)slot * nasr_lm::ROW_COLS + v] = next;
}
// the rows of the dirty streams, workgroups first .. first + n - 1 of the grid striding over (dirty stream, entry)
__device__ __forceinline__ void lm_refresh_dirty(const DecParams &p, int nd, int first, int n) {
    const int total = nd * nasr_lm::ROW_COLS;
    for (int i = ((int)blockIdx.x - first) * 256 + (int)threadIdx.x; i < total; i += n * 256) {
        const int d = i / nasr_lm::ROW_COLS, v = i - d * nasr_lm::ROW_COLS;
        lm_refresh_entry(p.lm_blk, p.lm_state, p.lm_row, p.lm_next, p.boost_bonus, p.boost_state, p.rows[p.dlist[d]].slot, v);
    }
}
// form (a): a launch of its own beside k_dec_pred
__global__ __launch_bounds__(256) void k_dec_lmrows(DecParams p) {
    const int nd = *p.n_dirty;
    if (nd == 0) return;
    lm_refresh_dirty(p, nd, 0, (int)gridDim.x);
}
// the rows of slots slot0 .. slot0 + n - 1 whatever their streams do: after nasr_engine_set_lm, the weight setter, a new phrase set, a stream's switch
__global__ __launch_bounds__(256) void k_lm_rows_slots(const nasr_lm::Greedy *blk, const int32_t *lm_state, float *lm_row, int32_t *lm_next, const float *boost_bonus,
                                                       const int *boost_state, int slot0, int n) {
    const int total = n * nasr_lm::ROW_COLS;
    for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < total; i += (int)gridDim.x * 256) {
        const int d = i / nasr_lm::ROW_COLS;
        lm_refresh_entry(blk, lm_state, lm_row, lm_next, boost_bonus, boost_state, slot0 + d, i - d * nasr_lm::ROW_COLS);
    }
}
static int lm_refresh_blocks(int B) { return 5 * (B < 32 ? B : 32); }      // 1040 entries = 4.06 workgroups of 256 per stream

// LMROWS: form (b) of the refresh -- the workgroups past the 40 of the projection stride over the bias rows of the same dirty streams
template <bool LMROWS = false>
__global__ __launch_bounds__(256) void k_dec_pred(DecParams p) {
    const int nd = *p.n_dirty;
    if (nd == 0) return;
    if (LMROWS) {
        if ((int)blockIdx.x >= JNT / 16) { lm_refresh_dirty(p, nd, JNT / 16, (int)gridDim.x - JNT / 16); return; }
    }
    __shared__ float red[4][MT_MAX][64][4];
    for (int i0 = 0; i0 < nd; i0 += 16 * MT_MAX) {
        const int left = nd - i0;
        if (left <= 16) pred_pass<1>(p, i0, nd, red);
        else if (left <= 32) pred_pass<2>(p, i0, nd, red);
        else pred_pass<4>(p, i0, nd, red);
    }
}

using nasr_lp::pack_key;                                            // (order-preserving logit bits) << 32 | (0xffffffff - index), nasr_logprob.h
static_assert(nasr_lp::LP_VOCAB == VOCAB && nasr_lp::SMALL_ROWS == 64, "nasr_logprob.h restates the joint kernels' shapes");
static_assert(nasr_lp::TILE_PARTS == 65 && nasr_lp::TILE_W == 16 && nasr_lp::WG_W == 64 && nasr_boost::VOCAB == VOCAB && nasr_boost::BLANK == BLANK && nasr_boost::COLS == 16 * ((VOCAB + 15) / 16), "nasr_boost.h restates the joint kernels' shapes");
// engine option "token_logprobs": the (max, sum of exp) part of a 16-entry vocab tile, lane (q, r) holding entries v0 .. v0 + 3 of row r's
// logits: nasr_lp::tile_part_wave (nasr_logprob.h, shared with kernels_align.hip)
__device__ __forceinline__ nasr_lp::Part lp_tile_part(float x0, float x1, float x2, float x3, int v0) { return nasr_lp::tile_part_wave(x0, x1, x2, x3, v0); }
// a copy of v the optimiser knows nothing about: what is computed from it shares no subexpression with what is computed from v
__device__ __forceinline__ float ent_opaque(float v) { asm volatile("" : "+v"(v)); return v; }
template <class Tp> __device__ __forceinline__ const Tp *ent_opaque(const Tp *v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ unsigned long long kmax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
    const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
    return ((unsigned long long)hi << 32) | lo;
}
// engine option "token_alternatives" (nasr_topk.h): the 8 largest RAW-logit keys of a 16-entry vocab tile, sorted, lane (q, r) holding entries
// v0 .. v0 + 3 of row r's logits; every lane of the row ends up with the same list (keys are unique).  After the xor-16 step a list has at
// most 8 entries, of which a lane contributes four: only those cross the lanes
__device__ __forceinline__ void alt_tile_keys(float x0, float x1, float x2, float x3, int v0, unsigned long long *a) {
    unsigned long long b[nasr_topk::KMAX];
    nasr_topk::lane_keys(x0, x1, x2, x3, v0, a);
#pragma unroll
    for (int j = 0; j < nasr_topk::KMAX; j++) b[j] = j < 4 ? shfl_xor_u64(a[j], 16) : 0ull;
    nasr_topk::merge8(a, b);
#pragma unroll
    for (int j = 0; j < nasr_topk::KMAX; j++) b[j] = shfl_xor_u64(a[j], 32);
    nasr_topk::merge8(a, b);
}

// ---- joint, few rows (<= 64 rows in the step): logits = W_out . relu(encproj[row] + g) + b_out and
// arg-max; grid = 65 (1040 padded vocab rows), 4 waves split K; first maximum wins (:899-906, :1220-1221)
// BOOST (engine option "phrase_boost", nasr_boost.h): the arg-max key is built from logit + bonus(automaton state of the row's slot, v) -- one
// 16-byte load per lane and row -- while the softmax parts stay those of the raw logits; with LP the lane that owns the tile's winner also leaves
// its raw logit in boost_raw [row][part] (one writer per element: a key names one vocabulary entry, and one lane holds it)
// ALT (engine option "token_alternatives", nasr_topk.h; always with LP): lane group 0 also leaves the tile's alt_k largest raw-logit keys in
// alt_key [row][part][alt_k], beside the part
// ENT (engine option "token_entropy", nasr_entropy.h; always with LP): lane group 0 also leaves the tile's entropy term in ent_part [row][part],
// beside the part.  The code that forms the part is the code of the form without ENT, and the term is computed AFTER it, from opaque copies of
// the logits and behind a test of its own (ent_opaque): the compiler contracts a * b + c * d into one of two FMAs or none depending on what
// else uses the products and on what the vectoriser pairs inside a basic block, so a term computed in one expression with the part moved the
// part's last bit (seen on the MI355X: ln P and the blank values differed in one ulp between the option on and off).  The price is that the
// pass repeats the part's exps
template <int MT, bool LP, bool BOOST, bool ALT, bool LMF, bool ENT>
__device__ __forceinline__ void joint_pass(const DecParams &p, int i0, int nr, float (*red)[MT_MAX][64][4]) {
    const int nt = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = lane >> 4, r = lane & 15;
    const float4 *w = (const float4 *)p.out_w + (size_t)nt * KG640 * 64 + lane;
    const int kg0 = wave * (KG640 / 4), kg1 = kg0 + KG640 / 4;
    const float *er[MT], *gr[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        int i = i0 + mt * 16 + r;
        if (i >= nr) i = i0;
        const unsigned rm = p.rowmap[i];
        const int b = (int)(rm & 0xffffu), f = (int)(rm >> 16);
        er[mt] = p.encproj + ((size_t)b * p.T + f) * JNT;
        gr[mt] = p.predg + (size_t)p.rows[b].slot * JNT;
    }
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    mfma_range<MT, true>(w, kg0, kg1, er, gr, q, acc);
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int j = 0; j < 4; j++) red[wave][mt][lane][j] = acc[mt][j];
    __syncthreads();
    const int mt = wave;
    const int i = i0 + mt * 16 + r;
    if (mt < MT) {
        unsigned long long best = 0ull;
        float lgs[4] = {0.f, 0.f, 0.f, 0.f}, bon[4] = {0.f, 0.f, 0.f, 0.f};
        if (BOOST) {
            const int slot = p.rows[p.rowmap[i < nr ? i : i0] & 0xffffu].slot;
            const nasr_boost::Bonus4 b4 = LMF ? *(const nasr_boost::Bonus4 *)(p.lm_row + (size_t)slot * nasr_lm::ROW_COLS + nt * 16 + q * 4)
                                              : nasr_boost::bonus4_of(p.boost_bonus, p.boost_state[slot], nt * 16 + q * 4);
            bon[0] = b4.x; bon[1] = b4.y; bon[2] = b4.z; bon[3] = b4.w;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int v = nt * 16 + q * 4 + j;
            if (v < VOCAB) {
                const float lg = (((red[0][mt][lane][j] + red[1][mt][lane][j]) + red[2][mt][lane][j]) + red[3][mt][lane][j]) + p.out_b[v];
                best = kmax(best, pack_key(BOOST ? lg + bon[j] : lg, v));
                if (LP) lgs[j] = lg;
            }
        }
        best = kmax(best, shfl_xor_u64(best, 16));
        best = kmax(best, shfl_xor_u64(best, 32));
        if (LP && BOOST) {
            const int wv = nasr_lp::key_index_of(best) - (nt * 16 + q * 4);
            if (best && i < nr && wv >= 0 && wv < 4)
                p.boost_raw[nasr_lp::scratch_index(nasr_lp::key_index(p.rowmap[i], p.T), nt, nasr_lp::TILE_PARTS)] = wv == 0 ? lgs[0] : wv == 1 ? lgs[1] : wv == 2 ? lgs[2] : lgs[3];
        }
        if (q == 0 && i < nr && best) {
            const unsigned rm = p.rowmap[i];
            atomicMax(&p.key[(size_t)(rm & 0xffffu) * p.T + (rm >> 16)], best);
        }
        if (LP) {                                      // one part per 16-entry tile: part nt of the row, written by lane group 0
            const nasr_lp::Part part = lp_tile_part(lgs[0], lgs[1], lgs[2], lgs[3], nt * 16 + q * 4);
            const int row = nasr_lp::joint_store_row(i0, MT, wave, lane, nr);
            if (row >= 0) p.lp_part[nasr_lp::scratch_index(nasr_lp::key_index(p.rowmap[row], p.T), nt, nasr_lp::TILE_PARTS)] = part;
            if (ALT) {
                unsigned long long top[nasr_topk::KMAX];
                alt_tile_keys(lgs[0], lgs[1], lgs[2], lgs[3], nt * 16 + q * 4, top);
                if (row >= 0) {
                    unsigned long long *dst = p.alt_key + nasr_topk::scratch_index(nasr_lp::key_index(p.rowmap[row], p.T), nt, nasr_lp::TILE_PARTS, p.alt_k);
#pragma unroll
                    for (int j = 0; j < nasr_topk::KMAX; j++) if (j < p.alt_k) dst[j] = top[j];
                }
            }
            if (ENT) {
                if (p.ent_part) {                      // bound whenever this form is launched: the test keeps the pass in basic blocks of its own (ent_opaque)
                    const nasr_ent::EPart ep = nasr_ent::tile_wave(ent_opaque(lgs[0]), ent_opaque(lgs[1]), ent_opaque(lgs[2]), ent_opaque(lgs[3]), nt * 16 + q * 4, p.ent_alpha);
                    if (row >= 0) p.ent_part[nasr_lp::scratch_index(nasr_lp::key_index(p.rowmap[row], p.T), nt, nasr_lp::TILE_PARTS)] = ep.e;
                }
            }
        }
    }
}

// LMF (engine option "lm_fusion", always with BOOST): the lane's four bias entries come from the slot's row (phrase bonus + lmbias, k_dec_lmrows)
// instead of the automaton's table; everything else is the boosted form
template <bool LP, bool BOOST, bool ALT, bool LMF = false, bool ENT = false>
__global__ __launch_bounds__(256) void k_dec_joint(DecParams p) {
    static_assert(BOOST || !LMF, "the fused form is a form of the boosted kernel");
    static_assert(LP || !ENT, "the entropy terms ride on the softmax parts");
    const int nr = *p.n_rows;
    if (nr == 0) return;
    __shared__ float red[4][MT_MAX][64][4];
    for (int i0 = 0; i0 < nr; i0 += 16 * MT_MAX) {
        const int tiles = nasr_lp::joint_pass_tiles(nr - i0);      // 1, 2 or 4 m-tiles: 16, 32 or more rows left
        if (tiles == 1) joint_pass<1, LP, BOOST, ALT, LMF, ENT>(p, i0, nr, red);
        else if (tiles == 2) joint_pass<2, LP, BOOST, ALT, LMF, ENT>(p, i0, nr, red);
        else joint_pass<4, LP, BOOST, ALT, LMF, ENT>(p, i0, nr, red);
    }
}

// ---- joint, many rows: 64 rows x 64 vocab entries per workgroup, grid = (17, ceil(B*T / 64)).
// Wave w owns vocab tile 4*blockIdx.x + w (weights straight from global, already in fragment order)
// and all four 16-row tiles; the relu(encproj + g) operand of a 64-deep K chunk is formed once per
// workgroup and staged in LDS (double-buffered, 16-byte chunks XOR-swizzled with the row).  The
// kernel is bound by the f32 MFMA (32 cycles per 16x16x4), 640 of them per wave.
// BEAMB (the boosted beam evaluation, launch_decode_rows_boost; always with LP, BOOST and ALT): the ALT lists are built from logit + bonus(state
// of the row's slot, v) instead of the raw logit, the softmax parts stay those of the raw logits, and every lane also leaves its four RAW logits
// of every row in raw_logits [row][1040] -- one aligned 16-byte store per lane and m-tile from the accumulators it holds, one writer per element.
// The per-part winner's raw logit (boost_raw) is not kept: the select kernel reads any entry's raw logit from the row
constexpr int JT_KC = 64;                       // K per LDS chunk = 4 k-groups
// LMF: as in k_dec_joint -- bstate holds the row's slot, and the four bias entries are one load from the slot's row
// ENT: as in k_dec_joint -- a pass of its own behind the form without ENT leaves the workgroup's entropy term beside its part
template <bool LP, bool BOOST, bool ALT, bool BEAMB = false, bool LMF = false, bool ENT = false>
__global__ __launch_bounds__(256) void k_dec_joint_tiled(DecParams p) {
    static_assert(!ENT || (LP && !BEAMB), "the entropy terms ride on the softmax parts of the greedy kernel");
    static_assert(!BEAMB || (LP && BOOST && ALT), "the boosted beam form is a form of the LP + BOOST + ALT kernel");
    static_assert(!LMF || (BOOST && !BEAMB), "the fused form is a form of the boosted greedy kernel");
    const int nr = *p.n_rows;
    const int m0 = blockIdx.y * 64;
    if (m0 >= nr) return;
    __shared__ __attribute__((aligned(16))) float xs[2][64 * JT_KC];
    __shared__ unsigned long long bests[4][64];
    __shared__ nasr_lp::Part lps[LP ? 4 : 1][64];      // token_logprobs: the four waves' tile parts of the 64 rows
    __shared__ nasr_lp::Part elps[ENT ? 4 : 1][64];    // token_entropy: the four waves' tile parts once more, and their entropy terms (3 KiB)
    __shared__ float ents[ENT ? 4 : 1][64];
    __shared__ float raws[LP && BOOST && !BEAMB ? 4 : 1][64];    // ... with phrase_boost: the raw logit of each wave's winner by boosted key
    // token_alternatives: the four waves' tile lists of the 64 rows, [wave][entry][row].  They take the place of the operand staging, which nobody
    // reads after the K loop's last barrier
    static_assert(sizeof(unsigned long long) * 4 * nasr_topk::KMAX * 64 <= sizeof(float) * 2 * 64 * JT_KC, "the lists fit the staging buffer");
    unsigned long long (*alts)[nasr_topk::KMAX][64] = (unsigned long long (*)[nasr_topk::KMAX][64])&xs[0][0];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
    const int nt = blockIdx.x * 4 + wave;
    const bool has_tile = nt * 16 < VOCAB;
    const float4 *w = (const float4 *)p.out_w + (size_t)(has_tile ? nt : 0) * KG640 * 64 + lane;
    int nmt = (nr - m0 + 15) >> 4;
    if (nmt > 4) nmt = 4;
    // staging role: thread -> (row, four 16-byte chunks)
    const int srow = threadIdx.x >> 2, sc0 = (threadIdx.x & 3) * 4;
    const unsigned srm = p.rowmap[m0 + srow < nr ? m0 + srow : m0];
    const float *erow = p.encproj + ((size_t)(srm & 0xffffu) * p.T + (srm >> 16)) * JNT + sc0 * 4;
    const float *grow = p.predg + (size_t)p.rows[srm & 0xffffu].slot * JNT + sc0 * 4;
    float4 ev[4], gv[4], wv[4], wn[4];
    auto gload = [&](int kc) {
#pragma unroll
        for (int i = 0; i < 4; i++) { ev[i] = *(const float4 *)(erow + kc * JT_KC + i * 4); gv[i] = *(const float4 *)(grow + kc * JT_KC + i * 4); }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float4 x = make_float4(fmaxf(ev[i].x + gv[i].x, 0.0f), fmaxf(ev[i].y + gv[i].y, 0.0f),
                                         fmaxf(ev[i].z + gv[i].z, 0.0f), fmaxf(ev[i].w + gv[i].w, 0.0f));
            *(float4 *)(&xs[buf][srow * JT_KC + (((sc0 + i) ^ (srow & 15)) << 2)]) = x;
        }
    };
    int bstate[4] = {0, 0, 0, 0};                   // phrase_boost: automaton state of this lane's row of every m-tile (it moves only in k_dec_commit)
    if (BOOST) {
#pragma unroll
        for (int mt = 0; mt < 4; mt++) {
            const int row = m0 + mt * 16 + r;
            const int slot = p.rows[p.rowmap[row < nr ? row : m0] & 0xffffu].slot;
            bstate[mt] = LMF ? slot : p.boost_state[slot];
        }
    }
    f32x4 acc[4];
#pragma unroll
    for (int mt = 0; mt < 4; mt++) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    gload(0);
#pragma unroll
    for (int u = 0; u < 4; u++) wv[u] = w[(size_t)u * 64];
    sstore(0);
    __syncthreads();
    constexpr int NKC = JNT / JT_KC;            // 10
    for (int kc = 0; kc < NKC; kc++) {
        const int cur = kc & 1;
        if (kc + 1 < NKC) {
            gload(kc + 1);
#pragma unroll
            for (int u = 0; u < 4; u++) wn[u] = w[(size_t)((kc + 1) * 4 + u) * 64];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int mt = 0; mt < 4; mt++) {
                if (mt < nmt) {
                    const float4 x = *(const float4 *)(&xs[cur][(mt * 16 + r) * JT_KC + (((u * 4 + q) ^ r) << 2)]);
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u].x, x.x, acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u].y, x.y, acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u].z, x.z, acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u].w, x.w, acc[mt], 0, 0, 0);
                }
            }
        }
        if (kc + 1 < NKC) {
            sstore(cur ^ 1);
#pragma unroll
            for (int u = 0; u < 4; u++) wv[u] = wn[u];
        }
        __syncthreads();
    }
    // arg-max: in-lane over the 4 vocab entries, across the 4 lane groups, across the 4 waves, then one
    // atomic per row
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {
        unsigned long long best = 0ull;
        float bon[4] = {0.f, 0.f, 0.f, 0.f};
        if (has_tile && mt < nmt) {
            if (BOOST) {
                const nasr_boost::Bonus4 b4 = LMF ? *(const nasr_boost::Bonus4 *)(p.lm_row + (size_t)bstate[mt] * nasr_lm::ROW_COLS + nt * 16 + q * 4)
                                                  : nasr_boost::bonus4_of(p.boost_bonus, bstate[mt], nt * 16 + q * 4);
                bon[0] = b4.x; bon[1] = b4.y; bon[2] = b4.z; bon[3] = b4.w;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int v = nt * 16 + q * 4 + j;
                if (v < VOCAB) best = kmax(best, pack_key(BOOST ? (acc[mt][j] + p.out_b[v]) + bon[j] : acc[mt][j] + p.out_b[v], v));
            }
        }
        best = kmax(best, shfl_xor_u64(best, 16));
        best = kmax(best, shfl_xor_u64(best, 32));
        if (q == 0) bests[wave][mt * 16 + r] = best;
        if (LP && BOOST && !BEAMB) {                   // the lane that holds the wave's winner leaves its raw logit
            const int wv = nasr_lp::key_index_of(best) - (nt * 16 + q * 4);
            if (best && wv >= 0 && wv < 4) {
                const float a = wv == 0 ? acc[mt][0] : wv == 1 ? acc[mt][1] : wv == 2 ? acc[mt][2] : acc[mt][3];
                raws[wave][mt * 16 + r] = a + p.out_b[nt * 16 + q * 4 + wv];
            }
        }
        if (LP) {
            const int v0 = has_tile ? nt * 16 + q * 4 : VOCAB;          // no tile: the empty part
            float lg[4];
#pragma unroll
            for (int j = 0; j < 4; j++) lg[j] = acc[mt][j] + p.out_b[v0 + j < VOCAB ? v0 + j : 0];
            const nasr_lp::Part part = lp_tile_part(lg[0], lg[1], lg[2], lg[3], v0);
            if (q == 0) lps[wave][mt * 16 + r] = part;
            if (BEAMB) {                               // the row's raw logits of this lane: columns 16 nt + 4 q .. + 3 of [row][1040], nt < 65
                const int row = m0 + mt * 16 + r;
                if (has_tile && row < nr)
                    *(float4 *)(p.raw_logits + (size_t)nasr_lp::key_index(p.rowmap[row], p.T) * nasr_boost::COLS + v0) = make_float4(lg[0], lg[1], lg[2], lg[3]);
            }
            if (ALT) {                                 // no tile: v0 = VOCAB leaves the empty list
                unsigned long long top[nasr_topk::KMAX];
                if (BEAMB) alt_tile_keys(lg[0] + bon[0], lg[1] + bon[1], lg[2] + bon[2], lg[3] + bon[3], v0, top);   // bon is 0 where the wave has no tile or the m-tile no row
                else alt_tile_keys(lg[0], lg[1], lg[2], lg[3], v0, top);
                if (q == 0) {
#pragma unroll
                    for (int j = 0; j < nasr_topk::KMAX; j++) alts[wave][j][mt * 16 + r] = top[j];
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 64 && m0 + threadIdx.x < nr) {
        const unsigned long long best = kmax(kmax(bests[0][threadIdx.x], bests[1][threadIdx.x]), kmax(bests[2][threadIdx.x], bests[3][threadIdx.x]));
        const unsigned rm = p.rowmap[m0 + threadIdx.x];
        if (best) atomicMax(&p.key[(size_t)(rm & 0xffffu) * p.T + (rm >> 16)], best);
        if (LP && BOOST && !BEAMB) {                   // the workgroup's winner is the winner of its wave: part blockIdx.x of the row
            int w = 0;
            unsigned long long kw = bests[0][threadIdx.x];
#pragma unroll
            for (int u = 1; u < 4; u++) if (bests[u][threadIdx.x] > kw) { kw = bests[u][threadIdx.x]; w = u; }
            if (kw) p.boost_raw[nasr_lp::scratch_index(nasr_lp::key_index(rm, p.T), blockIdx.x, nasr_lp::WG_PARTS)] = raws[w][threadIdx.x];
        }
    }
    if (LP) {                                      // one part per workgroup (64 entries): part blockIdx.x of the row, waves merged in order
        const int row = nasr_lp::tiled_store_row(blockIdx.y, threadIdx.x, nr);
        if (row >= 0) {
            const nasr_lp::Part part = nasr_lp::wg64(lps[0][threadIdx.x], lps[1][threadIdx.x], lps[2][threadIdx.x], lps[3][threadIdx.x]);
            p.lp_part[nasr_lp::scratch_index(nasr_lp::key_index(p.rowmap[row], p.T), blockIdx.x, nasr_lp::WG_PARTS)] = part;
            if (ALT) {                                 // the workgroup's list: its four waves' lists merged in wave order
                unsigned long long top[nasr_topk::KMAX], w[nasr_topk::KMAX];
#pragma unroll
                for (int j = 0; j < nasr_topk::KMAX; j++) top[j] = alts[0][j][threadIdx.x];
#pragma unroll
                for (int u = 1; u < 4; u++) {
#pragma unroll
                    for (int j = 0; j < nasr_topk::KMAX; j++) w[j] = alts[u][j][threadIdx.x];
                    nasr_topk::merge8(top, w);
                }
                unsigned long long *dst = p.alt_key + nasr_topk::scratch_index(nasr_lp::key_index(p.rowmap[row], p.T), blockIdx.x, nasr_lp::WG_PARTS, p.alt_k);
#pragma unroll
                for (int j = 0; j < nasr_topk::KMAX; j++) if (j < p.alt_k) dst[j] = top[j];
            }
        }
    }
    if (ENT) {
        // the entropy terms, after everything the form without ENT does and apart from it (k_dec_joint, ent_opaque): every wave's tile parts and
        // terms of the 64 rows once more from opaque copies of the logits, then the workgroup's four in wave order, stored beside the part
        if (p.ent_part) {
#pragma unroll
            for (int mt = 0; mt < 4; mt++) {
                const int v0 = has_tile ? nt * 16 + q * 4 : VOCAB;
                float lg[4];
#pragma unroll
                for (int j = 0; j < 4; j++) lg[j] = ent_opaque(acc[mt][j]) + p.out_b[v0 + j < VOCAB ? v0 + j : 0];
                const nasr_ent::EPart ep = nasr_ent::tile_wave(lg[0], lg[1], lg[2], lg[3], v0, p.ent_alpha);
                if (q == 0) { elps[wave][mt * 16 + r] = ep.p; ents[wave][mt * 16 + r] = ep.e; }
            }
            __syncthreads();
            const int row = nasr_lp::tiled_store_row(blockIdx.y, threadIdx.x, nr);
            if (row >= 0) {
                const int t = threadIdx.x;
                const nasr_ent::EPart ep = nasr_ent::wg64({elps[0][t], ents[0][t]}, {elps[1][t], ents[1][t]}, {elps[2][t], ents[2][t]}, {elps[3][t], ents[3][t]}, p.ent_alpha);
                p.ent_part[nasr_lp::scratch_index(nasr_lp::key_index(p.rowmap[row], p.T), blockIdx.x, nasr_lp::WG_PARTS)] = ep.e;
            }
        }
    }
}

// ---- commit: walk each stream's evaluated frames up to its first non-blank -------------------------
// FB (engine option "frame_blank_logprobs", always with LP): first the whole workgroup, one thread per rowmap row, leaves ln P(blank) of every row
// this iteration's joint kernel evaluated in fb_row (indexed like key; nasr_lp::blank_lp over the row's softmax parts, whose last part is blank
// alone; one writer per element).  That is row-parallel work inside the launch that exists: as a kernel of its own between the joint and the
// commit it cost a launch slot in EVERY iteration of a captured decode, idle ones included -- 10 % of a pipelined 1-stream step against 6 %
// here, 0.9 % against 0.6 % at 64 streams x R = 13 (profiles/frame_blank.md).  Then the stream's thread copies the values of the frames this iteration leaves -- [t0, new t): the blanks
// before the token, every frame when there is no token, and the token's own frame when it reaches MAX_SYMBOLS.  All of them are in rowmap
// (build_lists lists every frame from t to n_frames), so the value copied is that of the LAST evaluation on the frame
// LMF (engine option "lm_fusion", always with BOOST): the slot's LM state becomes the `next` the refresh left beside the bias entry of the token;
// the phrase automaton advances where "phrase_boost" is on too (boost_next is null otherwise)
// ENT (engine option "token_entropy", always with LP): the token's thread also finishes the entropy of the frame it commits from the parts and
// their entropy terms (nasr_ent::finish, f64 inside, rounded once) into tok_entropy, where it writes tok_logprob
template <bool LP, bool BOOST, bool ALT, bool FB, bool LMF = false, bool ENT = false>
__global__ __launch_bounds__(256) void k_dec_commit(DecParams p) {
    static_assert(LP || !FB, "the blank log-probabilities come from the softmax parts");
    static_assert(LP || !ENT, "the entropy comes from the softmax parts");
    static_assert(BOOST || !LMF, "the fused form is a form of the boosted kernel");
    __shared__ int sh[4];
    if (*p.n_active == 0) return;
    const int nd = *p.n_dirty;
    for (int i = threadIdx.x; i < nd; i += 256) p.ctrl[p.rows[p.dlist[i]].slot].dirty = 0;   // candidates are fresh now
    if (FB) {
        const int nr = *p.n_rows, np = nasr_lp::n_parts(p.B * p.T);
        for (int i = threadIdx.x; i < nr; i += 256) {
            const int ki = nasr_lp::key_index(p.rowmap[i], p.T);
            p.fb_row[ki] = (float)nasr_lp::blank_lp(p.lp_part + nasr_lp::scratch_index(ki, 0, np), np);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < p.B; b += 256) {
        const int slot = p.rows[b].slot;
        DecCtrl *ct = &p.ctrl[slot];
        if (!ct->active) continue;
        const int t0 = ct->t, nf = ct->n_frames;
        int f = t0, best = BLANK;
        unsigned long long k = 0ull;
        for (; f < nf; f++) {
            k = p.key[(size_t)b * p.T + f];
            best = (int)(0xffffffffu - (uint32_t)(k & 0xffffffffull));
            if (best != BLANK) break;                  // blank: next frame, state untouched (src/nemo-stream.cpp:908-911)
        }
        for (int g = t0; g < nf; g++) p.key[(size_t)b * p.T + g] = 0ull;
        if (f >= nf) {
            ct->iterations += nf - t0;
            ct->t = nf;
            ct->symbols = 0;
            ct->active = 0;
        } else {                                       // :921-926
            ct->iterations += f - t0 + 1;
            int sym = f > t0 ? 0 : ct->symbols;
            const int n = ct->n_tok;
            p.tok_ring[(size_t)slot * TOK_CAP + (n & (TOK_CAP - 1))] = best;
            p.tok_frame[(size_t)slot * TOK_CAP + (n & (TOK_CAP - 1))] = ct->frame0 + f;
            if (LP) {                                  // the parts of frame f were written by this iteration's joint kernel (f is in rowmap)
                const int np = nasr_lp::n_parts(p.B * p.T);
                const nasr_lp::Part *parts = p.lp_part + nasr_lp::scratch_index(b * p.T + f, 0, np);
                // phrase_boost: the key holds logit + bonus; the value stays the MODEL's probability of the token, from its raw logit
                const float logit = BOOST ? p.boost_raw[nasr_lp::scratch_index(b * p.T + f, nasr_boost::raw_part_of(best, np), np)] : nasr_lp::key_logit(k);
                if (ENT) {
                    if (p.tok_entropy)                     // always bound here; the parts are read through an opaque pointer: finish shares no product with the log-probability's sum (k_dec_joint, ent_opaque)
                        p.tok_entropy[(size_t)slot * TOK_CAP + (n & (TOK_CAP - 1))] = nasr_ent::finish(ent_opaque(parts), p.ent_part + nasr_lp::scratch_index(b * p.T + f, 0, np), np, p.ent_alpha);
                }
                if (!ALT) p.tok_logprob[(size_t)slot * TOK_CAP + (n & (TOK_CAP - 1))] = nasr_lp::finish(logit, parts, np);
                else {
                    // token_alternatives: this thread merges the frame's slice lists itself -- the streams of a step are merged side by side, one
                    // thread each; most slices end at their head, and the heads are loaded eight at a time (row_merge).  The token's own value comes from the same
                    // (m, log s), so it equals the entry of the alternatives that names the token bit for bit
                    float m, log_s;
                    nasr_topk::row_softmax(parts, np, &m, &log_s);
                    p.tok_logprob[(size_t)slot * TOK_CAP + (n & (TOK_CAP - 1))] = nasr_topk::lp_of(logit, m, log_s);
                    const int K = p.alt_k;
                    nasr_topk::RowTop rt;
                    nasr_topk::row_begin(rt);
                    nasr_topk::row_merge(rt, K, p.alt_key + nasr_topk::scratch_index(b * p.T + f, 0, np, K), np);
                    const size_t at = nasr_topk::ring_index(slot, n, TOK_CAP, K);
#pragma unroll
                    for (int j = 0; j < nasr_topk::KMAX; j++)
                        if (j < K) { p.alt_id[at + j] = nasr_topk::alt_id(rt.top[j]); p.alt_lp[at + j] = nasr_topk::alt_lp(rt.top[j], m, log_s); }
                }
            }
            if (BOOST && (!LMF || p.boost_next)) p.boost_state[slot] = nasr_boost::next_of(p.boost_next, p.boost_state[slot], best);   // the history moves where the decoder state does
            if (LMF) {
                if (p.lm_relook) {                         // measurement only: look (state, token) up once more instead of reading the next-state row
                    int32_t nx;
                    (void)nasr_lm::lmbias(*p.lm_blk, p.lm_state[slot], best, &nx);
                    p.lm_state[slot] = nx;
                } else p.lm_state[slot] = p.lm_next[(size_t)slot * nasr_lm::ROW_COLS + best];
            }
            ct->n_tok = n + 1;
            ct->prev_token = best;
            ct->cur ^= 1;
            ct->dirty = 1;
            int t = f;
            if (++sym >= MAX_SYMBOLS) { t++; sym = 0; }   // :849, :865
            ct->t = t;
            ct->symbols = sym;
            if (t >= nf) ct->active = 0;
        }
        if (FB) {
            float *ring = p.frame_blank + (size_t)slot * FRAME_CAP;
            const int t1 = ct->t, g0 = ct->frame0;
            for (int g = t0; g < t1; g++) ring[(unsigned)(g0 + g) & (unsigned)(FRAME_CAP - 1)] = p.fb_row[(size_t)b * p.T + g];
        }
    }
    __threadfence_block();
    build_lists(p, sh);
}

// ---- joint.enc projection hoisted out of the symbol loop: out[m][n] = W[n].x[m] + b[n] -------------
// (src/nemo-ggml.cpp:1204-1205; the reference recomputes it per symbol).  f32 MFMA, packed weights,
// grid = (N/16, ceil(M/64)), 4 waves split K.
__global__ __launch_bounds__(256) void k_encproj(const float *x, const float *wpk, const float *bias, float *out, int M, int K, int N) {
    __shared__ float red[4][MT_MAX][64][4];
    const int nt = blockIdx.x, b0 = blockIdx.y * 16 * MT_MAX;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
    const int KG = K / 16;
    const float4 *w = (const float4 *)wpk + (size_t)nt * KG * 64 + lane;
    const int kg0 = wave * (KG / 4), kg1 = kg0 + KG / 4;
    const float *xr[MT_MAX];
#pragma unroll
    for (int mt = 0; mt < MT_MAX; mt++) {
        int m = b0 + mt * 16 + r;
        if (m >= M) m = M - 1;
        xr[mt] = x + (size_t)m * K;
    }
    f32x4 acc[MT_MAX];
#pragma unroll
    for (int mt = 0; mt < MT_MAX; mt++) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    mfma_range<MT_MAX, false>(w, kg0, kg1, xr, nullptr, q, acc);
#pragma unroll
    for (int mt = 0; mt < MT_MAX; mt++)
#pragma unroll
        for (int j = 0; j < 4; j++) red[wave][mt][lane][j] = acc[mt][j];
    __syncthreads();
    const int mt = wave, m = b0 + mt * 16 + r;
    if (m < M) {
        float4 o;
        float *op = (float *)&o;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int n = nt * 16 + q * 4 + j;
            op[j] = (((red[0][mt][lane][j] + red[1][mt][lane][j]) + red[2][mt][lane][j]) + red[3][mt][lane][j]) + bias[n];
        }
        *(float4 *)(out + (size_t)m * N + nt * 16 + q * 4) = o;
    }
}
void launch_encproj(const float *x, const float *wpk, const float *bias, float *out, int M, int K, int N, hipStream_t st) {
    hipLaunchKernelGGL(k_encproj, dim3(N / 16, (M + 16 * MT_MAX - 1) / (16 * MT_MAX)), dim3(256), 0, st, x, wpk, bias, out, M, K, N);
}

void launch_decode_begin(const DecParams &p, hipStream_t st) {
    hipLaunchKernelGGL(k_dec_begin, dim3(1), dim3(256), 0, st, p);
}
template <bool LP, bool BOOST, bool ALT, bool LMF = false, bool ENT = false>
static void launch_joint_commit(const DecParams &p, hipStream_t st) {
    static_assert(LP || !ALT, "the alternatives take their probabilities from the softmax parts");
    if constexpr (LP && !ENT) {
        if (p.ent_part) { launch_joint_commit<LP, BOOST, ALT, LMF, true>(p, st); return; }      // "token_entropy" (lp_part comes with it): the ENT forms of the same three kernels
    }
    const int rows = p.B * p.T;
    if (rows <= nasr_lp::SMALL_ROWS) hipLaunchKernelGGL((k_dec_joint<LP, BOOST, ALT, LMF, ENT>), dim3((VOCAB + 15) / 16), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((k_dec_joint_tiled<LP, BOOST, ALT, false, LMF, ENT>), dim3((VOCAB + 63) / 64, (rows + 63) / 64), dim3(256), 0, st, p);
    if constexpr (LP) {
        if (p.frame_blank) {                           // "frame_blank_logprobs": the commit variant that also fills the ring
            hipLaunchKernelGGL((k_dec_commit<LP, BOOST, ALT, true, LMF, ENT>), dim3(1), dim3(256), 0, st, p);
            return;
        }
    }
    hipLaunchKernelGGL((k_dec_commit<LP, BOOST, ALT, false, LMF, ENT>), dim3(1), dim3(256), 0, st, p);
}
void launch_lm_rows(const nasr_lm::Greedy *blk, const int32_t *lm_state, float *lm_row, int32_t *lm_next, const float *boost_bonus, const int *boost_state,
                    int slot0, int n, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_lm_rows_slots, dim3(lm_refresh_blocks(n)), dim3(256), 0, st, blk, lm_state, lm_row, lm_next, boost_bonus, boost_state, slot0, n);
}
void launch_decode_candidates(const DecParams &p, hipStream_t st) {
    hipLaunchKernelGGL(k_dec_lstm<0>, dim3(HID / 4), dim3(256), 0, st, p);
    hipLaunchKernelGGL(k_dec_lstm<1>, dim3(HID / 4), dim3(256), 0, st, p);
    hipLaunchKernelGGL(k_dec_pred<false>, dim3(JNT / 16), dim3(256), 0, st, p);
}
// beam search (kernels_beam.hip): the candidates of the rows in dlist, then the tiled joint with softmax parts and alternatives over rowmap --
// always this kernel, so the logits of a row do not depend on how many rows the sub-batch has
void launch_decode_rows(const DecParams &p, hipStream_t st) {
    launch_decode_candidates(p, st);
    hipLaunchKernelGGL((k_dec_joint_tiled<true, false, true>), dim3((VOCAB + 63) / 64, (p.B * p.T + 63) / 64), dim3(256), 0, st, p);
}
// the boosted beam evaluation: the same with the tiled joint in its BEAMB form (p.boost_bonus, p.boost_state = the beam's own per-slot array,
// p.raw_logits [B * T][1040])
void launch_decode_rows_boost(const DecParams &p, hipStream_t st) {
    launch_decode_candidates(p, st);
    hipLaunchKernelGGL((k_dec_joint_tiled<true, true, true, true>), dim3((VOCAB + 63) / 64, (p.B * p.T + 63) / 64), dim3(256), 0, st, p);
}
// One iteration = recompute stale prediction-network outputs, evaluate every remaining (stream, frame)
// row, commit.  Every kernel exits at once when its work list is empty, so surplus iterations of a
// blindly enqueued (graph-captured) sequence cost only their launch slots.
void launch_decode_iter(const DecParams &p, hipStream_t st) {
    hipLaunchKernelGGL(k_dec_lstm<0>, dim3(HID / 4), dim3(256), 0, st, p);
    hipLaunchKernelGGL(k_dec_lstm<1>, dim3(HID / 4), dim3(256), 0, st, p);
    // engine option "lm_fusion" (lm_row): the bias rows of the dirty streams are refreshed beside g -- by extra workgroups of the projection
    // (lm_fold, the form kept: profiles/greedy_lm.md) or by a launch of their own -- and the joint and the commit are the fused forms of the boosted ones
    if (p.lm_row) {
        if (p.lm_fold) hipLaunchKernelGGL(k_dec_pred<true>, dim3(JNT / 16 + lm_refresh_blocks(p.B)), dim3(256), 0, st, p);
        else {
            hipLaunchKernelGGL(k_dec_pred<false>, dim3(JNT / 16), dim3(256), 0, st, p);
            hipLaunchKernelGGL(k_dec_lmrows, dim3(lm_refresh_blocks(p.B)), dim3(256), 0, st, p);
        }
        if (p.alt_key) launch_joint_commit<true, true, true, true>(p, st);
        else if (p.lp_part) launch_joint_commit<true, true, false, true>(p, st);
        else launch_joint_commit<false, true, false, true>(p, st);
        return;
    }
    hipLaunchKernelGGL(k_dec_pred<false>, dim3(JNT / 16), dim3(256), 0, st, p);
    // engine options "token_logprobs" (lp_part) and "phrase_boost" (boost_bonus): the variants that also leave the softmax parts / the token's
    // log-probability, and that add the phrase bonus to the arg-max key; with both off these are the kernels without either.  "token_alternatives"
    // (alt_key; lp_part comes with it) takes the variants that also leave every slice's largest keys / the token's K best outputs.
    // "frame_blank_logprobs" (frame_blank; lp_part comes with it) takes the commit variant that also fills the ring (launch_joint_commit)
    if (p.alt_key) { if (p.boost_bonus) launch_joint_commit<true, true, true>(p, st); else launch_joint_commit<true, false, true>(p, st); }
    else if (p.lp_part) { if (p.boost_bonus) launch_joint_commit<true, true, false>(p, st); else launch_joint_commit<true, false, false>(p, st); }
    else { if (p.boost_bonus) launch_joint_commit<false, true, false>(p, st); else launch_joint_commit<false, false, false>(p, st); }
}
// iterations enqueued before the host looks at n_active (the arithmetic is host-tested with the rest of nasr_step_plan.h)
int decode_blind_iterations(int frames) { return nasr_step::blind_iterations(frames); }

}  // namespace nasr
