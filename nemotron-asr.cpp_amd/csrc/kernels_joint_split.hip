// kernels_joint_split.hip -- the RNN-T joint's output layer on the bf16 MFMA (engine option "joint_split"):
//   logits[row][v] = out_w[v] . relu(encproj[row] + predg[slot(row)]) + out_b[v],   640 -> 1025,
// as three v_mfma_f32_16x16x32_bf16 products of split operands,
//   x = hi + lo + r,  hi = RNE_bf16(x),  lo = RNE_bf16(x - hi)  (x - hi is exact in f32),      w . x ~= w_hi . x_hi + w_lo . x_hi + w_hi . x_lo
// (dropped: w_lo . x_lo and the two residues, each <= 2^-16 |w||x|).  k_dec_joint_split takes the place of k_dec_joint_tiled
// (kernels_decode.hip), whose 640 v_mfma_f32_16x16x4_f32 per wave bind it, wherever DecParams::out_planes is set: launch_joint_commit above
// nasr_lp::SMALL_ROWS rows and launch_decode_rows.  NOT covered: k_dec_joint (up to 64 rows a step: bound by the weight stream, not by the MFMA),
// the BEAMB form of the tiled kernel (launch_decode_rows_boost, raw_logits) and the alignment lattice's joint (kernels_align.hip) stay f32.
//
// WEIGHTS: k_joint_weight_planes splits the packed f32 out_w (65 vocab tiles of 16 rows, rows past 1025 are 0) once into bf16 hi / lo planes in the
// A-fragment order of the bf16 instruction: (tile nt, 32-deep k step ks) is one 2 KiB block, block nt * 20 + ks; lane (q, r) owns
// W[16 nt + r][32 ks + 8 q .. + 8) -- 16 bytes of hi at byte 16 lane, 16 bytes of lo at 1024 + 16 lane.  A wave's operand of a k step is two contiguous
// 1 KiB reads and no VALU.  65 x 20 x 2 KiB = 2 662 400 bytes.
//
// WORK SPLIT: k_dec_joint_tiled's, so the part and list layouts of nasr_logprob.h / nasr_topk.h hold unchanged: grid (17, ceil(rows / 64)), 256
// threads; wave w owns vocab tile 4 blockIdx.x + w and all four 16-row tiles; the workgroup's part index is blockIdx.x.
//
// K LOOP: ten chunks of 64.  x = relu(encproj + g) of the chunk is formed once per workgroup (thread -> row tid / 4, 16 consecutive k), split
// ONCE per element and stored as two bf16 images [64 rows][64 k] in LDS, double-buffered: 2 x 2 x 8 KiB.  A row is 128 B = eight 16-byte columns;
// column c of row `row` lies at column c ^ ((row >> 1) & 7).  The B fragment of lane (q, r) for m-tile mt and k step s of the chunk is
// X[16 mt + r][32 s + 8 q .. + 8) = column 4 s + q of that row: one ds_read_b128 per image.
//   BANKS: 16 lanes of one q read column 4 s + q of 16 consecutive rows; row & 1 picks the 128-byte half of the 256-byte bank line and
//   (row >> 1) & 7 runs through all eight values, so (4 s + q) ^ that does too: 16 lanes cover the 64 banks once.
// Weight fragments come straight from the planes in global memory; the next chunk's fragments and operand rows are loaded before this chunk's
// MFMAs.  Per k step and m-tile three MFMAs in fixed order into ONE f32 accumulator: w_hi x_hi, w_lo x_hi, w_hi x_lo; k ascends from a zero
// accumulator, no split of K: a logit's bits depend on its operand row and its weight row alone, never on the row count, the row's position
// or the other rows.  Rows past nr read row m0's data and are never stored; nmt skips whole empty m-tiles.
//
// EPILOGUE: the 16x16 f32 accumulator of the bf16 instruction has the layout of the f32 one -- lane (q, r) holds vocab rows 16 nt + 4 q .. + 3
// of frame row r -- so everything behind the K loop is k_dec_joint_tiled's epilogue, statement for statement on the accumulators
// (joint_tile_epilogue): arg-max key with the first-maximum rule and the atomicMax into key, BOOST / LMF bias, boost_raw, softmax parts, ALT
// lists in the staging buffer after the last barrier, the ENT pass through opaque copies.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN section 27.
#include "nasr_internal.h"

namespace nasr {

typedef __attribute__((ext_vector_type(4))) float js_f32x4_t;
typedef __attribute__((ext_vector_type(2))) float js_f32x2_t;
typedef __attribute__((ext_vector_type(8))) __bf16 js_bf16x8_t;
typedef __attribute__((ext_vector_type(2))) __bf16 js_bf16x2_t;

constexpr int JS_KC = 64;                       // K per LDS chunk = 2 k steps of the bf16 MFMA
constexpr int JS_NKC = JNT / JS_KC;             // 10
constexpr int JS_KS = JNT / 32;                 // 20 k steps
constexpr int JS_TILES = (VOCAB + 15) / 16;     // 65
constexpr int JS_IMG = 64 * JS_KC;              // bf16 per image: 8 KiB
static_assert(JNT % JS_KC == 0 && JS_KC == 64, "a row of an image is eight 16-byte columns");
static_assert((size_t)JS_TILES * JS_KS * 2048 == JOINT_PLANE_BYTES, "nasr_internal.h restates the planes' size");
static_assert(nasr_lp::LP_VOCAB == VOCAB && nasr_lp::WG_W == 64 && nasr_lp::WG_PARTS == (VOCAB + 63) / 64 && nasr_boost::VOCAB == VOCAB, "the tiled kernel's work split");

// (a, b) -> packed bf16 pairs hi = RNE(x), lo = RNE(x - hi)
static __device__ __forceinline__ void js_split2(float a, float b, uint32_t &hi, uint32_t &lo) {
    const js_f32x2_t x = {a, b};
    hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(x, js_bf16x2_t));          // v_cvt_pk_bf16_f32
    const js_f32x2_t r = {a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u)};
    lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, js_bf16x2_t));
}
static __device__ __forceinline__ void js_split8(const float4 &x0, const float4 &x1, uint4 &hi, uint4 &lo) {
    js_split2(x0.x, x0.y, hi.x, lo.x);
    js_split2(x0.z, x0.w, hi.y, lo.y);
    js_split2(x1.x, x1.y, hi.z, lo.z);
    js_split2(x1.z, x1.w, hi.w, lo.w);
}
static __device__ __forceinline__ js_f32x4_t js_mfma3(const uint4 &w_hi, const uint4 &w_lo, const uint4 &x_hi, const uint4 &x_lo, js_f32x4_t acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(js_bf16x8_t, w_hi), __builtin_bit_cast(js_bf16x8_t, x_hi), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(js_bf16x8_t, w_lo), __builtin_bit_cast(js_bf16x8_t, x_hi), acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(js_bf16x8_t, w_hi), __builtin_bit_cast(js_bf16x8_t, x_lo), acc, 0, 0, 0);
}

// ---- the planes: one thread per (tile nt, k step ks, lane) = 16 bytes of hi and 16 of lo; grid = 65 * 20 * 64 / 256 = 325 ---------------------
// The packed f32 matrix (nasr_eng::pack_f32_mfma) holds tile (nt, kg) = 16 rows x 16 k as 1 KiB, lane q' * 16 + r = W[16 nt + r][16 kg + 4 q' .. + 4):
// k = 32 ks + 8 q .. + 8 of row r are the float4 of lanes (2 (q & 1), r) and (2 (q & 1) + 1, r) of k-group 2 ks + (q >> 1)
__global__ __launch_bounds__(256) void k_joint_weight_planes(const float4 *__restrict__ w, uint4 *__restrict__ planes) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= JS_TILES * JS_KS * 64) return;
    const int lane = i & 63, blk = i >> 6, nt = blk / JS_KS, ks = blk - nt * JS_KS, q = lane >> 4, r = lane & 15;
    const float4 *src = w + ((size_t)(nt * (JNT / 16) + 2 * ks + (q >> 1)) * 64 + 2 * (q & 1) * 16 + r);
    uint4 hi, lo;
    js_split8(src[0], src[16], hi, lo);
    planes[(size_t)blk * 128 + lane] = hi;
    planes[(size_t)blk * 128 + 64 + lane] = lo;
}
void launch_joint_weight_planes(const float *out_w_packed, void *planes, hipStream_t st) {
    hipLaunchKernelGGL(k_joint_weight_planes, dim3((JS_TILES * JS_KS * 64 + 255) / 256), dim3(256), 0, st, (const float4 *)out_w_packed, (uint4 *)planes);
}

// ---- the one-line wrappers of kernels_decode.hip, restated ------------------------------------------------------------------------------------------
using nasr_lp::pack_key;
static __device__ __forceinline__ nasr_lp::Part lp_tile_part(float x0, float x1, float x2, float x3, int v0) { return nasr_lp::tile_part_wave(x0, x1, x2, x3, v0); }
static __device__ __forceinline__ float ent_opaque(float v) { asm volatile("" : "+v"(v)); return v; }
static __device__ __forceinline__ unsigned long long kmax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
static __device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
    const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
    return ((unsigned long long)hi << 32) | lo;
}
static __device__ __forceinline__ void alt_tile_keys(float x0, float x1, float x2, float x3, int v0, unsigned long long *a) {
    unsigned long long b[nasr_topk::KMAX];
    nasr_topk::lane_keys(x0, x1, x2, x3, v0, a);
#pragma unroll
    for (int j = 0; j < nasr_topk::KMAX; j++) b[j] = j < 4 ? shfl_xor_u64(a[j], 16) : 0ull;
    nasr_topk::merge8(a, b);
#pragma unroll
    for (int j = 0; j < nasr_topk::KMAX; j++) b[j] = shfl_xor_u64(a[j], 32);
    nasr_topk::merge8(a, b);
}

// what the epilogue passes between its waves: k_dec_joint_tiled's arrays
template <bool LP, bool BOOST, bool ENT>
struct JsEpilogueLds {
    unsigned long long bests[4][64];
    nasr_lp::Part lps[LP ? 4 : 1][64];            // token_logprobs: the four waves' tile parts of the 64 rows
    nasr_lp::Part elps[ENT ? 4 : 1][64];          // token_entropy: the four waves' tile parts once more, and their entropy terms
    float ents[ENT ? 4 : 1][64];
    float raws[LP && BOOST ? 4 : 1][64];          // ... with phrase_boost: the raw logit of each wave's winner by boosted key
};

// k_dec_joint_tiled's epilogue (its forms without BEAMB) on the accumulators acc[mt][j] = logit of vocab entry 16 nt + 4 q + j, frame row
// m0 + 16 mt + r, bias not yet added.  Every thread of the workgroup calls it behind the K loop's last barrier; alts is the operand staging
// buffer, which nobody reads from there on
template <bool LP, bool BOOST, bool ALT, bool LMF, bool ENT>
static __device__ __forceinline__ void joint_tile_epilogue(const DecParams &p, const js_f32x4_t (&acc)[4], int nr, int m0, int nmt, const int (&bstate)[4],
                                                           JsEpilogueLds<LP, BOOST, ENT> &s, unsigned long long (*alts)[nasr_topk::KMAX][64]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
    const int nt = blockIdx.x * 4 + wave;
    const bool has_tile = nt * 16 < VOCAB;
    // arg-max: in-lane over the 4 vocab entries, across the 4 lane groups, across the 4 waves, then one atomic per row
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
        if (q == 0) s.bests[wave][mt * 16 + r] = best;
        if (LP && BOOST) {                             // the lane that holds the wave's winner leaves its raw logit
            const int wv = nasr_lp::key_index_of(best) - (nt * 16 + q * 4);
            if (best && wv >= 0 && wv < 4) {
                const float a = wv == 0 ? acc[mt][0] : wv == 1 ? acc[mt][1] : wv == 2 ? acc[mt][2] : acc[mt][3];
                s.raws[wave][mt * 16 + r] = a + p.out_b[nt * 16 + q * 4 + wv];
            }
        }
        if (LP) {
            const int v0 = has_tile ? nt * 16 + q * 4 : VOCAB;          // no tile: the empty part
            float lg[4];
#pragma unroll
            for (int j = 0; j < 4; j++) lg[j] = acc[mt][j] + p.out_b[v0 + j < VOCAB ? v0 + j : 0];
            const nasr_lp::Part part = lp_tile_part(lg[0], lg[1], lg[2], lg[3], v0);
            if (q == 0) s.lps[wave][mt * 16 + r] = part;
            if (ALT) {                                 // no tile: v0 = VOCAB leaves the empty list
                unsigned long long top[nasr_topk::KMAX];
                alt_tile_keys(lg[0], lg[1], lg[2], lg[3], v0, top);
                if (q == 0) {
#pragma unroll
                    for (int j = 0; j < nasr_topk::KMAX; j++) alts[wave][j][mt * 16 + r] = top[j];
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 64 && m0 + threadIdx.x < nr) {
        const unsigned long long best = kmax(kmax(s.bests[0][threadIdx.x], s.bests[1][threadIdx.x]), kmax(s.bests[2][threadIdx.x], s.bests[3][threadIdx.x]));
        const unsigned rm = p.rowmap[m0 + threadIdx.x];
        if (best) atomicMax(&p.key[(size_t)(rm & 0xffffu) * p.T + (rm >> 16)], best);
        if (LP && BOOST) {                             // the workgroup's winner is the winner of its wave: part blockIdx.x of the row
            int w = 0;
            unsigned long long kw = s.bests[0][threadIdx.x];
#pragma unroll
            for (int u = 1; u < 4; u++) if (s.bests[u][threadIdx.x] > kw) { kw = s.bests[u][threadIdx.x]; w = u; }
            if (kw) p.boost_raw[nasr_lp::scratch_index(nasr_lp::key_index(rm, p.T), blockIdx.x, nasr_lp::WG_PARTS)] = s.raws[w][threadIdx.x];
        }
    }
    if (LP) {                                      // one part per workgroup (64 entries): part blockIdx.x of the row, waves merged in order
        const int row = nasr_lp::tiled_store_row(blockIdx.y, threadIdx.x, nr);
        if (row >= 0) {
            const nasr_lp::Part part = nasr_lp::wg64(s.lps[0][threadIdx.x], s.lps[1][threadIdx.x], s.lps[2][threadIdx.x], s.lps[3][threadIdx.x]);
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
                if (q == 0) { s.elps[wave][mt * 16 + r] = ep.p; s.ents[wave][mt * 16 + r] = ep.e; }
            }
            __syncthreads();
            const int row = nasr_lp::tiled_store_row(blockIdx.y, threadIdx.x, nr);
            if (row >= 0) {
                const int t = threadIdx.x;
                const nasr_ent::EPart ep = nasr_ent::wg64({s.elps[0][t], s.ents[0][t]}, {s.elps[1][t], s.ents[1][t]}, {s.elps[2][t], s.ents[2][t]}, {s.elps[3][t], s.ents[3][t]}, p.ent_alpha);
                p.ent_part[nasr_lp::scratch_index(nasr_lp::key_index(p.rowmap[row], p.T), blockIdx.x, nasr_lp::WG_PARTS)] = ep.e;
            }
        }
    }
}

template <bool LP, bool BOOST, bool ALT, bool LMF, bool ENT>
__global__ __launch_bounds__(256) void k_dec_joint_split(DecParams p) {
    static_assert(!ENT || LP, "the entropy terms ride on the softmax parts");
    static_assert(!ALT || LP, "the alternatives take their probabilities from the softmax parts");
    static_assert(!LMF || BOOST, "the fused form is a form of the boosted kernel");
    const int nr = *p.n_rows;
    const int m0 = blockIdx.y * 64;
    if (m0 >= nr) return;
    __shared__ __attribute__((aligned(16))) bf16_t xs[2][2][JS_IMG];       // [buffer][hi, lo][64 rows][64 k], 16-byte columns swizzled
    __shared__ JsEpilogueLds<LP, BOOST, ENT> epi;
    // token_alternatives: the four waves' tile lists of the 64 rows, [wave][entry][row], take the place of the operand staging
    static_assert(sizeof(unsigned long long) * 4 * nasr_topk::KMAX * 64 <= sizeof(xs), "the lists fit the staging buffer");
    unsigned long long (*alts)[nasr_topk::KMAX][64] = (unsigned long long (*)[nasr_topk::KMAX][64])&xs[0][0][0];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
    const int nt = blockIdx.x * 4 + wave;
    const bool has_tile = nt * 16 < VOCAB;
    const uint4 *w = (const uint4 *)p.out_planes + (size_t)(has_tile ? nt : 0) * JS_KS * 128 + lane;
    int nmt = (nr - m0 + 15) >> 4;
    if (nmt > 4) nmt = 4;
    // staging role: thread -> (row, 16 consecutive k = two 16-byte bf16 columns per image)
    const int srow = threadIdx.x >> 2, sc0 = (threadIdx.x & 3) * 2, ssw = (srow >> 1) & 7;
    const unsigned srm = p.rowmap[m0 + srow < nr ? m0 + srow : m0];
    const float *erow = p.encproj + ((size_t)(srm & 0xffffu) * p.T + (srm >> 16)) * JNT + sc0 * 8;
    const float *grow = p.predg + (size_t)p.rows[srm & 0xffffu].slot * JNT + sc0 * 8;
    float4 ev[4], gv[4];
    uint4 wv[2][2], wn[2][2];                       // [k step of the chunk][hi, lo]
    auto gload = [&](int kc) {
#pragma unroll
        for (int i = 0; i < 4; i++) { ev[i] = *(const float4 *)(erow + kc * JS_KC + i * 4); gv[i] = *(const float4 *)(grow + kc * JS_KC + i * 4); }
    };
    auto wload = [&](int kc, uint4 (&dst)[2][2]) {
#pragma unroll
        for (int s = 0; s < 2; s++) { dst[s][0] = w[(size_t)(kc * 2 + s) * 128]; dst[s][1] = w[(size_t)(kc * 2 + s) * 128 + 64]; }
    };
    auto sstore = [&](int buf) {
        float4 x[4];
#pragma unroll
        for (int i = 0; i < 4; i++)
            x[i] = make_float4(fmaxf(ev[i].x + gv[i].x, 0.0f), fmaxf(ev[i].y + gv[i].y, 0.0f), fmaxf(ev[i].z + gv[i].z, 0.0f), fmaxf(ev[i].w + gv[i].w, 0.0f));
#pragma unroll
        for (int h = 0; h < 2; h++) {
            uint4 hi, lo;
            js_split8(x[2 * h], x[2 * h + 1], hi, lo);
            const int at = srow * JS_KC + (((sc0 + h) ^ ssw) << 3);
            *(uint4 *)(&xs[buf][0][at]) = hi;
            *(uint4 *)(&xs[buf][1][at]) = lo;
        }
    };
    int bstate[4] = {0, 0, 0, 0};                   // phrase_boost: automaton state (LMF: slot) of this lane's row of every m-tile
    if (BOOST) {
#pragma unroll
        for (int mt = 0; mt < 4; mt++) {
            const int row = m0 + mt * 16 + r;
            const int slot = p.rows[p.rowmap[row < nr ? row : m0] & 0xffffu].slot;
            bstate[mt] = LMF ? slot : p.boost_state[slot];
        }
    }
    js_f32x4_t acc[4];
#pragma unroll
    for (int mt = 0; mt < 4; mt++) acc[mt] = (js_f32x4_t){0.f, 0.f, 0.f, 0.f};
    gload(0);
    wload(0, wv);
    sstore(0);
    __syncthreads();
    for (int kc = 0; kc < JS_NKC; kc++) {
        const int cur = kc & 1;
        if (kc + 1 < JS_NKC) { gload(kc + 1); wload(kc + 1, wn); }
#pragma unroll
        for (int s = 0; s < 2; s++) {
#pragma unroll
            for (int mt = 0; mt < 4; mt++) {
                if (mt < nmt) {
                    const int at = (mt * 16 + r) * JS_KC + (((s * 4 + q) ^ (r >> 1)) << 3);      // (row >> 1) & 7 of row 16 mt + r is r >> 1
                    const uint4 x_hi = *(const uint4 *)(&xs[cur][0][at]), x_lo = *(const uint4 *)(&xs[cur][1][at]);
                    acc[mt] = js_mfma3(wv[s][0], wv[s][1], x_hi, x_lo, acc[mt]);
                }
            }
        }
        if (kc + 1 < JS_NKC) {
            sstore(cur ^ 1);
#pragma unroll
            for (int s = 0; s < 2; s++) { wv[s][0] = wn[s][0]; wv[s][1] = wn[s][1]; }
        }
        __syncthreads();
    }
    joint_tile_epilogue<LP, BOOST, ALT, LMF, ENT>(p, acc, nr, m0, nmt, bstate, epi, alts);
}

template <bool LP, bool BOOST, bool ALT, bool LMF, bool ENT>
void launch_joint_split(const DecParams &p, hipStream_t st) {
    hipLaunchKernelGGL((k_dec_joint_split<LP, BOOST, ALT, LMF, ENT>), dim3((VOCAB + 63) / 64, (p.B * p.T + 63) / 64), dim3(256), 0, st, p);
}
// every form launch_joint_commit and launch_decode_rows (kernels_decode.hip) can take: <LP, BOOST, ALT, LMF>, and with LP its ENT twin
#define NASR_JOINT_SPLIT_FORM(LP, BOOST, ALT, LMF, ENT) template void launch_joint_split<LP, BOOST, ALT, LMF, ENT>(const DecParams &, hipStream_t);
NASR_JOINT_SPLIT_FORM(false, false, false, false, false)
NASR_JOINT_SPLIT_FORM(false, true, false, false, false)
NASR_JOINT_SPLIT_FORM(false, true, false, true, false)
#define NASR_JOINT_SPLIT_LP(BOOST, ALT, LMF) NASR_JOINT_SPLIT_FORM(true, BOOST, ALT, LMF, false) NASR_JOINT_SPLIT_FORM(true, BOOST, ALT, LMF, true)
NASR_JOINT_SPLIT_LP(false, false, false)
NASR_JOINT_SPLIT_LP(false, true, false)
NASR_JOINT_SPLIT_LP(true, false, false)
NASR_JOINT_SPLIT_LP(true, true, false)
NASR_JOINT_SPLIT_LP(true, false, true)
NASR_JOINT_SPLIT_LP(true, true, true)
#undef NASR_JOINT_SPLIT_LP
#undef NASR_JOINT_SPLIT_FORM

}  // namespace nasr
