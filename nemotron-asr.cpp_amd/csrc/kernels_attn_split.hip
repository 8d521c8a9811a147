// kernels_attn_split.hip -- the f32 engine's attention on the bf16 MFMA: k_off_attn_f32_split, the offline path's full-context relative-position
// attention (engine option "f32_split_attn", DESIGN section 24, described first), and k_attention_f32_split, the streaming cached attention (engine
// option "f32_split_attn_stream", DESIGN section 25, described above the kernel).  Both: f32 operands in HBM, f32 softmax, f32 context, and every matrix product as three
// v_mfma_f32_16x16x32_bf16 of split operands,
//   x = hi + lo + r,  hi = RNE_bf16(x),  lo = RNE_bf16(x - hi)  (x - hi is exact in f32),      a . b ~= a_hi . b_hi + a_hi . b_lo + a_lo . b_hi
// (dropped: a_lo . b_lo and the two residues, each <= 2^-16 |a||b|).  The operation, OffAttnParams and the work items
// (off, T, q0, 0) are k_off_attn_f32's (kernels_offline.hip); the geometry is k_off_attn_bf16's.
//
// One workgroup per (utterance, 64-query block) x head; wave w owns the 16 queries i0 = q0 + 16 w .. + 16 and keeps (q + u) and (q + v),
// split once at kernel entry, in registers.  The keys are walked in blocks of 64 with an online softmax.  What the four waves of a
// workgroup share in a key block -- the 64 K rows, the 127-row position band, the 64 V rows -- is split ONCE per workgroup into a bf16
// hi / lo image in LDS, and the waves read MFMA fragments from the image.  The images take turns in one 36 KiB region (four phases per key
// block), because all of them together (K 34 KiB + band 68 KiB + V^T 36 KiB) would leave one workgroup per CU:
//   phase K    rows j0 .. j0 + 63 of K               content  S^T[j][i] = K[j] . (q_i + u)           4 tiles of 16 keys per wave
//   phase P0/1 band rows 64 hf .. + 64                position P[b][i]   = Pos[rb + b] . (q_i + v)    band row b = (j - j0) - (i - q0) + 63 in [0, 127),
//              table row rb + b = j - i + 2047 (rb = j0 - q0 + 1984).  Wave w needs band rows 48 - 16 w .. + 80: the five 16-row tiles
//              3 - w .. 7 - w of the workgroup's eight, each computed in the half that holds it, and skewed through the wave's own LDS strip
//              exactly as in k_off_attn_bf16 (column (j - j0) - (i - i0) + 15 of query row i - i0)
//   phase V    V^T[d][k] of keys j0 .. j0 + 63 (zeros past T)   O^T[d][i] += V^T[d][k] . p^T[k][i]     the f32 exponentials split in registers
// The global loads of a phase are issued before the MFMAs of the phase in front of it (32 registers of f32 in flight), the split and the
// image stores sit between two barriers.  (S + P) / sqrt(128), keys j >= T masked to -inf, rows i >= T never written.  Row indices are
// clamped into the utterance (keys, queries) and into the table (band row 127, which no score reads, can lie past row 4094).
// ORDER per accumulator and k step: b_hi a_hi, b_lo a_hi, b_hi a_lo (a = the query-side operand); k steps and key blocks ascending: the
// bits of a context row depend on its own utterance alone (batch == alone).
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN section 24.
#include "nasr_internal.h"
#include "nasr_offline.h"
#include "nasr_wave.h"

namespace nasr {

constexpr int AS_BN = 64;                // keys per block of the online softmax
constexpr int AS_KP = DH + 8;            // bf16 per row of a row image (K, band half): rows 4 banks apart, a 16-lane ds_read_b128 covers 64 banks once
constexpr int AS_VP = AS_BN + 8;         // bf16 per row of the V^T image (k_off_attn_bf16's pitch)
constexpr int AS_HALF = DH * AS_VP;      // bf16 between the hi and the lo image: the larger of 64 x 136 and 128 x 72
constexpr int AS_SP = 84;                // floats per query row of a wave's band scores (80 + 4)
constexpr int AS_LDS = 2 * AS_HALF * 2 + 4 * 16 * AS_SP * 4;          // 36 864 + 21 504 = 58 368 B
static_assert(AS_HALF >= AS_BN * AS_KP, "the image region holds a row image");
static_assert(2 * AS_LDS <= 160 * 1024, "two workgroups per CU");
static_assert(OFF_QB_SPLIT == 64 && DH == 128 && OFFLINE_MAX_T % OFF_QB_SPLIT == 0, "the band arithmetic below");

typedef __attribute__((ext_vector_type(8))) __bf16 as_bf16x8_t;
typedef __attribute__((ext_vector_type(2))) __bf16 as_bf16x2_t;
typedef __attribute__((ext_vector_type(2))) float as_f32x2_t;
typedef __attribute__((ext_vector_type(4))) float as_f32x4_t;

// (a, b) -> packed bf16 pairs hi = RNE(x), lo = RNE(x - hi)
__device__ __forceinline__ void as_split2(float a, float b, uint32_t &hi, uint32_t &lo) {
    const as_f32x2_t x = {a, b};
    hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(x, as_bf16x2_t));          // v_cvt_pk_bf16_f32
    const as_f32x2_t r = {a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u)};
    lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, as_bf16x2_t));
}
// 8 consecutive dims of q + bias -> one MFMA fragment each of hi and lo
__device__ __forceinline__ void as_q_plus(const float4 &x0, const float4 &x1, const float *bias, uint4 &hi, uint4 &lo) {
    const float4 b0 = *(const float4 *)bias, b1 = *(const float4 *)(bias + 4);
    as_split2(x0.x + b0.x, x0.y + b0.y, hi.x, lo.x);
    as_split2(x0.z + b0.z, x0.w + b0.w, hi.y, lo.y);
    as_split2(x1.x + b1.x, x1.y + b1.y, hi.z, lo.z);
    as_split2(x1.z + b1.z, x1.w + b1.w, hi.w, lo.w);
}
__device__ __forceinline__ as_f32x4_t as_mfma3(const uint4 &a_hi, const uint4 &a_lo, const uint4 &b_hi, const uint4 &b_lo, as_f32x4_t acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(as_bf16x8_t, a_hi), __builtin_bit_cast(as_bf16x8_t, b_hi), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(as_bf16x8_t, a_lo), __builtin_bit_cast(as_bf16x8_t, b_hi), acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(as_bf16x8_t, a_hi), __builtin_bit_cast(as_bf16x8_t, b_lo), acc, 0, 0, 0);
}

// 64 rows x 128 f32 (rows row0 .. row0 + 63 of a matrix of leading dimension ld, clamped to [0, last]) -> 8 float4 per thread: a wave
// instruction reads two whole 512-byte rows
__device__ __forceinline__ void as_load_rows(const float *base, int ld, int row0, int last, float4 (&raw)[8]) {
    const int rr = threadIdx.x >> 5, c4 = (threadIdx.x & 31) * 4;
#pragma unroll
    for (int u = 0; u < 8; u++) {
        int row = row0 + 8 * u + rr;
        row = row < 0 ? 0 : (row > last ? last : row);
        raw[u] = *(const float4 *)(base + (size_t)row * ld + c4);
    }
}
// ... split, into the row image [64][AS_KP] (hi at img, lo at img + AS_HALF)
__device__ __forceinline__ void as_store_rows(bf16_t *img, const float4 (&raw)[8]) {
    const int rr = threadIdx.x >> 5, c4 = (threadIdx.x & 31) * 4;
#pragma unroll
    for (int u = 0; u < 8; u++) {
        uint2 hi, lo;
        as_split2(raw[u].x, raw[u].y, hi.x, lo.x);
        as_split2(raw[u].z, raw[u].w, hi.y, lo.y);
        bf16_t *dst = img + (8 * u + rr) * AS_KP + c4;
        *(uint2 *)dst = hi;
        *(uint2 *)(dst + AS_HALF) = lo;
    }
}
// V of keys j0 + 2 jj, + 1 (jj = thread & 31), dims 16 dg .. + 16 (dg = thread >> 5); zeros past T: a weight of 0 never meets a stale value
__device__ __forceinline__ void as_load_v(const float *Vb, int j0, int T, float4 (&raw)[8]) {
    const int j = j0 + 2 * (threadIdx.x & 31), d0 = 16 * (threadIdx.x >> 5);
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
        for (int c = 0; c < 4; c++)
            raw[4 * k + c] = j + k < T ? *(const float4 *)(Vb + (size_t)(j + k) * OFF_QKV_LD + d0 + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// ... split, transposed into the V^T image [128][AS_VP]: one 4-byte store per dimension and half (the key pair)
__device__ __forceinline__ void as_store_vt(bf16_t *img, const float4 (&raw)[8]) {
    const int jj2 = 2 * (threadIdx.x & 31), d0 = 16 * (threadIdx.x >> 5);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float a[4] = {raw[c].x, raw[c].y, raw[c].z, raw[c].w}, b[4] = {raw[4 + c].x, raw[4 + c].y, raw[4 + c].z, raw[4 + c].w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            uint32_t hi, lo;
            as_split2(a[e], b[e], hi, lo);
            bf16_t *dst = img + (d0 + 4 * c + e) * AS_VP + jj2;
            *(uint32_t *)dst = hi;
            *(uint32_t *)(dst + AS_HALF) = lo;
        }
    }
}

__global__ __launch_bounds__(256) void k_off_attn_f32_split(OffAttnParams p) {
    __shared__ __attribute__((aligned(16))) bf16_t img[2 * AS_HALF];
    __shared__ __attribute__((aligned(16))) float sp[4][16 * AS_SP];
    const int4 it = p.items[blockIdx.x];
    const int h = blockIdx.y, off = it.x, T = it.y, q0 = it.z;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
    const int i0 = q0 + 16 * wave;
    const float *Qb = (const float *)p.qkv + (size_t)off * OFF_QKV_LD + h * DH;
    const float *Kb = Qb + D, *Vb = Qb + 2 * D;
    const float *Pb = (const float *)p.pos + h * DH;
    int iq = i0 + r;
    if (iq > T - 1) iq = T - 1;                                   // rows past the utterance: valid memory of its own, never written
    uint4 qu_hi[4], qu_lo[4], qv_hi[4], qv_lo[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        const float *src = Qb + (size_t)iq * OFF_QKV_LD + ks * 32 + q * 8;
        const float4 x0 = *(const float4 *)src, x1 = *(const float4 *)(src + 4);
        as_q_plus(x0, x1, p.bias_u + h * DH + ks * 32 + q * 8, qu_hi[ks], qu_lo[ks]);
        as_q_plus(x0, x1, p.bias_v + h * DH + ks * 32 + q * 8, qv_hi[ks], qv_lo[ks]);
    }
    const float scale = 0.08838834764831845f;                    // 1/sqrt(128), applied to the sum as in the reference
    float m_run = -INFINITY, l_run = 0.0f;
    as_f32x4_t o[8];
#pragma unroll
    for (int dt = 0; dt < 8; dt++) o[dt] = (as_f32x4_t){0.f, 0.f, 0.f, 0.f};
    // the fragment of image row (16 tile + r), k chunk ks: 8 consecutive dims
    const bf16_t *frag = img + r * AS_KP + q * 8;
    float4 raw[8];
    as_load_rows(Kb, OFF_QKV_LD, 0, T - 1, raw);
    for (int j0 = 0; j0 < T; j0 += AS_BN) {
        const int rb = j0 - q0 + (OFFLINE_MAX_T - OFF_QB_SPLIT);  // table row of band row 0: j0 - (q0 + 63) + 2047, >= 0 as q0 <= 1984
        // ---- phase K ------------------------------------------------------------------------------------------------------------
        __syncthreads();                                          // the previous block's V^T reads are done
        as_store_rows(img, raw);
        __syncthreads();
        as_load_rows(Pb, D, rb, OFFLINE_NREL - 1, raw);
        as_f32x4_t s[4];
#pragma unroll
        for (int kt = 0; kt < 4; kt++) {
            as_f32x4_t acc = (as_f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                const bf16_t *a = frag + 16 * kt * AS_KP + ks * 32;
                acc = as_mfma3(*(const uint4 *)a, *(const uint4 *)(a + AS_HALF), qu_hi[ks], qu_lo[ks], acc);
            }
            s[kt] = acc;
        }
        // ---- phases P0, P1: band tile t = pt + 3 - wave lies in half t >> 2 ------------------------------------------------------------
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {
            __syncthreads();
            as_store_rows(img, raw);
            __syncthreads();
            if (hf == 0) as_load_rows(Pb, D, rb + 64, OFFLINE_NREL - 1, raw);
            else as_load_v(Vb, j0, T, raw);
#pragma unroll
            for (int pt = 0; pt < 5; pt++) {
                const int t = pt + 3 - wave;
                if ((t >> 2) != hf) continue;                     // wave-uniform
                as_f32x4_t acc = (as_f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 4; ks++) {
                    const bf16_t *a = frag + 16 * (t & 3) * AS_KP + ks * 32;
                    acc = as_mfma3(*(const uint4 *)a, *(const uint4 *)(a + AS_HALF), qv_hi[ks], qv_lo[ks], acc);
                }
                *(float4 *)&sp[wave][r * AS_SP + 16 * pt + 4 * q] = make_float4(acc[0], acc[1], acc[2], acc[3]);
            }
        }
        // ---- phase V ------------------------------------------------------------------------------------------------------------
        __syncthreads();
        as_store_vt(img, raw);
        __syncthreads();                                          // ... and the wave's band scores are visible to its lanes
        if (j0 + AS_BN < T) as_load_rows(Kb, OFF_QKV_LD, j0 + AS_BN, T - 1, raw);
        // scores of query r, keys j0 + 16 kt + 4 q + e; the four lanes r, r + 16, r + 32, r + 48 hold the 64 keys of one query
        float sv[4][4], mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; kt++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int jl = 16 * kt + 4 * q + e;
                float v = (s[kt][e] + sp[wave][r * AS_SP + jl - r + 15]) * scale;
                if (j0 + jl >= T) v = -INFINITY;
                sv[kt][e] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);                     // finite: key j0 < T is in every block
        const float alpha = __expf(m_run - m_new);
        float ps = 0.0f;
#pragma unroll
        for (int kt = 0; kt < 4; kt++)
#pragma unroll
            for (int e = 0; e < 4; e++) { sv[kt][e] = __expf(sv[kt][e] - m_new); ps += sv[kt][e]; }
        ps += __shfl_xor(ps, 16);
        ps += __shfl_xor(ps, 32);
        l_run = l_run * alpha + ps;
        m_run = m_new;
#pragma unroll
        for (int dt = 0; dt < 8; dt++) { o[dt][0] *= alpha; o[dt][1] *= alpha; o[dt][2] *= alpha; o[dt][3] *= alpha; }
        // the k order of the P.V MFMA is k_off_attn_bf16's permutation: lane group q holds keys 4 q .. 4 q + 3 of two 16-key tiles
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            uint4 b_hi, b_lo;
            as_split2(sv[2 * ks][0], sv[2 * ks][1], b_hi.x, b_lo.x);
            as_split2(sv[2 * ks][2], sv[2 * ks][3], b_hi.y, b_lo.y);
            as_split2(sv[2 * ks + 1][0], sv[2 * ks + 1][1], b_hi.z, b_lo.z);
            as_split2(sv[2 * ks + 1][2], sv[2 * ks + 1][3], b_hi.w, b_lo.w);
#pragma unroll
            for (int dt = 0; dt < 8; dt++) {
                const bf16_t *row = img + (16 * dt + r) * AS_VP + 32 * ks + 4 * q;
                const uint2 h0 = *(const uint2 *)row, h1 = *(const uint2 *)(row + 16);
                const uint2 l0 = *(const uint2 *)(row + AS_HALF), l1 = *(const uint2 *)(row + AS_HALF + 16);
                o[dt] = as_mfma3(make_uint4(h0.x, h0.y, h1.x, h1.y), make_uint4(l0.x, l0.y, l1.x, l1.y), b_hi, b_lo, o[dt]);
            }
        }
    }
    if (i0 + r < T) {
        const float inv = 1.0f / l_run;
        float *dst = (float *)p.ctx + (size_t)(off + i0 + r) * D + h * DH + 4 * q;
#pragma unroll
        for (int dt = 0; dt < 8; dt++) *(float4 *)(dst + 16 * dt) = make_float4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
    }
}

void launch_off_attention_split(const OffAttnParams &p, int n_items, hipStream_t st) {
    if (n_items > 0) hipLaunchKernelGGL(k_off_attn_f32_split, dim3(n_items, NH), dim3(256), 0, st, p);
}

// ---- streaming: the cached relative-position attention of an f32 engine on the bf16 MFMA (engine option "f32_split_attn_stream") ----
// The operation and AttnParams are k_attention<false>'s (kernels_layer.hip), the work split is k_attention_mfma's: one workgroup of 4 waves per
// (head, stream, group of query rows); a group is one chunk for T >= 4 and 16 rows = 16 / T chunks for T <= 2; its keys are the SPAN of
// 70 + (chunks in the group) T <= 86 ring rows; row (chunk g, frame i) attends the window of 70 + T keys that starts (g - g0) T rows into the span,
// with the cache validity min(valid_len + g T, 70); every weight outside the window is exactly 0.  Every operand stays f32 in memory and every
// product is as_mfma3 of split operands, k steps ascending from a zero accumulator:
//   scores^T  S[j][i] = K[j] . (q_i + u), P[r][i] = Pos[r] . (q_i + v)      6 key tiles + 7 position tiles of 16 rows, dealt over the waves (tile t
//             goes to wave t & 3; tiles that start past the span / the table are skipped).  A K or position row is the A operand of exactly one
//             wave: its lanes load it from global memory straight into the operand layout (two float4 per lane and k step) and split it in
//             registers.  (q + u) and (q + v) of the group's rows are split once into four swizzled bf16 images (k_attention_mfma's swizzle).
//   softmax   f32, one wave per row, two span positions per lane; the rel-shift is the LDS gather sp[i][j + T - 1 - ic]; the f32 weights are split
//             into a hi and a lo image that take the place of the (q + u) images
//   context^T O[d][i] = sum_j V^T[d][j] w[i][j]     8 d tiles x 3 k steps x 3 products, wave w owns d = 32 w .. + 32.  V^T[d][8 keys] is exactly the
//             A operand of one lane of one wave, so V does not pass through LDS: every lane loads its 48 V elements itself (16 lanes = 64 contiguous
//             bytes of a ring row, a wave instruction = 4 ring rows), up front with everything else, and splits them after the softmax.  No V^T image,
//             no fourth barrier, 29.5 KiB of LDS instead of 60.
// Every global load is requested before the first wait: one round trip per workgroup.  Rows past nrows use zero queries, get zero weights and
// are never written; K rows are clamped into the span and position rows into the table, V past the span is 0.
// BITS: a context row depends on its own stream and on the step's chunking (T, TS) only -- batch == alone.  At T <= 2 the k steps of P.V start at
// the span, not at the row's window: a row's bits can depend on which chunks share its workgroup (as in k_attention_mfma, not in k_attention<false>).
constexpr int SS_SKP = 100, SS_SPP = 116;                 // row pitches (floats) of the score tiles: 96 / 112 + 4 (k_attention_mfma's)
constexpr int SS_IMG = 16 * 256;                          // one bf16 image [16 rows][128]: 256 B per row, 16-byte chunk c of row i at chunk (c ^ i) & 15
constexpr int SS_LDS = 4 * SS_IMG + 16 * (SS_SKP + SS_SPP) * 4;       // 16 384 + 13 824 = 30 208 B

__device__ __forceinline__ void ss_split8(const float4 &x0, const float4 &x1, uint4 &hi, uint4 &lo) {
    as_split2(x0.x, x0.y, hi.x, lo.x);
    as_split2(x0.z, x0.w, hi.y, lo.y);
    as_split2(x1.x, x1.y, hi.z, lo.z);
    as_split2(x1.z, x1.w, hi.w, lo.w);
}

__global__ __launch_bounds__(256) void k_attention_f32_split(AttnParams p) {
    __shared__ __attribute__((aligned(16))) char lds[SS_LDS];
    char *const qu_s = lds, *const qv_s = lds + 2 * SS_IMG;          // hi image, lo image SS_IMG behind it              phases 0-1
    char *const w_s = lds;                                           // softmax weights, hi and lo                        phases 2-3
    float *const sk = (float *)(lds + 4 * SS_IMG), *const sp = sk + 16 * SS_SKP;      // score tiles                       phases 1-2
    const int h = blockIdx.x, b = blockIdx.y, T = p.T, KV = LCTX + T, n_rel = KV + T - 1;
    const int TS = p.TS > 0 ? p.TS : p.T;
    const int QB = T <= 2 ? 16 : T;                          // query rows per workgroup
    const int r0 = blockIdx.z * QB, nrows = TS - r0 < QB ? TS - r0 : QB;
    const int g0 = r0 / T;                                   // first chunk of the group
    const int span = LCTX + ((nrows + T - 1) / T) * T;       // ring rows the group can see (<= 86 < 96)
    const RowDesc rd = p.rows[b];
    const size_t row0 = (size_t)b * TS + (size_t)r0;
    int head0 = rd.kv_head + g0 * T;
    while (head0 >= KVC) head0 -= KVC;
    const float *kbase = (const float *)p.kv_pool + (size_t)rd.slot * p.kv_slot_stride + h * DH;
    const float *vbase = kbase + (size_t)KVC * D;
    const float *pbase = (const float *)p.posproj + h * DH;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
    // ---- every global read of the workgroup, in the order of use: queries and biases, this wave's K / position tiles, this lane's V elements ----
    float4 qreg[2], ureg[2], breg[2];
#pragma unroll
    for (int it = 0; it < 2; it++) {
        const int e = threadIdx.x + it * 256, i = e >> 5, c4 = (e & 31) * 4;
        qreg[it] = i < nrows ? *(const float4 *)(p.q + (row0 + i) * D + h * DH + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        ureg[it] = *(const float4 *)(p.bias_u + h * DH + c4);
        breg[it] = *(const float4 *)(p.bias_v + h * DH + c4);
    }
    float4 av[4][8];                                       // tiles wave, wave + 4, wave + 8, wave + 12 of the 6 key + 7 position tiles
    bool live[4];
#pragma unroll
    for (int n = 0; n < 4; n++) {
        const int t = wave + 4 * n;
        live[n] = t < 13 && (t < 6 ? t * 16 < span : (t - 6) * 16 < n_rel);      // wave-uniform
        if (live[n]) {
            const float *arow;
            if (t < 6) {
                int j = t * 16 + r;
                if (j >= span) j = span - 1;
                int ring = head0 + j;
                if (ring >= KVC) ring -= KVC;
                arow = kbase + (size_t)ring * D;
            } else {
                int rr = (t - 6) * 16 + r;
                if (rr >= n_rel) rr = n_rel - 1;
                arow = pbase + (size_t)rr * D;
            }
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                av[n][2 * ks] = *(const float4 *)(arow + ks * 32 + q * 8);
                av[n][2 * ks + 1] = *(const float4 *)(arow + ks * 32 + q * 8 + 4);
            }
        }
    }
    float vreg[2][3][8];                                   // V^T[d = 32 wave + 16 d2 + r][key 32 ks + 8 q + u]
#pragma unroll
    for (int ks = 0; ks < 3; ks++)
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int j = ks * 32 + q * 8 + u;
            int ring = head0 + j;
            if (ring >= KVC) ring -= KVC;
            const float *vrow = vbase + (size_t)ring * D + wave * 32 + r;
            vreg[0][ks][u] = j < span ? vrow[0] : 0.0f;
            vreg[1][ks][u] = j < span ? vrow[16] : 0.0f;
        }
    // ---- phase 0: (q + u), (q + v) -> bf16 hi / lo images ----
#pragma unroll
    for (int it = 0; it < 2; it++) {
        const int e = threadIdx.x + it * 256, i = e >> 5, c4 = (e & 31) * 4;
        const int off = i * 256 + ((((c4 >> 3) ^ i) & 15) << 4) + (c4 & 7) * 2;
        const float4 x = qreg[it], u = ureg[it], v = breg[it];
        uint2 hi, lo;
        as_split2(x.x + u.x, x.y + u.y, hi.x, lo.x);
        as_split2(x.z + u.z, x.w + u.w, hi.y, lo.y);
        *(uint2 *)(qu_s + off) = hi;
        *(uint2 *)(qu_s + SS_IMG + off) = lo;
        as_split2(x.x + v.x, x.y + v.y, hi.x, lo.x);
        as_split2(x.z + v.z, x.w + v.w, hi.y, lo.y);
        *(uint2 *)(qv_s + off) = hi;
        *(uint2 *)(qv_s + SS_IMG + off) = lo;
    }
    __syncthreads();
    // ---- phase 1: key tiles and relative-position tiles, A split in registers ----
#pragma unroll
    for (int n = 0; n < 4; n++) {
        const int t = wave + 4 * n;
        if (live[n]) {
            const bool isk = t < 6;
            const char *bq = isk ? qu_s : qv_s;
            as_f32x4_t acc = (as_f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                uint4 a_hi, a_lo;
                ss_split8(av[n][2 * ks], av[n][2 * ks + 1], a_hi, a_lo);
                const char *bp = bq + r * 256 + ((((ks << 2) | q) ^ r) << 4);
                acc = as_mfma3(a_hi, a_lo, *(const uint4 *)bp, *(const uint4 *)(bp + SS_IMG), acc);
            }
            // D[j][i]: lane holds query i = r, rows 4q + reg
            float *dst = isk ? sk + r * SS_SKP + t * 16 + q * 4 : sp + r * SS_SPP + (t - 6) * 16 + q * 4;
            *(float4 *)dst = make_float4(acc[0], acc[1], acc[2], acc[3]);
        }
    }
    __syncthreads();                          // ... and every read of the query images is done: their first half becomes the weight images
    // ---- phase 2: rel-shift gather + mask + softmax -> hi / lo weights over the span (zero outside the row's window) ----
    const float scale = 0.08838834764831845f;                    // 1/sqrt(128), applied to the sum of the two terms
    for (int i = wave; i < 16; i += 4) {
        const int il = r0 + i, g = il / T, ic = il - g * T;      // (chunk, frame in chunk) of this row
        const int wo = (g - g0) * T;                             // its window starts wo rows into the span
        const int valid = rd.valid_len + g * T < LCTX ? rd.valid_len + g * T : LCTX;
        const int mask_upto = LCTX - valid;
        const int j0 = lane - wo, j1 = lane + 64 - wo;           // window index of span positions lane, lane + 64
        const bool in0 = i < nrows && j0 >= 0 && j0 < KV, in1 = i < nrows && j1 >= 0 && j1 < KV;
        float v0 = -INFINITY, v1 = -INFINITY;
        if (in0) { v0 = (sk[i * SS_SKP + lane] + sp[i * SS_SPP + j0 + T - 1 - ic]) * scale; if (j0 < mask_upto) v0 += -1e9f; }
        if (in1) { v1 = (sk[i * SS_SKP + lane + 64] + sp[i * SS_SPP + j1 + T - 1 - ic]) * scale; if (j1 < mask_upto) v1 += -1e9f; }
        const float mx = wave_max(fmaxf(v0, v1));
        const float e0 = in0 ? __expf(v0 - mx) : 0.0f;
        const float e1 = in1 ? __expf(v1 - mx) : 0.0f;
        const float sum = wave_sum(e0 + e1);
        const float inv = i < nrows ? 1.0f / sum : 0.0f;
        uint32_t hi, lo;
        as_split2(e0 * inv, e1 * inv, hi, lo);
        const int p0 = lane, p1 = lane + 64;
        const int o0 = i * 256 + ((((p0 >> 3) ^ i) & 15) << 4) + (p0 & 7) * 2, o1 = i * 256 + ((((p1 >> 3) ^ i) & 15) << 4) + (p1 & 7) * 2;
        *(bf16_t *)(w_s + o0) = (bf16_t)(hi & 0xffffu);
        *(bf16_t *)(w_s + SS_IMG + o0) = (bf16_t)(lo & 0xffffu);
        *(bf16_t *)(w_s + o1) = (bf16_t)(hi >> 16);
        *(bf16_t *)(w_s + SS_IMG + o1) = (bf16_t)(lo >> 16);
    }
    __syncthreads();
    // ---- phase 3: O^T[d][i] = V^T . w^T, this wave's 2 d tiles x 3 k steps; the V elements are split here ----
#pragma unroll
    for (int d2 = 0; d2 < 2; d2++) {
        as_f32x4_t acc = (as_f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 3; ks++) {
            const float *v = vreg[d2][ks];
            uint4 a_hi, a_lo;
            ss_split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), a_hi, a_lo);
            const char *bp = w_s + r * 256 + (((((ks << 2) | q) ^ r) & 15) << 4);
            acc = as_mfma3(a_hi, a_lo, *(const uint4 *)bp, *(const uint4 *)(bp + SS_IMG), acc);
        }
        if (r < nrows)     // D[d][i]: lane holds query i = r, d = 32 wave + 16 d2 + 4q + reg
            store_wt_f4((float *)p.ctx_out + (row0 + r) * D + h * DH + wave * 32 + d2 * 16 + q * 4, make_float4(acc[0], acc[1], acc[2], acc[3]));
    }
}

void launch_attention_split(const AttnParams &p, hipStream_t st) {
    const int TS = p.TS > 0 ? p.TS : p.T, QB = p.T <= 2 ? 16 : p.T;
    hipLaunchKernelGGL(k_attention_f32_split, dim3(NH, p.B, (TS + QB - 1) / QB), dim3(256), 0, st, p);
}

}  // namespace nasr
