// kernels_attn_split.hip -- the offline path's full-context relative-position attention for the f32 engine on the bf16 MFMA
// (engine option "f32_split_attn"): f32 operands in HBM, f32 softmax, f32 context, and every matrix product as three
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

}  // namespace nasr
