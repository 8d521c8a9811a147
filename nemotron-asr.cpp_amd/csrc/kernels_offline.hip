// kernels_offline.hip -- the kernels of the offline (full-context) path that the streaming path has no form of
// (reference src/nemo-ggml.cpp:1038-1079 build_encoder, :668-755 build_rel_pos_mha): whole-utterance subsampling front,
// cache-free depthwise conv, full-context relative-position attention, decode-window gather.  Utterances of a call are
// packed densely (row m of utterance b = row_off[b] + t); no kernel reads a row of another utterance.
#include "nasr_internal.h"
#include "nasr_wave.h"
#include "nasr_post.h"
#include "nasr_offline.h"
#include "nasr_conv0_dw.h"

namespace nasr {

// ---- attention tile constants (tests/test_offline_index_maps.py reads them from this file) ----------------
constexpr int OFF_QB_BF16 = 64;         // query rows per workgroup, bf16 kernel: 4 waves x 16
constexpr int OFF_QB_F32 = 16;          // query rows per workgroup, f32 kernel: 4 waves x 4
constexpr int OFF_BN = 64;              // keys per block of the online softmax
constexpr int OFF_BAND = 80;            // position-table rows computed per (wave, key block): 16 + 64 - 1 = 79, five 16-row tiles
constexpr int OFF_VT_PITCH = 72;        // bf16 per row of the V^T image (64 keys + 8: rows 8 apart share a bank only every 8th row)
constexpr int OFF_SP_PITCH = 84;        // floats per query row of a wave's band scores (80 + 4)
constexpr int OFF_LDS_BF16 = DH * OFF_VT_PITCH * 2 + 4 * 16 * OFF_SP_PITCH * 4;   // 39 936 B
constexpr int OFF_WG_PER_CU = 4;        // 4 x 39 936 B <= 160 KiB of LDS per CU
constexpr int OFF_LDS_F32 = 4 * OFFLINE_MAX_T * 4 + 4 * 2 * DH * 4;                // 36 864 B
static_assert(OFF_LDS_BF16 * OFF_WG_PER_CU <= 160 * 1024, "LDS of the bf16 attention kernel");
static_assert(OFF_LDS_F32 <= 64 * 1024, "LDS of the f32 attention kernel");
static_assert(OFF_BAND >= 16 + OFF_BN - 1, "band covers a 16 x 64 tile");
static_assert(OFF_SP_PITCH >= OFF_BAND, "band row pitch");

typedef __attribute__((ext_vector_type(8))) __bf16 off_bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float off_f32x4_t;

__device__ __forceinline__ uint32_t off_pk2(float x, float y) { return (uint32_t)f32_to_bf16(x) | ((uint32_t)f32_to_bf16(y) << 16); }

// q + bias (f32) rounded to bf16, 8 consecutive dims of one head row
__device__ __forceinline__ uint4 off_q_plus(uint4 raw, const float *bias) {
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; e++)
        o[e] = off_pk2(__uint_as_float(w[e] << 16) + bias[2 * e], __uint_as_float(w[e] & 0xffff0000u) + bias[2 * e + 1]);
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// ---- full-context relative-position attention, bf16 operands on the MFMA (v_mfma_f32_16x16x32_bf16), f32 softmax --------
// One workgroup per (utterance, 64-query block) x head; wave w owns query rows i0 = q0 + 16 w .. + 16 and walks the keys in
// blocks of 64 with an online softmax.  Per key block:
//   content  S^T[j][i] = K[j] . (q_i + u)             4 tiles of 16 keys   (A = key rows straight from global, B = queries)
//   position P[r][i]   = Pos[rbase + r] . (q_i + v)    5 tiles of 16 rows of the band r = (j - j0) - (i - i0) + 15 in [0, 79)
//            the score of (i, j) reads band row (j - j0) - (i - i0) + 15 = table row j - i + 2047 (rel = i - j), skewed through LDS
//   (S + P) / sqrt(128), keys j >= T masked to -inf; O^T[d][i] += V^T[d][k] . p^T[k][i] with V^T staged in LDS once per block.
// The k order of the P.V MFMA is a permutation (lane group q holds keys 4q..4q+3 of two 16-key tiles) used alike for both
// operands, so the exponentials never leave the registers they were formed in.  Rows i >= T are never written.
__global__ __launch_bounds__(256) void k_off_attn_bf16(OffAttnParams p) {
    __shared__ __attribute__((aligned(16))) bf16_t vt[DH * OFF_VT_PITCH];
    __shared__ __attribute__((aligned(16))) float sp[4][16 * OFF_SP_PITCH];
    const int4 it = p.items[blockIdx.x];
    const int h = blockIdx.y, off = it.x, T = it.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
    const int i0 = it.z + 16 * wave;
    const bf16_t *Qb = (const bf16_t *)p.qkv + (size_t)off * OFF_QKV_LD + h * DH;
    const bf16_t *Kb = Qb + D, *Vb = Qb + 2 * D;
    const bf16_t *Pb = (const bf16_t *)p.pos + h * DH;
    int iq = i0 + r;
    if (iq > T - 1) iq = T - 1;                                   // rows past the utterance: valid memory of its own, never written
    uint4 qu[4], qv[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        const uint4 raw = *(const uint4 *)(Qb + (size_t)iq * OFF_QKV_LD + ks * 32 + q * 8);
        qu[ks] = off_q_plus(raw, p.bias_u + h * DH + ks * 32 + q * 8);
        qv[ks] = off_q_plus(raw, p.bias_v + h * DH + ks * 32 + q * 8);
    }
    const float scale = 0.08838834764831845f;                    // 1/sqrt(128), applied to the sum as in the reference
    float m_run = -INFINITY, l_run = 0.0f;
    off_f32x4_t o[8];
#pragma unroll
    for (int dt = 0; dt < 8; dt++) o[dt] = (off_f32x4_t){0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < T; j0 += OFF_BN) {
        __syncthreads();                                          // the previous block's V^T and band reads are done
        {   // V^T image of keys j0 .. j0 + 63 (zeros past T: a weight of 0 never meets a stale value)
            const int j = threadIdx.x >> 2, dq = (threadIdx.x & 3) * 32;
            uint4 v4[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v4[u] = j0 + j < T ? *(const uint4 *)(Vb + (size_t)(j0 + j) * OFF_QKV_LD + dq + 8 * u) : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t w4[4] = {v4[u].x, v4[u].y, v4[u].z, v4[u].w};
#pragma unroll
                for (int e = 0; e < 8; e++)
                    vt[(dq + 8 * u + e) * OFF_VT_PITCH + j] = (bf16_t)((e & 1) ? (w4[e >> 1] >> 16) : (w4[e >> 1] & 0xffffu));
            }
        }
        off_f32x4_t s[4];
#pragma unroll
        for (int kt = 0; kt < 4; kt++) {
            int jr = j0 + 16 * kt + r;
            if (jr > T - 1) jr = T - 1;                           // masked below
            off_f32x4_t acc = (off_f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                const uint4 a = *(const uint4 *)(Kb + (size_t)jr * OFF_QKV_LD + ks * 32 + q * 8);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(off_bf16x8_t, a), __builtin_bit_cast(off_bf16x8_t, qu[ks]), acc, 0, 0, 0);
            }
            s[kt] = acc;
        }
        const int rbase = j0 - i0 + (OFFLINE_MAX_T - 16);         // table row of band row 0: j0 - (i0 + 15) + 2047
#pragma unroll
        for (int pt = 0; pt < OFF_BAND / 16; pt++) {
            int rr = rbase + 16 * pt + r;
            if (rr > OFFLINE_NREL - 1) rr = OFFLINE_NREL - 1;     // only band row 79 can lie past the table, and no score reads it
            off_f32x4_t acc = (off_f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                const uint4 a = *(const uint4 *)(Pb + (size_t)rr * D + ks * 32 + q * 8);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(off_bf16x8_t, a), __builtin_bit_cast(off_bf16x8_t, qv[ks]), acc, 0, 0, 0);
            }
            *(float4 *)&sp[wave][r * OFF_SP_PITCH + 16 * pt + 4 * q] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        }
        __syncthreads();
        // scores of query r, keys j0 + 16 kt + 4 q + e; the four lanes r, r + 16, r + 32, r + 48 hold the 64 keys of one query
        float sv[4][4], mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; kt++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int jl = 16 * kt + 4 * q + e;
                float v = (s[kt][e] + sp[wave][r * OFF_SP_PITCH + jl - r + 15]) * scale;
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
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            const uint4 b = make_uint4(off_pk2(sv[2 * ks][0], sv[2 * ks][1]), off_pk2(sv[2 * ks][2], sv[2 * ks][3]),
                                       off_pk2(sv[2 * ks + 1][0], sv[2 * ks + 1][1]), off_pk2(sv[2 * ks + 1][2], sv[2 * ks + 1][3]));
#pragma unroll
            for (int dt = 0; dt < 8; dt++) {
                const bf16_t *row = vt + (16 * dt + r) * OFF_VT_PITCH + 32 * ks + 4 * q;
                const uint2 lo = *(const uint2 *)row, hi = *(const uint2 *)(row + 16);
                const uint4 a = make_uint4(lo.x, lo.y, hi.x, hi.y);
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(off_bf16x8_t, a), __builtin_bit_cast(off_bf16x8_t, b), o[dt], 0, 0, 0);
            }
        }
    }
    if (i0 + r < T) {
        const float inv = 1.0f / l_run;
        bf16_t *dst = (bf16_t *)p.ctx + (size_t)(off + i0 + r) * D + h * DH + 4 * q;
#pragma unroll
        for (int dt = 0; dt < 8; dt++) {
            uint2 v;
            v.x = off_pk2(o[dt][0] * inv, o[dt][1] * inv);
            v.y = off_pk2(o[dt][2] * inv, o[dt][3] * inv);
            *(uint2 *)(dst + 16 * dt) = v;
        }
    }
}

// ---- the same in f32 (the f32 engine: parity with the f32 reference), exact two-pass softmax on the VALU ----------------
// One workgroup per (utterance, 16-query block) x head, wave w takes queries q0 + 4 w .. + 4 one after another: lane = key for
// the scores (row of the wave in LDS), lane = dimension for P.V.
__global__ __launch_bounds__(256) void k_off_attn_f32(OffAttnParams p) {
    __shared__ __attribute__((aligned(16))) float qs[4][2][DH];
    __shared__ float sc[4][OFFLINE_MAX_T];
    const int4 it = p.items[blockIdx.x];
    const int h = blockIdx.y, off = it.x, T = it.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float *Qb = (const float *)p.qkv + (size_t)off * OFF_QKV_LD + h * DH;
    const float *Kb = Qb + D, *Vb = Qb + 2 * D;
    const float *Pb = (const float *)p.pos + h * DH;
    const float scale = 0.08838834764831845f;
    for (int qi = 0; qi < 4; qi++) {
        const int i = it.z + 4 * wave + qi;
        const bool live = i < T;
        __syncthreads();
        if (live)
            for (int d = lane; d < DH; d += 64) {
                const float x = Qb[(size_t)i * OFF_QKV_LD + d];
                qs[wave][0][d] = x + p.bias_u[h * DH + d];
                qs[wave][1][d] = x + p.bias_v[h * DH + d];
            }
        __syncthreads();
        float mx = -INFINITY;
        if (live)
            for (int j = lane; j < T; j += 64) {
                const float4 *kr = (const float4 *)(Kb + (size_t)j * OFF_QKV_LD);
                const float4 *pr = (const float4 *)(Pb + (size_t)(j - i + OFFLINE_MAX_T - 1) * D);
                const float4 *u4 = (const float4 *)qs[wave][0], *v4 = (const float4 *)qs[wave][1];
                float s1 = 0.f, s2 = 0.f;
#pragma unroll 8
                for (int c = 0; c < DH / 4; c++) {
                    const float4 k = kr[c], pp = pr[c], a = u4[c], b = v4[c];
                    s1 += a.x * k.x; s1 += a.y * k.y; s1 += a.z * k.z; s1 += a.w * k.w;
                    s2 += b.x * pp.x; s2 += b.y * pp.y; s2 += b.z * pp.z; s2 += b.w * pp.w;
                }
                const float v = (s1 + s2) * scale;
                sc[wave][j] = v;
                mx = fmaxf(mx, v);
            }
        mx = wave_max(mx);
        float sum = 0.f;
        if (live)
            for (int j = lane; j < T; j += 64) {
                const float e = __expf(sc[wave][j] - mx);
                sc[wave][j] = e;
                sum += e;
            }
        sum = wave_sum(sum);
        __syncthreads();
        if (live) {
            const float inv = 1.0f / sum;
            for (int d = lane; d < DH; d += 64) {
                float acc = 0.f;
                for (int j = 0; j < T; j++) acc += (sc[wave][j] * inv) * Vb[(size_t)j * OFF_QKV_LD + d];
                ((float *)p.ctx)[(size_t)(off + i) * D + h * DH + d] = acc;
            }
        }
    }
}

int off_attn_qb(int act_bf16) { return act_bf16 ? OFF_QB_BF16 : OFF_QB_F32; }

void launch_off_attention(const OffAttnParams &p, int n_items, int act_bf16, hipStream_t st) {
    if (n_items <= 0) return;
    if (act_bf16) hipLaunchKernelGGL(k_off_attn_bf16, dim3(n_items, NH), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_off_attn_f32, dim3(n_items, NH), dim3(256), 0, st, p);
}

// ---- depthwise conv with a zero causal history of ks - 1 frames + LayerNorm + SiLU: one workgroup per row --------------
// k_dwconv's arithmetic (same order: z0 w0, then + z_k w_k) with the conv cache replaced by zeros; tpos[m] = frame of row m
// within its utterance, so rows in front of frame 0 (another utterance) are never read.
__global__ __launch_bounds__(256) void k_off_dwconv(const float *glu, const int *tpos, const float *dw, int ks, const float *ln_w,
                                                    const float *ln_b, void *out, int act_bf16) {
    __shared__ float sh[8];
    const int m = blockIdx.x, t = tpos[m], c4 = threadIdx.x * 4, ks1 = ks - 1;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < ks; k++) {
        const int back = ks1 - k;                                 // rows before this one
        const float4 z = t >= back ? *(const float4 *)(glu + (size_t)(m - back) * D + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 w = *(const float4 *)(dw + (size_t)k * D + c4);
        if (k == 0) acc = make_float4(z.x * w.x, z.y * w.y, z.z * w.z, z.w * w.w);
        else { acc.x += z.x * w.x; acc.y += z.y * w.y; acc.z += z.z * w.z; acc.w += z.w * w.w; }
    }
    const float4 lw = *(const float4 *)(ln_w + c4), lb = *(const float4 *)(ln_b + c4);
    float4 n = ln4(acc, lw, lb, sh, threadIdx.x);
    n.x = n.x / (1.0f + __expf(-n.x)); n.y = n.y / (1.0f + __expf(-n.y));
    n.z = n.z / (1.0f + __expf(-n.z)); n.w = n.w / (1.0f + __expf(-n.w));
    store_act4(out, (size_t)m * D + c4, n, act_bf16);
}
void launch_off_dwconv(const float *glu, const int *tpos, int M, const float *dw, int ks, const float *ln_w, const float *ln_b,
                       void *out, int act_bf16, hipStream_t st) {
    if (M > 0) hipLaunchKernelGGL(k_off_dwconv, dim3(M), dim3(256), 0, st, glu, tpos, dw, ks, ln_w, ln_b, out, act_bf16);
}

// ---- conv0 + the first depthwise conv (nasr_conv0_dw.h) on a whole utterance --------------------------------------------
// The mel is read from the packed utterance buffer instead of a stream's ring.  Grid = (H2 max, utterances); out rows of
// utterance b start at desc.out_row (rows of [W2][256]).
template <bool OUT_BF16>
__global__ __launch_bounds__(256) void k_off_conv0_dw(const OffSubDesc *desc, const float *mel_all, const float *w0t, const float *b0,
                                                      const float *w2t, const float *b2, void *out) {
    constexpr int W1 = 65, W2 = 33;
    __shared__ __attribute__((aligned(16))) float sm[7][144];
    const OffSubDesc dd = desc[blockIdx.y];
    const int t2 = blockIdx.x, n_mel = dd.n_mel;
    const int H1 = n_mel / 2 + 1, H2 = H1 / 2 + 1;
    if (n_mel <= 0 || t2 >= H2) return;                           // whole workgroup (no barrier is skipped by part of it); no mel: no rows
    const float *mel = mel_all + (size_t)dd.mel_off * NMEL;
    for (int i = threadIdx.x; i < 7 * 144; i += 256) {
        const int rr = i / 144, iw = i - rr * 144 - 6, ih = 4 * t2 - 6 + rr;
        sm[rr][i - rr * 144] = (ih >= 0 && ih < n_mel && iw >= 0 && iw < NMEL) ? mel[(size_t)ih * NMEL + iw] : 0.0f;
    }
    conv0_dw_row<OUT_BF16>(sm, t2, H1, W1, W2, 0, W2, w0t, b0, w2t, b2, out, (size_t)dd.out_row + t2);
}
void launch_off_conv0_dw(const OffSubDesc *desc, int B, int max_h2, const float *mel_all, const float *w0t, const float *b0,
                         const float *w2t, const float *b2, void *out, int out_bf16, hipStream_t st) {
    if (B <= 0 || max_h2 <= 0) return;
    if (out_bf16) hipLaunchKernelGGL(k_off_conv0_dw<true>, dim3(max_h2, B), dim3(SUBC), 0, st, desc, mel_all, w0t, b0, w2t, b2, out);
    else hipLaunchKernelGGL(k_off_conv0_dw<false>, dim3(max_h2, B), dim3(SUBC), 0, st, desc, mel_all, w0t, b0, w2t, b2, out);
}

// ---- decode window: rows [w0, w0 + n_b) of every utterance's joint.enc output -> [B][W][640] (the decode's row layout) ----
__global__ __launch_bounds__(256) void k_off_window(const float *encproj, const int4 *win, int W, float *out) {
    const int t = blockIdx.x, b = blockIdx.y;
    const int4 wd = win[b];                                       // (first packed row of the window, frames in it, -, -)
    if (t >= wd.y) return;
    const float *src = encproj + (size_t)(wd.x + t) * JNT;
    float *dst = out + ((size_t)b * W + t) * JNT;
    for (int c = threadIdx.x; c < JNT; c += 256) dst[c] = src[c];
}
void launch_off_window(const float *encproj, const int4 *win, int B, int W, float *out, hipStream_t st) {
    if (B > 0) hipLaunchKernelGGL(k_off_window, dim3(W, B), dim3(256), 0, st, encproj, win, W, out);
}

// fresh decoder state of the offline slots: zero LSTM state, prev_token = blank, no candidate yet (k_stream_reset's values)
__global__ __launch_bounds__(256) void k_off_dec_reset(int B, float *h, float *c, DecCtrl *ctrl) {
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < 4 * HID; i += 256) { h[(size_t)b * 4 * HID + i] = 0.f; c[(size_t)b * 4 * HID + i] = 0.f; }
    if (threadIdx.x == 0) {
        DecCtrl d;
        d.t = 0; d.n_frames = 0; d.symbols = 0; d.prev_token = BLANK;
        d.cur = 0; d.n_tok = 0; d.active = 0; d.iterations = 0; d.row = 0;
        d.dirty = 1; d.frame0 = 0; d.frame_next = 0;
        ctrl[b] = d;
    }
}
void launch_off_dec_reset(int B, float *h, float *c, DecCtrl *ctrl, hipStream_t st) {
    if (B > 0) hipLaunchKernelGGL(k_off_dec_reset, dim3(B), dim3(256), 0, st, B, h, c, ctrl);
}

}  // namespace nasr
