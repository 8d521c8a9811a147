// nasr_conv0_dw.h -- conv0 (3x3 stride-2, 1 -> 256 channels, + ReLU) fused into the first depthwise 3x3 stride-2 conv
// (src/nemo-ggml.cpp:969-978, pads (2 before, 1 after) on both axes :905-913, :936-943): the body of k_sub_conv0_dw
// (kernels_front.hip: a chunk of a stream's mel ring) and of k_off_conv0_dw (kernels_offline.hip: a whole utterance).
// conv0's output [H1][65][256] f32 is 9x larger than its input and was the largest intermediate of the step (260 MB at 64
// streams x R = 13); its 9 MACs per element are cheaper to redo than to store and re-read.  Every conv0 value is formed
// exactly as the unfused kernel formed it (same order; both files are compiled without FMA contraction), so the result is
// bit-identical.
#pragma once
#include "nasr_internal.h"

namespace nasr {

// One workgroup per output row t2, one thread per channel.  sm: the 7 mel rows 4*t2-6 .. 4*t2 the row depends on, zero
// padded (an out-of-range tap adds w*0 where the unfused kernel skipped it: same sum), 6 columns of left pad so that output
// column f2 reads the 7x7 patch at columns 4*f2 .. 4*f2+6 -- staged by the caller, which has not passed a barrier since.
// Writes columns [f2_lo, f2_hi) of row out_row of out [rows][W2][256], channel fastest.
template <bool OUT_BF16>
__device__ __forceinline__ void conv0_dw_row(const float (&sm)[7][144], int t2, int H1, int W1, int W2, int f2_lo, int f2_hi,
                                             const float *w0t /*[9][256]*/, const float *b0, const float *w2t /*[9][256]*/,
                                             const float *b2, void *out, size_t out_row) {
    const int c = threadIdx.x;
    float w0[9], w2[9];
#pragma unroll
    for (int k = 0; k < 9; k++) { w0[k] = w0t[k * SUBC + c]; w2[k] = w2t[k * SUBC + c]; }
    const float bias0 = b0[c], bias2 = b2[c];
    __syncthreads();
    // conv0 column 2*f2 (tap kw2 = 0) is column 2*(f2-1) + 2 (tap kw2 = 2) of the previous output: its three activated
    // values are carried over instead of recomputed (the same values: a third of the conv0 arithmetic less)
    float carry[3] = {0.0f, 0.0f, 0.0f};
    for (int f2 = f2_lo; f2 < f2_hi; f2++) {
        float p[7][8];
#pragma unroll
        for (int r = 0; r < 7; r++) {
            const float4 lo = *(const float4 *)&sm[r][4 * f2], hi = *(const float4 *)&sm[r][4 * f2 + 4];
            p[r][0] = lo.x; p[r][1] = lo.y; p[r][2] = lo.z; p[r][3] = lo.w;
            p[r][4] = hi.x; p[r][5] = hi.y; p[r][6] = hi.z; p[r][7] = hi.w;
        }
        float acc2 = 0.0f;
#pragma unroll
        for (int kh2 = 0; kh2 < 3; kh2++) {
            const int t = 2 * t2 + kh2 - 2;               // conv0 output row feeding this tap
            if (t < 0 || t >= H1) continue;
#pragma unroll
            for (int kw2 = 0; kw2 < 3; kw2++) {
                const int f = 2 * f2 + kw2 - 2;           // conv0 output column
                if (f < 0 || f >= W1) continue;
                float a0;
                if (kw2 == 0 && f2 > f2_lo) a0 = carry[kh2];
                else {
                    float acc = 0.0f;
#pragma unroll
                    for (int kh = 0; kh < 3; kh++)
#pragma unroll
                        for (int kw = 0; kw < 3; kw++) {
                            // bf16 engine (OUT_BF16): fused multiply-adds -- this kernel runs at the f32 VALU's issue rate (134 M outputs x ~130 separate multiplies and
                            // adds at 512 streams x R = 13: 500 us), the result is rounded to bf16 below and compared to the oracle with a tolerance.  The f32
                            // engine keeps the reference's separate roundings (bit-identical subsampling, tests/test_gpu_parity.py).
                            if (OUT_BF16) acc = __builtin_fmaf(w0[kh * 3 + kw], p[2 * kh2 + kh][2 * kw2 + kw], acc);
                            else acc += w0[kh * 3 + kw] * p[2 * kh2 + kh][2 * kw2 + kw];
                        }
                    a0 = fmaxf(acc + bias0, 0.0f);
                }
                if (kw2 == 2) carry[kh2] = a0;
                if (OUT_BF16) acc2 = __builtin_fmaf(w2[kh2 * 3 + kw2], a0, acc2);
                else acc2 += w2[kh2 * 3 + kw2] * a0;
            }
        }
        acc2 += bias2;
        const size_t o = (out_row * W2 + f2) * SUBC + c;
        if (OUT_BF16) ((bf16_t *)out)[o] = f32_to_bf16(acc2);
        else ((float *)out)[o] = acc2;
    }
}

}  // namespace nasr
