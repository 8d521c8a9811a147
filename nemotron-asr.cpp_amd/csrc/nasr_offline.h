// nasr_offline.h -- kernels of the offline (full-context) path, kernels_offline.hip; driver in nasr_offline.hip.
#pragma once
#include "nasr_internal.h"
#include "nasr_offline_plan.h"

namespace nasr {

constexpr int OFFLINE_MAX_T = nasr_plan::OFFLINE_MAX_FRAMES;   // 2048
constexpr int OFFLINE_NREL = 2 * OFFLINE_MAX_T - 1;             // 4095 rows of the relative-position table, row r <-> rel = 2047 - r
constexpr int OFF_QKV_LD = 3 * D;                               // q | k | v of a row, act dtype
constexpr int OFF_DEC_WIN = 256;                                // encoder frames per decode window
constexpr int OFF_MIN_ROWS = 64;                                // GEMMs of the path run on at least this many rows (above the skinny kernel's 32)

struct OffAttnParams {
    const void *qkv;              // [M][3072] act dtype
    const void *pos;              // [4095][1024] act dtype (this layer's linear_pos applied to the sinusoid rows)
    const float *bias_u, *bias_v; // [8][128]
    const int4 *items;            // per workgroup: (first packed row of the utterance, T, first query row, 0)
    void *ctx;                    // [M][1024] act dtype
};
struct OffSubDesc { int mel_off, n_mel, out_row, pad; };

int off_attn_qb(int act_bf16);    // query rows per attention workgroup
void launch_off_attention(const OffAttnParams &p, int n_items, int act_bf16, hipStream_t st);
void launch_off_dwconv(const float *glu, const int *tpos, int M, const float *dw, int ks, const float *ln_w, const float *ln_b,
                       void *out, int act_bf16, hipStream_t st);
void launch_off_conv0_dw(const OffSubDesc *desc, int B, int max_h2, const float *mel_all, const float *w0t, const float *b0,
                         const float *w2t, const float *b2, void *out, int out_bf16, hipStream_t st);
void launch_off_window(const float *encproj, const int4 *win, int B, int W, float *out, hipStream_t st);
void launch_off_dec_reset(int B, float *h, float *c, DecCtrl *ctrl, hipStream_t st);

}  // namespace nasr
