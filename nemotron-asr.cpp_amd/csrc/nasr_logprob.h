// nasr_logprob.h -- the arithmetic and the index maps of the per-token log-probability (engine option "token_logprobs"), pure code
// without HIP so that the CPU suite compiles it with g++ under sanitizers (tests/test_logprob_math.py), like nasr_gemm_plan.h /
// nasr_offline_plan.h.  kernels_decode.hip includes it and runs the same functions on the device.
//
//   lp(token) = logit[token] - lse,   lse = m + log(sum_v exp(logit[v] - m)),   m = max_v logit[v],   v over the 1025 joint outputs
//
// The joint kernels hold a row's logits spread over lanes, waves and workgroups.  Each writes per row a fixed number of PARTS
// (m, s = sum exp(x - m)) over a fixed slice of the vocabulary, always reduced in the same order:
//   lane     4 consecutive logits of one MFMA accumulator: m = their max, s = the exps added in ascending vocab order   (lane4)
//   tile     16 logits = the four lane groups of a wave: merge(merge(q0, q1), merge(q2, q3)), the xor-16 / xor-32 butterfly (tile16)
//   k_dec_joint (up to 64 rows a step)       one part per 16-entry tile: 65 parts, part = blockIdx.x
//   k_dec_joint_tiled (more rows)            one part per workgroup = 64 entries, its four waves' tiles merged in wave order
//                                            ((w0, w1), w2), w3: 17 parts, part = blockIdx.x (the last holds entry 1024 alone)
// and k_dec_commit merges the parts of the one frame it commits in ascending part index (finish).  Parts go to a scratch
// [key index][n_parts] with plain stores, one writer per element: no atomics, nothing depends on which workgroup finishes first.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NASR_LP_HD __host__ __device__ __forceinline__
#else
#define NASR_LP_HD inline
#endif

namespace nasr_lp {

constexpr int LP_VOCAB = 1025;
constexpr int TILE_W = 16, WG_W = 64;                                   // vocabulary entries per part: k_dec_joint / k_dec_joint_tiled
constexpr int TILE_PARTS = (LP_VOCAB + TILE_W - 1) / TILE_W;            // 65
constexpr int WG_PARTS = (LP_VOCAB + WG_W - 1) / WG_W;                  // 17
constexpr int SMALL_ROWS = 64;                                          // launch rule of launch_decode_iter: B * T rows up to this take k_dec_joint

struct alignas(8) Part { float m, s; };                                           // max and sum of exp(x - max) over a slice; the empty slice is (-inf, 0)

NASR_LP_HD float neg_inf() { return -__builtin_inff(); }
NASR_LP_HD Part empty_part() { Part p; p.m = neg_inf(); p.s = 0.0f; return p; }

// ---- the packed arg-max key: (order-preserving image of the logit's bits) << 32 | (0xffffffff - vocab index) --------------------
NASR_LP_HD uint32_t f32_bits(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
NASR_LP_HD float bits_f32(uint32_t u) { float v; __builtin_memcpy(&v, &u, 4); return v; }
NASR_LP_HD unsigned long long pack_key(float v, int idx) {
    uint32_t u = f32_bits(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                     // order-preserving
    return ((unsigned long long)u << 32) | (unsigned long long)(0xffffffffu - (uint32_t)idx);
}
NASR_LP_HD int key_index_of(unsigned long long key) { return (int)(0xffffffffu - (uint32_t)(key & 0xffffffffull)); }
NASR_LP_HD float key_logit(unsigned long long key) {                    // pack_key is invertible: the winning logit, bit for bit
    const uint32_t u = (uint32_t)(key >> 32);
    return bits_f32((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// ---- parts ---------------------------------------------------------------------------------------------------------------------
// the first n_valid (0 .. 4) of a lane's four logits
NASR_LP_HD Part lane4(float x0, float x1, float x2, float x3, int n_valid) {
    if (n_valid <= 0) return empty_part();
    Part p;
    p.m = x0;
    if (n_valid > 1) p.m = fmaxf(p.m, x1);
    if (n_valid > 2) p.m = fmaxf(p.m, x2);
    if (n_valid > 3) p.m = fmaxf(p.m, x3);
    p.s = expf(x0 - p.m);
    if (n_valid > 1) p.s += expf(x1 - p.m);
    if (n_valid > 2) p.s += expf(x2 - p.m);
    if (n_valid > 3) p.s += expf(x3 - p.m);
    return p;
}
// symmetric in its arguments (both lanes of a butterfly step get the same bits)
NASR_LP_HD Part merge(Part a, Part b) {
    Part p;
    p.m = fmaxf(a.m, b.m);
    if (p.m == neg_inf()) { p.s = 0.0f; return p; }
    p.s = a.s * expf(a.m - p.m) + b.s * expf(b.m - p.m);
    return p;
}
NASR_LP_HD Part tile16(Part q0, Part q1, Part q2, Part q3) { return merge(merge(q0, q1), merge(q2, q3)); }
#if defined(__HIPCC__)
// tile16 on the device, for the joint kernels (kernels_decode.hip, kernels_align.hip): lane (q, r) of a wave holds entries v0 .. v0 + 3 of row r's
// logits, the four lane groups meet over the xor-16 / xor-32 butterfly; every lane of the row ends up with the same bits (merge is symmetric)
__device__ __forceinline__ Part tile_part_wave(float x0, float x1, float x2, float x3, int v0);
#endif
NASR_LP_HD Part wg64(Part w0, Part w1, Part w2, Part w3) { return merge(merge(merge(w0, w1), w2), w3); }
NASR_LP_HD int lane_valid(int v0) { const int n = LP_VOCAB - v0; return n < 0 ? 0 : (n > 4 ? 4 : n); }     // of the lane's entries v0 .. v0 + 3

#if defined(__HIPCC__)
__device__ __forceinline__ Part tile_part_wave(float x0, float x1, float x2, float x3, int v0) {
    Part a = lane4(x0, x1, x2, x3, lane_valid(v0)), b;
    b.m = __shfl_xor(a.m, 16); b.s = __shfl_xor(a.s, 16);
    a = merge(a, b);
    b.m = __shfl_xor(a.m, 32); b.s = __shfl_xor(a.s, 32);
    return merge(a, b);
}
#endif

// lp of the winning logit from a row's parts, merged in ascending part index.  logit - (m + log s) is evaluated as (logit - m) - log s: the
// same value, but its rounding error does not grow with |m| (the winning logit IS m, so the first difference is exactly 0)
NASR_LP_HD float finish(float logit, const Part *parts, int n_parts) {
    float m = neg_inf();
    for (int i = 0; i < n_parts; i++) m = fmaxf(m, parts[i].m);
    float s = 0.0f;
    for (int i = 0; i < n_parts; i++) s += parts[i].s * expf(parts[i].m - m);
    return (logit - m) - logf(s);
}

// engine option "frame_blank_logprobs": lp of BLANK from a row's parts.  Blank is vocabulary entry 1024 = LP_VOCAB - 1, and in both layouts the last
// part holds that entry alone: 1024 = 64 * 16 is entry 0 of tile 64 (the 65th part of width 16), whose other 15 entries lie past the vocabulary,
// and 1024 = 16 * 64 is entry 0 of workgroup 16 (the 17th part of width 64), whose tiles 65 .. 67 do not exist (empty parts).  lane4 with one valid
// entry leaves m = that entry, and merging with empty parts keeps m, so parts[n_parts - 1].m is blank's raw logit bit for bit and the joint kernels
// need nothing new.  Blank never gets a phrase bonus, so the raw logit is also what the arg-max saw.
static_assert((LP_VOCAB - 1) % TILE_W == 0 && (LP_VOCAB - 1) / TILE_W == TILE_PARTS - 1, "blank is alone in the last 16-entry part");
static_assert((LP_VOCAB - 1) % WG_W == 0 && (LP_VOCAB - 1) / WG_W == WG_PARTS - 1, "blank is alone in the last 64-entry part");
// blank_lp = finish(parts[n_parts - 1].m, parts, n_parts): the same parts in the same ascending order, but the sum, the difference and the
// logarithm are taken in f64 and the caller rounds to f32 once (k_dec_commit).  Two reasons, both specific to blank.  Blank is mostly NOT
// the arg-max where a token is emitted, so logit - m is not 0 and the value can be large (-150 at a sharp joint): an f32 subtraction there
// rounds at half an ulp of 128 .. 256 = 7.6e-6, and the final one again.  And where blank does not win many parts contribute the same small
// term, which an f32 running sum rounds the same way 65 times over: 3.5e-6 on the "large negative logits" row of tests/test_frame_blank_math.py.
// In f64 the value stays within 2e-6 of the float64 softmax at every magnitude and the ring holds its nearest f32.  One thread does this once
// per evaluated row, at most 65 terms: the wider arithmetic costs nothing measurable
NASR_LP_HD double blank_lp(const Part *parts, int n_parts) {
    float m = neg_inf();
    for (int i = 0; i < n_parts; i++) m = fmaxf(m, parts[i].m);
    double s = 0.0;
    for (int i = 0; i < n_parts; i++) s += (double)(parts[i].s * expf(parts[i].m - m));
    return ((double)parts[n_parts - 1].m - (double)m) - log(s);
}

// host restatement of what a kernel leaves in the scratch for one row: `width` = TILE_W or WG_W, out[n_parts_of_width(width)]
NASR_LP_HD int parts_of_width(int width) { return (LP_VOCAB + width - 1) / width; }
NASR_LP_HD Part tile_of(const float *logits, int nt) {                  // 16-entry tile nt of a row's 1025 logits
    Part q[4];
    for (int k = 0; k < 4; k++) {
        const int v0 = nt * TILE_W + k * 4, n = lane_valid(v0);
        q[k] = lane4(n > 0 ? logits[v0] : 0.0f, n > 1 ? logits[v0 + 1] : 0.0f, n > 2 ? logits[v0 + 2] : 0.0f, n > 3 ? logits[v0 + 3] : 0.0f, n);
    }
    return tile16(q[0], q[1], q[2], q[3]);
}
NASR_LP_HD void row_parts(const float *logits, int width, Part *out) {
    const int n = parts_of_width(width);
    for (int p = 0; p < n; p++) {
        if (width == TILE_W) out[p] = tile_of(logits, p);
        else out[p] = wg64(tile_of(logits, 4 * p), tile_of(logits, 4 * p + 1), tile_of(logits, 4 * p + 2), tile_of(logits, 4 * p + 3));
    }
}

// ---- where the parts live ------------------------------------------------------------------------------------------------------
NASR_LP_HD int n_parts(int step_rows) { return step_rows <= SMALL_ROWS ? TILE_PARTS : WG_PARTS; }            // step_rows = B * T of the launch
NASR_LP_HD size_t scratch_parts(int max_step_rows) {                                                         // Parts to allocate
    const size_t small = (size_t)SMALL_ROWS * TILE_PARTS, large = (size_t)(max_step_rows > 0 ? max_step_rows : 0) * WG_PARTS;
    return small > large ? small : large;
}
NASR_LP_HD int key_index(unsigned rowmap_entry, int T) { return (int)(rowmap_entry & 0xffffu) * T + (int)(rowmap_entry >> 16); }   // (frame << 16 | batch row) -> b * T + f
NASR_LP_HD size_t scratch_index(int key_idx, int part, int parts) { return (size_t)key_idx * parts + part; }

// k_dec_joint, grid 65 x 256 threads: the pass over rowmap rows [i0, i0 + 16 * pass_tiles) -- wave w finishes m-tile w, its lanes
// 0 .. 15 (lane group 0) store part blockIdx.x of row i0 + 16 w + lane.  Returns the rowmap row a thread stores for, or -1.
NASR_LP_HD int joint_pass_tiles(int rows_left) { return rows_left <= 16 ? 1 : (rows_left <= 32 ? 2 : 4); }
NASR_LP_HD int joint_store_row(int i0, int pass_tiles, int wave, int lane, int n_rows) {
    if (wave >= pass_tiles || (lane >> 4) != 0) return -1;
    const int i = i0 + wave * 16 + (lane & 15);
    return i < n_rows ? i : -1;
}
// k_dec_joint_tiled, grid (17, ceil(rows / 64)) x 256 threads: threads 0 .. 63 of workgroup (x, y) store part x of row 64 y + thread
NASR_LP_HD int tiled_store_row(int block_y, int thread, int n_rows) {
    if (thread >= 64) return -1;
    const int i = block_y * 64 + thread;
    return i < n_rows ? i : -1;
}

}  // namespace nasr_lp
