// nasr_gemm_plan.h -- which kernel a bf16 GEMM runs on, as a value: the geometry constants the kernels of kernels_gemm.hip and the choice
// share, the list of kernel instances with their LDS sizes (written once: init_gemm_kernel_attributes() and the plan read the same table),
// and gemm_plan_bf16(), the whole ladder of launch_gemm_bf16.  Pure host code without HIP calls, so that it is compiled and swept on a
// CPU under sanitizers (tests/test_gemm_plan.py, against a table recorded from the launcher it replaced).  Include after
// nasr_internal.h (GemmParams, Epi).  The ring depths of round 5's loops (K32_SLOT, T3_NS, W2_NS, WE_LD, wide2_lds) stay in kernels_gemm.hip, beside
// the counted waits written for them and where tests/test_kernel_index_maps.py reads them: the table below holds the sizes they give, checked there.
#pragma once
#include <stddef.h>
namespace nasr {
// ---- geometry ----------------------------------------------------------------------------------------------------------------
constexpr int TM = 128;               // rows of a 128 x 128 / 128 x 64 tile
constexpr int G2_SLOT = 32768;        // ring slot of the 64-deep kernels: 16 KiB activation panel + 16 KiB weight tiles
constexpr int T64_SLOT = 24576, T64_STG_LD = 68;
constexpr int T64W_NS = 3, T64W_HALF = T64W_NS * T64_SLOT;          // 73 728 B per K-half
constexpr int STG_LD = 132;      // floats per staged row (128 + 4: the 16 rows of a float4 store spread over the banks)
constexpr int PS_NS = 3, PS_STAGE = PS_NS * G2_SLOT, PS_LDS = PS_STAGE + 65536;
constexpr int WD_NS = 4;
// MT = 16-row m-tiles per wave: the tile has BM = 32 MT rows.  MT = 8 (256 rows) and MT = 7 (224 rows = 16 streams x R = 13: 7 168 rows
// are 32 of them, so that N = 4096 gives 512 tiles = two FULL rounds of the chip where 256-row tiles give 1.75, and N = 2048 one
// round of 256 smaller tiles instead of 224 larger ones) -- gemm_plan_bf16 takes the one whose rounds x rows is smaller.
template <int BN, int MT> struct WideCfg {
    static constexpr int BM = 32 * MT;
    static constexpr int SLOT = (BM + BN) * 64;               // bytes per 32-deep chunk
    static constexpr int NT = BN / 64;                        // weight fragments (16-row tiles) per wave and chunk
    static constexpr int NP = BM / 16;                        // LDS-DMA pieces of the activation panel (16 rows x 64 B each)
    static constexpr int PIECES = NP + BN / 16;               // + the weight tiles of 1 KiB
    static constexpr int DMA = (PIECES + 7) / 8;              // LDS-DMA instructions per wave and chunk (a wave without a piece of its own repeats the last one)
    static constexpr int STG_LD = BN + 4;                     // floats per staged row
    static constexpr size_t LDS = (size_t)WD_NS * SLOT > (size_t)64 * (BN + 4) * 4 ? (size_t)WD_NS * SLOT : (size_t)64 * (BN + 4) * 4;
};
// the ring of ns slots, or the f32 tile the epilogue parks in it, whichever is larger
constexpr size_t gemm_lds_bytes(int ns) { return (size_t)ns * G2_SLOT > (size_t)TM * STG_LD * 4 ? (size_t)ns * G2_SLOT : (size_t)TM * STG_LD * 4; }
// ---- the kernel instances gemm_plan_bf16 can return: X(id, kernel, dynamic LDS bytes).  kernels_gemm.hip expands the same list into its
// table of kernel pointers, so the set that gets its LDS attribute and the set that is launched are one list. -----------------------------
#define NASR_GEMM_INSTANCES(X)                                                                    \
    X(GI_SKINNY1, (k_gemm_skinny<1>), 0)                                                          \
    X(GI_SKINNY2, (k_gemm_skinny<2>), 0)                                                          \
    X(GI_SKINNY4, (k_gemm_skinny<4>), 0)                                                          \
    X(GI_TILED2_K32, (k_gemm_tiled2_k32<4>), 67584)          /* the staged tile: > 4 x 16 KiB */     \
    X(GI_T64W, (k_gemm_t64w), 2 * T64W_HALF)                                                      \
    X(GI_T64_3, (k_gemm_t64<3>), 3 * T64_SLOT)                                                    \
    X(GI_T64_4, (k_gemm_t64<4>), 4 * T64_SLOT)                                                    \
    X(GI_WIDE2_192_7, (k_gemm_wide2<192, 7>), 139264)         /* eight epilogue regions */       \
    X(GI_WIDE2_256_7, (k_gemm_wide2<256, 7>), 153600)         /* 5 ring slots */                 \
    X(GI_WIDE_256_7, (k_gemm_wide<256, 7>), (WideCfg<256, 7>::LDS))                               \
    X(GI_WIDE_256_8, (k_gemm_wide<256, 8>), (WideCfg<256, 8>::LDS))                               \
    X(GI_PERSIST_PART, (k_gemm_persist<EPI_PART_F32>), PS_LDS)                                    \
    X(GI_PERSIST_SILU, (k_gemm_persist<EPI_SILU_ACT>), PS_LDS)                                    \
    X(GI_PERSIST_QKV, (k_gemm_persist<EPI_QKV>), PS_LDS)                                          \
    X(GI_PERSIST_GLU, (k_gemm_persist<EPI_GLU>), PS_LDS)                                          \
    X(GI_PERSIST_BIAS, (k_gemm_persist<EPI_BIAS_F32>), PS_LDS)                                    \
    X(GI_PERSIST_BIAS_RELU, (k_gemm_persist<EPI_BIAS_RELU_F32>), PS_LDS)                          \
    X(GI_TILED3, (k_gemm_tiled3), 81920)          /* 5 x 16 KiB */                                \
    X(GI_ROLES, (k_gemm_roles<4>), gemm_lds_bytes(4))                                             \
    X(GI_TILED2, (k_gemm_tiled2<4>), gemm_lds_bytes(4))
#define X(id, k, lds) id,
enum GemmInst { NASR_GEMM_INSTANCES(X) GI_COUNT };
#undef X
#define X(id, k, lds) (int)(lds),
constexpr int GEMM_INST_LDS[GI_COUNT] = {NASR_GEMM_INSTANCES(X)};
#undef X
#define X(id, k, lds) #k,
constexpr const char *GEMM_INST_NAME[GI_COUNT] = {NASR_GEMM_INSTANCES(X)};
#undef X

struct GemmPlan {
    GemmInst inst;
    unsigned grid[3];
    int block, lds;                    // lds = GEMM_INST_LDS[inst]
    int n_groups, m_chunks;            // the kernel's two trailing arguments (k_gemm_skinny takes none)
    int splits;                        // GemmParams::splits as the kernel is to see it
};

// ---- the rules --------------------------------------------------------------------------------------------------------------
// Largest M served by the weight-streaming ("skinny") kernel; above it the LDS-tiled kernels take over.  Round 1 had 128 (chosen
// on synchronous steps).  Re-measured in round 2 (ms per step, <= 32 / <= 64 / <= 128 rows skinny):
//   three lanes: 64 streams x R = 0 (M = 64) 1.15 / 1.33 / 1.33; 40 / 48 streams x R = 0 1.04 / 1.13 and 1.06 / 1.19 / -;
//                64 x R = 1 (M = 128) 1.29 / 1.30 / 1.89; 8 x R = 13 and 16 x R = 6 (M = 112) 1.13 / 1.13 / 1.62;
//                32 rows and fewer: skinny wins (32 streams x R = 0 0.94 against 1.00 tiled; 16 x R = 1 0.89 / 0.99)
//   synchronous: M = 64 2.66 / - / 2.56, M = 48 2.56 / - / 2.41, M = 112 2.66 / - / 2.81, M = 128 2.95 / - / 3.17
// -> 32 rows.  ONE threshold for both modes: which kernel a GEMM runs on must not depend on the mode, or pipelined steps would
// stop being bit-identical to synchronous ones (the synchronous step pays <= 6 % for it between 33 and 64 rows and gains above).
constexpr int gemm_skinny_max_m() { return 32; }

// 128 x 64 tiles (k_gemm_t64): for the split-K GEMMs with N = 1024 when that halves the split factor, and for any other GEMM
// whose 128 x 128 tiling gives at most 64 workgroups (a quarter of the CUs).  With pipelined steps "fill the chip" is the wrong
// rule for the in-between sizes: CUs one launch leaves idle run another chain's kernels.  Measured with three lanes, half-width
// tiles wherever the 128 x 128 tiling had <= 128 workgroups against the split-K form only: 16 streams x R = 13 (32-64 tiles)
// 1.22 vs 1.32 ms per step, 32 streams (64-128 tiles) 1.82 vs 1.77, 64 streams (pw1: 112 tiles -> 224) 2.66 vs 2.65 -- although
// alone the 112-tile launch takes 13.3 us and the vendor library's MT128x64 kernel 10.6 (tests/prof_gemm_shapes.sh).
// Round 4: for the split-K GEMMs only up to 64 tiles of 128 x 128 (M <= 1 024).  Above that two K-halves of 128 x 128 tiles fill the chip by themselves
// (72-120 tiles x 2 <= 256 workgroups) where the half-width form makes 288-480 workgroups of a shape that moves 1.5 x the operand bytes per flop: 112 streams
// x R = 13 (104 tiles) synchronous 5.92 -> 5.30 ms, pipelined 3.82 -> 3.77; 128 streams (112 tiles) pipelined 4.21 -> 4.14, synchronous 5.52 -> 5.69
// (profiles/r4_tile_order.md).  Engine option "t64_tiles": t64_p1 = GemmParams::t64_tiles_p1 (the engine's option + 1; 0 = the default of 64), carried per
// GEMM so that several engines in one process cannot change each other's choice; gemm_pick_splits() and gemm_plan_bf16() both ask here.
inline bool gemm_use_t64(int M, int N, int epi, int t64_p1) {
    if (M <= gemm_skinny_max_m()) return false;
    const int tiles = (N / 128) * ((M + 127) / 128);
    if (epi == EPI_PART_F32) return N == 1024 && tiles <= (t64_p1 > 0 ? t64_p1 - 1 : 64);
    return tiles <= 64;
}
// output-tile width the large-M kernel will use (128, or 64 for the N = 1024 split-K GEMMs)
inline int gemm_tile_n(int M, int N, int epi, int t64_p1) { return gemm_use_t64(M, N, epi, t64_p1) ? 64 : 128; }
// EPI_RESID_F32 needs the complete K sum in one workgroup: the welded two-slice 128 x 64 form where gemm_pick_splits chose two slices of
// half-width tiles (256 < M <= 1 024 at the default "t64_tiles"), or any launch without split-K
inline bool gemm_welded(int M, int N, int K, int splits, int t64_p1) {
    return splits == 2 && (K & 127) == 0 && gemm_use_t64(M, N, EPI_PART_F32, t64_p1);
}
// a GEMM whose A rows come out of a k_post can carry that k_post as its head phase (GemmParams::chain) when it runs on the 128 x 128 tiles of
// k_gemm_tiled2_k32: more than 32 rows, no split-K, N a multiple of 128, at most 64 row chunks (the counters)
inline bool gemm_chain_ok(int M, int N, int K, int splits) {
    return M > gemm_skinny_max_m() && splits == 1 && N % 128 == 0 && (K & 63) == 0 && (M + TM - 1) / TM <= 64;
}
// can a residual GEMM (N = 1024 ... D columns, `splits` K slices by gemm_pick_splits) add its product to the residual stream in its own epilogue
// (EPI_RESID_F32)?  Yes where one workgroup owns the complete K sum of a tile: no split-K, or the two-slice 128 x 64 form (k_gemm_t64w)
inline bool gemm_resid_foldable(int M, int N, int K, int splits, int t64_p1) {
    if (M <= gemm_skinny_max_m()) return false;
    return splits == 1 || gemm_welded(M, N, K, splits, t64_p1);
}

// K slices of a residual GEMM (part = A.W^T, followed by k_post); split_tasks = engine option "split_tasks" (0 = the rule, 200)
inline int gemm_pick_splits(bool bf16, int M, int N, int K, int t64_p1, int split_tasks) {
    if (!bf16) return 1;
    const bool skinny = M <= gemm_skinny_max_m();
    int tasks = skinny ? (N / 16) * ((M + 63) / 64) : (N / gemm_tile_n(M, N, EPI_PART_F32, t64_p1)) * ((M + 127) / 128);
    // partial traffic grows with the split factor, and with pipelined steps the CUs a launch leaves idle run another chain's
    // kernels: four splits only up to 40 tiles (three lanes, R = 13: 12 / 16 streams = 32 tiles 1.15 / 1.23 ms with 4 splits
    // against 1.23 / 1.30 with 2; 24 streams = 48 tiles 1.53 vs 1.50; 32 streams = 64 tiles 1.82 vs 1.68; 64 streams = 112 tiles:
    // 2 splits 2.76, 1 split 2.75, 4 splits 3.03)
    // Round 5: one slice from 200 tiles of 128 x 128 (256 streams x R = 13: 224 tiles, 7.76 -> 7.48 ms per pipelined step): that many workgroups fill the chip
    // by themselves, and a GEMM that owns its tiles' whole K sums adds to the residual stream in its own epilogue -- no partial slabs, k_post is the
    // LayerNorm alone.  Counted in 128 x 128 tiles whatever the tile the plan takes, so that every kernel variant sums in the same order.
    if (!skinny && (N / 128) * ((M + 127) / 128) >= (split_tasks > 0 ? split_tasks : 200)) return 1;
    if (!skinny) return tasks <= 40 ? 4 : (tasks < 256 ? 2 : 1);
    constexpr int skinny_cap = 8;
    int s = 1;
    while (s < skinny_cap && tasks * s < 256 && (K / 32) / (s * 2) >= 4) s *= 2;
    return s;
}

// Pipelined steps (GemmParams::coresident): four launch chains advance in lock-step rounds, so the GEMM launches of a round start
// together and, with one 96-128 KiB workgroup per CU, run one after the other -- a round costs the SUM of its GEMMs.  With rings of
// <= 72 KiB two of them share every CU: one workgroup's ring fill and barrier waits run under the other's MFMAs (64 streams x
// R = 13: 2.64 -> 2.48 ms per step; alone on the chip the shallower rings cost 8 %, so synchronous steps keep the deep ones).
// From seven 128-row tiles up (M > 768), where every GEMM of the step covers most of the chip: measured per step with four lanes,
// 64 streams x R = 13 (M = 896) 2.61 -> 2.47 ms, 48 streams (M = 672) 2.05 -> 2.03, 40 streams (M = 560) 1.76 -> 1.81, 32 streams 1.51 -> 1.59.
inline bool gemm_coresident(const GemmParams &p, int num_cus) {
    constexpr int min_m = 769;
    if (p.coresident >= 2) return p.coresident == 2;          // engine option "gemm_cores" (A/B runs, the bit-identity test)
    // more than one wave of tiles (M >= 1 792): workgroups of ONE launch start as earlier ones finish, so the two on a CU are out of
    // phase by themselves -- synchronous steps gain as well (128 streams x R = 13: 6.51 -> 5.95 ms, 512 streams 19.9 -> 18.6 ms).
    // Only with more tiles than CUs: a launch that puts at most one workgroup on a CU has nothing to pair and keeps the deep rings
    // (cold operands, us per launch, deep / shallow: 1 792 rows pw1 224 tiles 12.6 / 16.7, W2 112 tiles 28.3 / 32.4; 3 584 rows W2 224 tiles
    // 34.7 / 45.1, Wo 12.0 / 14.8 -- profiles/r4_tile_order.md)
    if (p.coresident == 1 && p.M >= min_m) return true;
    const long tiles = (long)(p.N / gemm_tile_n(p.M, p.N, p.epi, p.t64_tiles_p1)) * ((p.M + TM - 1) / TM) * (p.splits < 1 ? 1 : p.splits);
    return p.M >= 1792 && tiles > num_cus;
}
// round 5's loops (k_gemm_wide2, k_gemm_tiled3) unless GemmParams::prio >> 2 == 5: rounds 1-4's (engine option "gemm_prio" = 20: A/B runs, gemm_variant_identity.py).
// The probes this field also selected during the round (s_setprio around the MFMA cluster, "every fragment first", DMA between the MFMA groups on the old kernels) are
// gone from the tree: profiles/r5_gemm_tile_stamps.md, r5_gemm_loops_probe_{7168,896}.txt.
inline bool gemm_new_loops(const GemmParams &p) { return (p.prio >> 2) == 0 || (p.prio >> 2) == 4; }

// ---- the plan: every rung of the ladder in the order the launcher had them; p.splits < 1 counts as 1 -------------------------------
inline GemmPlan gemm_plan_bf16(const GemmParams &p, int num_cus) {
    const int splits = p.splits < 1 ? 1 : p.splits;
    const auto plan = [](GemmInst inst, unsigned gx, int block, int n_groups, int m_chunks, int ks) { return GemmPlan{inst, {gx, 1, 1}, block, GEMM_INST_LDS[inst], n_groups, m_chunks, ks}; };
    if (p.M <= gemm_skinny_max_m()) {
        GemmPlan s = plan(p.M <= 16 ? GI_SKINNY1 : p.M <= 32 ? GI_SKINNY2 : GI_SKINNY4, (unsigned)(p.N / 16), 256, 0, 0, splits);
        s.grid[1] = (unsigned)splits; s.grid[2] = (unsigned)((p.M + 63) / 64);
        return s;
    }
    const int n_groups = p.N / 128, m_chunks = (p.M + TM - 1) / TM;
    const unsigned tiles128 = (unsigned)(n_groups * m_chunks * splits);
    // chained launch (the caller asked gemm_chain_ok()): k_gemm_tiled2_k32 is the kernel that carries a head phase
    if (p.chain.head_wgs > 0) return plan(GI_TILED2_K32, p.chain.head_wgs + tiles128, 512, n_groups, m_chunks, splits);
    // the caller asked gemm_resid_foldable(): both K slices in one 16-wave workgroup; the kernel sees splits = 1 (tile_of(): one workgroup per tile)
    if (p.epi == EPI_RESID_F32 && splits == 2) return plan(GI_T64W, (unsigned)((p.N / 64) * m_chunks), 1024, p.N / 64, m_chunks, 1);
    const bool cores = gemm_coresident(p, num_cus);
    // half-width tiles: the caller chose splits for N / 64 column groups (gemm_tile_n); 3 slots = 72 KiB: two workgroups per CU
    if (gemm_use_t64(p.M, p.N, p.epi, p.t64_tiles_p1)) return plan(cores ? GI_T64_3 : GI_T64_4, (unsigned)((p.N / 64) * m_chunks * splits), 512, p.N / 64, m_chunks, splits);
    // more than one wave of tiles: 256 x 256 tiles (half the operand bytes per flop) where their rounds fill the chip -- the last round at
    // least 5 / 8 full, or three rounds and more (persist_probe, cold operands, us per launch against the per-tile pair: 7 168 rows W1 448
    // tiles 78 / 83, pw1 224 tiles 38 / 45, QKV 336 tiles 69 / 70: a wash, left alone; 15 360 rows N = 1024 240 tiles 109 / 160).  The
    // 256 x 128 form measured worse than the per-tile kernels with cold operands (W2 at 7 168 rows 92 / 77) and is not used.
    // Synchronous steps only -- alone on the chip the QKV launch at 7 168 rows takes 52 us instead of 62, but a pipelined 512-stream step got SLOWER with it
    // (13.65 against 13.50 ms, same box, three-way A/B): the half-empty round is where the other lanes' launches run.
    // N = 3072 (QKV) on 224 x 192 tiles where 224 x 256 leaves a half-empty last round: 7 168 rows 384 tiles = 1.5 rounds -> 512 = two full rounds of
    // 3 / 4-size tiles, 3 584 rows 192 tiles (0.75 of the chip) -> 256.  k_gemm_wide2 only (its wave-private epilogue takes 48-column blocks).
    const bool wide2_ok = gemm_new_loops(p) && (p.K & 63) == 0 && p.K >= 256;          // k_gemm_wide2 needs K / 32 even and >= 8
    if (!p.no_wide && wide2_ok && p.coresident != 1 && splits == 1 && p.M >= 1792 && p.N % 192 == 0 && p.N % 256 == 0) {
        const long mw = (p.M + 223) / 224, t192 = (long)(p.N / 192) * mw, t256 = (long)(p.N / 256) * mw;
        const long c192 = (t192 + num_cus - 1) / num_cus * 192, c256 = (t256 + num_cus - 1) / num_cus * 256;
        if (c192 < c256 && t192 >= (long)num_cus * 7 / 8) return plan(GI_WIDE2_192_7, (unsigned)t192, 512, p.N / 192, (int)mw, splits);
    }
    if (!p.no_wide && splits == 1 && p.M >= (p.coresident == 1 ? (p.wide_min_rows > 0 ? p.wide_min_rows : 1344) : 1792) && (p.K & 31) == 0 && p.N % 256 == 0) {
        // 256- or 224-row tiles: whichever needs fewer rounds x rows (7 168 rows: N = 4096 two full rounds of 224-row tiles instead of
        // 1.75 of 256-row ones, N = 2048 one round of 256 smaller tiles; 15 360 rows stay at 256).  Cold operands, us per launch, 256 / 224 rows:
        // W1 at 7 168 rows 78.8 / 74.9, pw1 38.4 / 35.4, W1 at 3 584 rows 43.8 / 41.0; synchronous steps 512 streams 18.08 -> 17.82 ms, 256
        // streams 9.56 -> 9.42; pipelined steps (three pieces) 384 streams 10.95 -> 10.82, 512 streams 14.32 = (profiles/r4_wide_tiles.md).
        int best_mt = 0;
        long best_cost = 0;
        for (int mt = 8; mt >= 7; mt--) {
            const int bm = 32 * mt, mw = (p.M + bm - 1) / bm;
            const long tiles = (long)(p.N / 256) * mw, last = tiles % num_cus;
            if (!(tiles >= (long)num_cus * 7 / 8 && (last == 0 || last * 8 >= (long)num_cus * 5 || tiles >= (long)num_cus * 3))) continue;
            const long cost = (tiles + num_cus - 1) / num_cus * bm;
            if (!best_mt || cost < best_cost) { best_mt = mt; best_cost = cost; }
        }
        // Pipelined steps (other lanes' workgroups fill the CUs a launch leaves idle): 224-row tiles from 32 of them (round 4: 96; round 5, profiles/r5_gemm_tile_stamps.md section 3:
        // what a pipelined step pays for a GEMM is its CU-time, and a 224 x 256 tile costs 40 % less of it than four 128 x 128 ones -- 256 streams 7.4 -> 7.2 ms), where the rule above finds
        // too few to fill the chip.  What a pipelined step is short of is operand delivery -- at 64 streams the LDS fills of a step's
        // 128 x 128 tiles add up to 23 GB = 9.5 TB/s, between what the Infinity Cache (8.6) and an XCD's L2 (17-19) deliver -- and a
        // 224 x 256 tile moves 0.54 of the bytes per flop.  ms per step, four lanes, without / with: 96 streams 3.37 / 3.33, 128 streams
        // 4.30 / 4.19, 192 streams 6.22 / 6.02; from 64 tiles: 4.21 (128 streams), 3.35 (96); at 64 streams (64 / 48 / 32 tiles) 2.42 -> 2.54, W1's 64 tiles alone 2.415 -> 2.449: not taken.
        // With it: 256 streams 8.00 -> 7.93, 384 streams 11.75 -> 11.43, 512 streams (every GEMM of the layer on these tiles) 15.31 -> 14.49.
        if (!best_mt && p.coresident == 1 && p.wide_rows != 2 && (long)(p.N / 256) * ((p.M + 223) / 224) >= (p.wide_min_tiles > 0 ? p.wide_min_tiles : 32)) best_mt = 7;      // engine option "wide_min_tiles"
        if (p.wide_rows == 256 && best_mt) best_mt = 8;      // engine option "wide_tiles" = 256: round 4's first form only
        if (best_mt) {
            const int mw = (p.M + 32 * best_mt - 1) / (32 * best_mt);
            return plan(best_mt == 8 ? GI_WIDE_256_8 : wide2_ok ? GI_WIDE2_256_7 : GI_WIDE_256_7, (unsigned)((long)(p.N / 256) * mw), 512, p.N / 256, mw, splits);
        }
    }
    // several 128 x 128 tiles per CU: the persistent tile loop (one workgroup per CU; ring fills and epilogues off the critical path).
    // From 1.75 tiles per CU: below that a workgroup has no second tile to hide anything under.
    if (!p.no_persist && splits == 1 && p.K >= 1024 && (p.K & 63) == 0 && (long)n_groups * m_chunks * 4 >= (long)num_cus * 7) {
        const int inst = p.epi == EPI_PART_F32 ? GI_PERSIST_PART : p.epi == EPI_SILU_ACT ? GI_PERSIST_SILU : p.epi == EPI_QKV ? GI_PERSIST_QKV : p.epi == EPI_GLU ? GI_PERSIST_GLU
                       : p.epi == EPI_BIAS_F32 ? GI_PERSIST_BIAS : p.epi == EPI_BIAS_RELU_F32 ? GI_PERSIST_BIAS_RELU : -1;
        if (inst >= 0) return plan((GemmInst)inst, (unsigned)num_cus, 1024, n_groups, m_chunks, splits);      // the act-dtype bias epilogues (subsampling) stay on the per-tile kernels
    }
    // two workgroups per CU: k_gemm_tiled3 (5 x 16 KiB; an even number of 32-deep chunks >= 6 per K slice), else k_gemm_tiled2_k32 (4 x 16 KiB ring + the staged tile: 66 KiB)
    if (cores && gemm_new_loops(p) && ((p.K >> 6) / splits) * 2 >= 6 && (p.K >> 6) % splits == 0) return plan(GI_TILED3, tiles128, 512, n_groups, m_chunks, splits);
    if (cores) return plan(GI_TILED2_K32, tiles128, 512, n_groups, m_chunks, splits);
    constexpr int roles_min_chunks = 8;          // k_gemm_roles from 8 chunks per workgroup; slightly slower below, where k_gemm_tiled2 stays
    return (p.K >> 6) / splits >= roles_min_chunks ? plan(GI_ROLES, tiles128, 1024, n_groups, m_chunks, splits) : plan(GI_TILED2, tiles128, 512, n_groups, m_chunks, splits);
}

}  // namespace nasr
