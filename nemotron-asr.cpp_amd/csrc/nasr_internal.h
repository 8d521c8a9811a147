// nasr_internal.h -- shared declarations of the HIP engine (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nasr_constants.h"
#include "nasr_logprob.h"
#include "nasr_entropy.h"
#include "nasr_boost.h"
#include "nasr_topk.h"
#include "nasr_align.h"
#include "nasr_beam.h"
#include "nasr_resample.h"
#include "nasr_history.h"

namespace nasr {

typedef uint16_t bf16_t;

struct DecCtrl {          // per-slot decoder control block (device resident)
    int t;                // current encoder frame within the chunk
    int n_frames;         // frames to decode in this chunk
    int symbols;          // symbols emitted for the current frame
    int prev_token;
    int cur;              // which of the two LSTM state versions is committed
    int n_tok;            // tokens written to the token ring so far (monotonic)
    int active;
    int iterations;       // total LSTM+joint evaluations (stat)
    int row;              // batch row of this slot in the current step
    int dirty;            // the uncommitted LSTM candidate / joint.pred vector is stale (committed state changed)
    int frame0;           // absolute encoder-frame index of frame 0 of the current step (token timestamps)
    int frame_next;       // absolute index of the first frame of the next step
};

// ---- epilogues of the GEMM kernels ------------------------------------------------------
enum Epi {
    EPI_PART_F32 = 0,   // out_f32[split][m][n] = acc                      (split-K partials)
    EPI_SILU_ACT,       // out_act[m][n] = silu(acc)
    EPI_QKV,            // n<1024: q f32; else K/V ring rows (act dtype)
    EPI_GLU,            // interleaved (value,gate) pairs -> out_f32[m][n/2] = v*sigmoid(g)
    EPI_BIAS_F32,       // out_f32[m][n] = acc + bias[n]
    EPI_BIAS_RELU_ACT,  // out_act[m][n] = relu(acc + bias[n])
    EPI_BIAS_RELU_F32,  // out_f32[m][n] = relu(acc + bias[n])
    EPI_BIAS_ACT,       // out_act[m][n] = acc + bias[n]
    EPI_RESID_F32,      // out_f32[m][n] = fmaf(resid_scale, acc, resid[m][n])   (round 5: the residual add in the producing GEMM; acc = the complete K sum)
};

struct PostParams {       // x += scale * sum_s part[s]; then LayerNorm(s)
    float *x; int M;
    const float *part; int splits; float scale;   // splits = 0: no residual update
    const float *ln1_w, *ln1_b;   // if ln_out: x = LN1(x) written back first
    int ln_out;
    const float *ln2_w, *ln2_b;   // a = LN2(x) (null: no act output)
    void *a_out; int act_bf16;
    float *copy_out;              // optional f32 copy of the final x (taps / encoder out)
};
// Round 5: a CHAINED launch.  The residual + LayerNorm that produces a GEMM's A rows used to be its own launch (k_post) between the GEMM that
// wrote the residual and the GEMM that reads the normalised rows: 97 launches per 24-layer step whose removal saved 0.41 of a pipelined
// 64-stream step's 2.48 ms (profiles/r5_configs2_launch_structure.md, r5_ablation_b64_R13.json) although their own duration is 5 us -- what they cost is a place in the dependent chain
// (a boundary on either side, a round trip of loads, two reductions).  In a chained launch the first `head_wgs` workgroups of the grid ARE
// that k_post (nasr_post.h: the same body, `head_rows` rows each, in row order), and the tile workgroups behind them start by streaming
// their WEIGHT panels into the LDS ring, then wait until the rows of their own row chunk are published (one counter per row chunk, agent
// scope; MI355X_MICROARCH.md, inter-workgroup visibility: write-through stores + vmcnt(0) + barrier + one atomic add per head workgroup;
// one relaxed poll + buffer_inv sc1 + barrier on the tile side), then fill the activation half of the ring.  Head workgroups never wait and
// have the lowest block ids, so every wait is on a workgroup that is already running or queued ahead; a poll that does not end within
// ~50 ms sets `chain.error` and gives up (the launch then finishes with wrong numbers and the engine reports it) rather than hang the GPU.
struct ChainParams {
    PostParams post;          // rows [0, post.M) = the GEMM's A rows
    int head_wgs;             // 0: an ordinary launch
    int head_rows;            // rows per head workgroup (a divisor of 128: a head workgroup's rows lie in one row chunk)
    unsigned *flags;          // 128 words: [0, 64) rows published per row chunk, [64, 128) tile workgroups of the chunk that have passed the wait (the last one resets both)
    unsigned *error;          // set to 1 by a tile workgroup that gave up waiting
};

struct GemmParams {
    const void *A;        // activations [M][K] (act dtype: bf16 or f32), row stride lda
    const void *W;        // weights: bf16 packed tiles or f32 row-major [N][K]
    int M, N, K;
    int lda;
    // optional batched row map for A: row m -> (m / rows_per_batch)*batch_stride +
    // row_offset*lda + (m % rows_per_batch)*lda ; disabled when rows_per_batch == 0
    int rows_per_batch, batch_stride, row_offset;
    int splits;           // split-K factor (EPI_PART_F32 only)
    int epi;
    float *out_f32;  int ldo;     // f32 output / partials ([split][M][ldo])
    void  *out_act;  int ldo_act; // act-dtype output
    const float *bias;
    // EPI_RESID_F32: the residual stream the product is added to (may be out_f32 itself: every element is read and written by one thread)
    const float *resid; float resid_scale;
    // EPI_QKV
    float *q_out;                 // [M][1024] f32
    void  *kv_pool;               // K/V rings of this layer: [slot][2][KVC][1024] act dtype
    int64_t kv_slot_stride;       // elements between slots
    const RowDesc *rows;  int T;  // row m -> stream m / T, frame m % T
    // pipelined steps: this launch shares the chip with other launch chains' GEMMs -- the large-M kernels then use the variants
    // whose LDS ring lets two workgroups share a CU (same arithmetic in the same order: bit-identical to the default kernels)
    int coresident;       // 0: synchronous step, 1: pipelined step (the rule of nasr_gemm_plan.h decides), 2 / 3: always / never (engine option "gemm_cores")
    // wave priority of the co-resident kernels (round-4 probe, tests/micro/cores_probe.hip): bit 0 = s_setprio 3 for the whole kernel,
    // bit 1 = back to 0 before the epilogue.  0 = leave the default (what ships unless the probe says otherwise).
    // prio >> 2 (round 5, engine option "gemm_prio"): 0 = round 5's loops (k_gemm_wide2, k_gemm_tiled3), 5 = rounds 1-4's (k_gemm_wide, k_gemm_tiled2_k32): A/B runs and the identity test
    int prio;
    // f32 GEMMs above four rows run on the f32-input MFMA (k_gemm_f32_mfma); 1 = the FMA tile kernel k_gemm_f32 instead (engine
    // option "f32_mfma" = 0: the other side of the bit-identity test)
    int f32_fma_tile;
    // 1 = never the persistent tile loop (k_gemm_persist), whatever the size: engine option "persistent_gemm" = 0, the other side
    // of its bit-identity test
    int no_persist;
    // 1 = never the 256-row tiles (k_gemm_wide): engine option "wide_tiles" = 0, the other side of their bit-identity test
    int no_wide;
    // 256 = of the wide tiles only the 256-row form (engine option "wide_tiles" = 256: A/B against the 224-row form); 2 = not the pipelined steps'
    // tile-count rule ("wide_tiles" = 3); 0 = the launcher's rule
    int wide_rows;
    // tile order of the LDS-tiled bf16 kernels (tile_of(), kernels_gemm.hip): 0 = bands of column groups above 4 row chunks, 1 = always,
    // 2 = never (the row chunk fastest; engine option "tile_bands" = 0: the order of rounds 1-3)
    int tile_bands;
    // engine option "t64_tiles" + 1 (0 = the default, 64): the split-K GEMMs with N = 1024 take 128 x 64 tiles up to this many 128 x 128 tiles
    int t64_tiles_p1;
    int wide_min_tiles;   // pipelined steps: 224 x 256 tiles from this many of them (0 = 32)
    int wide_min_rows;    // ... and from this many rows (0 = 1 344)
    int narrow_stores;    // 1: four columns per thread in every epilogue (engine option "epilogue16" = 0: rounds 1-4's 8-byte stores of the 16-bit outputs)
    ChainParams chain;
#ifdef NASR_GEMM_STAMPS
    unsigned long long *stamps;   // tests/micro/prio_probe.hip only (its own compile of kernels_gemm.hip): per workgroup 8 values, see k_gemm_wide2
#endif
};

// ---- kernel launchers (defined in the .hip files) -----------------------------------
void init_gemm_kernel_attributes();    // one-time hipFuncSetAttribute calls (never inside a stream capture)
void init_fused_kernel_attributes();
void launch_gemm_bf16(const GemmParams &p, hipStream_t st);      // the kernel it takes and the rules its callers ask (gemm_chain_ok, gemm_resid_foldable, ...): nasr_gemm_plan.h
void launch_gemm_f32(const GemmParams &p, hipStream_t st);
void launch_pack_weight_bf16(const float *w_f32, bf16_t *packed, int N, int K, hipStream_t st);
void launch_f32_to_bf16(const float *in, bf16_t *out, int64_t n, hipStream_t st);

struct MelParams {
    const PcmDesc *desc; int B; int max_frames;
    float *abuf;          // [slot][2][ABUF_CAP]
    float *last_sample;   // [slot]
    float *mel_ring;      // [slot][MEL_RING][128]
    const float *window;  // [512] padded Hann
    const float *fbT;     // [257][128] transposed filterbank
    const int *fb_band;   // [128][2] first / one-past-last bin with a non-zero weight of every filter
    const float *cos_t, *sin_t;  // [512]
    float *tap; int tap_cap;     // optional debug copy of produced frames [B][tap_cap][128]
};
void launch_mel(const MelParams &p, int max_n, hipStream_t st);
void launch_mel_put(const float *staged, const PcmDesc *desc, int B, int max_frames, float *mel_ring, hipStream_t st);
void launch_mel_zero(const PcmDesc *desc, int B, int max_frames, float *mel_ring, hipStream_t st);
struct StreamResetParams {      // one launch per stream start / reset (kernels_front.hip: k_stream_reset)
    float *const *cc_pools;     // device array [n_layers] of the layers' conv-cache pools
    void *const *kv_pools;      // device array [n_layers] of the layers' K/V ring pools ([slot][2][KVC][1024], esz bytes per element)
    int esz, kv_head;           // element size of the rings; ring index of logical key 0 (the 70 window rows from there are zeroed)
    int n_layers, slot;
    int cc_slot_floats;         // 2 * (ks - 1) * 1024
    int keep_reference_state;   // NASR_RESET_REFERENCE: conv caches, audio-buffer carry and last_sample survive
    float *abuf, *last_sample, *mel_ring, *dec_h, *dec_c;
    DecCtrl *ctrl;
    int *boost_state; int boost_init;   // engine option "phrase_boost" (null when off): the slot's automaton state goes back to the root (or 0 = disabled)
    int32_t *lm_state; const nasr_lm::Greedy *lm_blk; int lm_enabled;   // engine option "lm_fusion" (null when off): the slot's LM state goes back to the model's start (or disabled)
    float *aud_hist;            // [slot][2][nasr_rs::HIST_MAX] input history of the audio converter: cleared in both modes
};
void launch_stream_reset(const StreamResetParams &p, hipStream_t st);
// one launch per stream fork (kernels_front.hip: k_stream_fork): workgroup i moves piece i of the copy plan (nasr_fork_plan.h).  A piece whose
// addresses and length are multiples of 16 moves as 16-byte vectors, any other as 4-byte words; the pieces of a launch are disjoint
struct StreamForkPiece { const char *src; char *dst; uint32_t bytes, pad; };
struct StreamForkParams { const StreamForkPiece *pieces; int n_pieces; };
void launch_stream_fork(const StreamForkParams &p, hipStream_t st);
// k_stream_pack / k_stream_unpack (nasr_snapshot.h): the pieces as above with pad = the index of the piece's first word in the device section;
// sums[i] = the checksum partial of piece i
struct StreamPackParams { const StreamForkPiece *pieces; int n_pieces; unsigned long long *sums; };
void launch_stream_pack(const StreamPackParams &p, hipStream_t st);
void launch_stream_unpack(const StreamPackParams &p, hipStream_t st);

// audio input conversion (kernels_audio.hip, nasr_resample.h): one per stream of a launch
struct AudioDesc {
    const void *in;             // the push: n_push interleaved input frames (device memory)
    const float *table;         // coefficients of the stream's rate, c[j + half]
    int16_t *out;               // n_out samples at 16 kHz: outputs out_first .. out_first + n_out - 1 of the stream
    float *hist;                // the slot's [2][nasr_rs::HIST_MAX], or null: nothing before the push, no history kept
    long long n_before, n_push; // input frames taken before this launch / in it
    long long out_first, n_out;
    int enc, channels, channel; // nasr_rs::ENC_*, 1 .. 8, channel index or -1 = mean
    int L, M, half, par;        // par: parity of hist that holds the frames before the push (the launch writes the other)
    int lds_table;              // 1: the workgroup copies the table into LDS first (only where 2 half + 1 <= LDS_TABLE_MAX)
};
constexpr int LDS_TABLE_MAX = 256;
void launch_audio_convert(const AudioDesc *descs, int B, long long max_out, hipStream_t st);

void launch_sub_conv0_dw(const RowDesc *rows, int B, int chunk_mel, const float *mel_ring, const float *w0t, const float *b0,
                         const float *w2t, const float *b2, void *out, int out_bf16, int H1, int W1, hipStream_t st);
void launch_sub_dw(const float *in, int B, int Hin, int Win, const float *wt, const float *bias, void *out,
                   int out_bf16, hipStream_t st);

void launch_post(const PostParams &p, hipStream_t st);

struct AttnParams {
    const float *q;       // [M][1024]
    const void *kv_pool; int64_t kv_slot_stride; int act_bf16;
    const void *posproj;  // [n_rel][1024] act dtype, row r <-> rel = (70+T-1) - r
    const float *bias_u, *bias_v;  // [8][128]
    const RowDesc *rows; int B; int T;
    int TS;               // rows per stream in this launch = G*T when G chunks of a stream are batched (0: = T)
    void *ctx_out;        // [M][1024] act dtype
    int ablate;           // measurement only (engine option "ablate" bits 64 / 128): k_attention_mfma without its V^T LDS writes / without its K and position loads
};
void launch_attention(const AttnParams &p, hipStream_t st);

struct ConvParams {
    const float *glu;     // [M][1024] f32
    float *cc_pool; int64_t cc_slot_stride;  // [slot][2][ks-1][1024] (this layer)
    const float *dw;      // [ks][1024]
    const float *ln_w, *ln_b;
    const RowDesc *rows; int B; int T; int ks;
    void *c_out; int act_bf16;
    int stream_form;      // 1: one workgroup per stream where the shape allows (k_dwconv_stream; engine option "dwconv_stream", same bits)
};
void launch_dwconv(const ConvParams &p, hipStream_t st);

struct DecParams {
    const RowDesc *rows; int B; int T;
    DecCtrl *ctrl;               // [slot]
    float *h, *c;                // [slot][2 versions][2 layers][640]
    const float *encproj;        // [M][640]  (joint.enc applied, bias included)
    const float *embed;          // [1025][640]
    const float *w_ih[2], *w_hh[2], *b_ih[2], *b_hh[2];
    const float *pred_w, *pred_b, *out_w, *out_b;
    float *predg;                // [slot][640]  joint.pred(h1') + b_pred of the current LSTM candidate
    unsigned long long *key;     // [B * T] packed argmax keys, one per (row, frame)
    int *n_active;               // device counters: streams with frames left,
    int *n_dirty;                //   entries of dlist,
    int *n_rows;                 //   entries of rowmap
    int *dlist;                  // [B] batch rows whose LSTM candidate must be recomputed
    unsigned *rowmap;            // [B * T] (frame << 16 | batch row) of every frame still to decode
    int *tok_ring;               // [slot][TOK_CAP]
    int *tok_frame;              // [slot][TOK_CAP] absolute encoder frame of each token
    // engine option "token_logprobs" (both null when it is off: the launches are then the kernels without it)
    nasr_lp::Part *lp_part;            // [B * T][n_parts] (max, sum of exp(x - max)) of every vocab slice of every evaluated row (nasr_logprob.h)
    float *tok_logprob;          // [slot][TOK_CAP] natural-log softmax probability of each token where it was emitted
    // engine option "phrase_boost" (all null when it is off), nasr_boost.h
    const float *boost_bonus;    // [states][1040] bonus of every vocabulary entry in every automaton state
    const int32_t *boost_next;   // [states][1040] state after emitting that entry
    int *boost_state;            // [slot] automaton state of the slot's emitted history (0: boosting disabled for it, 1: root)
    float *boost_raw;            // [B * T][n_parts] with "token_logprobs" too: raw logit of every part's winner by boosted key
    float *raw_logits;           // [B * T][1040] the boosted beam evaluation only (launch_decode_rows_boost): every row's raw logits
    // engine option "token_alternatives" = alt_k (all null / 0 when it is off), nasr_topk.h; these variants always leave the softmax parts too,
    // so lp_part and tok_logprob are set with them
    unsigned long long *alt_key; // [B * T][n_parts][alt_k] the alt_k largest raw-logit keys of every vocab slice of every evaluated row
    int32_t *alt_id;             // [slot][TOK_CAP][alt_k] ids of the alt_k largest joint outputs where each token was emitted, descending
    float *alt_lp;               // [slot][TOK_CAP][alt_k] their natural-log softmax probabilities
    int alt_k;
    // engine option "frame_blank_logprobs" (both null when it is off; lp_part and the LP kernels come with it)
    float *fb_row;               // [B * T] indexed like key: ln P(blank) of every row the iteration's joint kernel evaluated (k_dec_commit, FB)
    float *frame_blank;          // [slot][FRAME_CAP] ring by absolute frame number: the value at the last evaluation of every frame the decode has left
    // engine option "lm_fusion" (all null when it is off: the launches are then the ones without it), nasr_lm.h / DESIGN 17
    const nasr_lm::Greedy *lm_blk;   // the fixed block: the model's view and the greedy weights (rewritten by the setters, never moved)
    int32_t *lm_state;           // [slot] LM state of the slot's emitted history (nasr_lm::STATE_DISABLED: switched off)
    float *lm_row;               // [slot][1040] phrase bonus + lmbias of every vocabulary entry in the slot's states
    int32_t *lm_next;            // [slot][1040] LM state after emitting that entry
    int lm_fold;                 // 1: the rows are refreshed by extra workgroups of k_dec_pred, 0: by a launch of their own
    int lm_relook;               // measurement only: 1 = k_dec_commit looks the token up again instead of reading lm_next
    // engine option "token_entropy" (null / 0 when it is off; lp_part and the LP kernels come with it), nasr_entropy.h
    float *ent_part;             // [B * T][n_parts] beside lp_part: the entropy term of every vocab slice of every evaluated row
    float *tok_entropy;          // [slot][TOK_CAP] entropy of order ent_alpha (nats) of the joint's softmax where each token was emitted
    float ent_alpha;
};
// the bias rows of slots slot0 .. slot0 + n - 1 from their current states (boost_bonus / boost_state null without "phrase_boost")
void launch_lm_rows(const nasr_lm::Greedy *blk, const int32_t *lm_state, float *lm_row, int32_t *lm_next, const float *boost_bonus, const int *boost_state,
                    int slot0, int n, hipStream_t st);
void launch_decode_begin(const DecParams &p, hipStream_t st);
void launch_decode_iter(const DecParams &p, hipStream_t st);
int decode_blind_iterations(int frames);
void launch_encproj(const float *x, const float *wpk, const float *bias, float *out, int M, int K, int N, hipStream_t st);
// the LSTM candidate and g = joint.pred(h1') + b_pred of the rows in p.dlist (*p.n_dirty of them): the first three launches of launch_decode_iter
void launch_decode_candidates(const DecParams &p, hipStream_t st);

// ---- engine option "frame_history" (kernels_history.hip, nasr_history.h) ------------------------------------------------------------
// the append: one launch at the head of a step's decode sequence, right behind launch_decode_begin (DecCtrl::frame0 of the step is in force)
struct HistAppendParams {
    const RowDesc *rows; int B; int T;   // the decode's own descriptors: row (b, t) is encproj row b * T + t, valid while t < rows[b].n_dec
    const DecCtrl *ctrl;         // [slot]
    const float *encproj;        // [B * T][640]
    float *ring; int N; int slots;   // [slots][N][640]
    int wg_rows;                 // 0: the rule (one row per workgroup); 4: four rows per workgroup (measurement only, same bytes)
};
void launch_history_append(const HistAppendParams &p, hipStream_t st);
// the gather: frames [first, first + count) of slot's ring -> packed rows [out_row, out_row + count) (count <= N, the window kept: the host's check)
struct HistWindow { long long first; int slot, count, out_row, pad; };
void launch_history_gather(const HistWindow *win, int n, int max_count, const float *ring, int N, float *out, hipStream_t st);

// ---- forced alignment / transcript scoring on the RNN-T lattice (kernels_align.hip, nasr_align.h) ------------------------------
struct AlignPredParams {         // teacher forcing, step u: decoder slot k = utterance k of the sub-batch
    const nasr_align::Utt *utt; int n; int u;
    const int32_t *tok;          // the transcripts, utterance k at utt[k].tok0
    DecCtrl *ctrl; int *dlist; int *n_dirty;
    const float *predg;          // [slot][640] g of step u - 1
    float *g;                    // [sum (U + 1)][640]
};
void launch_align_pred_step(const AlignPredParams &p, hipStream_t st);
struct AlignParams {
    const nasr_align::Utt *utt;
    const nasr_align::Tile *tiles;   // the tiles of this launch, one workgroup each
    const float *encproj;        // [M][640] packed rows of the sub-batch
    const float *g;              // [sum (U + 1)][640]
    const int32_t *tok;
    const float *out_w, *out_b;  // the joint's output layer, packed as for the decode
    float *lp_blank, *lp_token;  // [cells]
};
void launch_align_lattice(const AlignParams &p, int n_tiles, hipStream_t st);
struct AlignRecParams {
    const nasr_align::Utt *utt;
    const float *lp_blank, *lp_token;
    unsigned char *bp;           // [cells] 1 = the best path enters the cell by a token move
    double *scores;              // [n][2] loglik, best
    int32_t *frames; float *tok_lp;   // [sum U]
};
void launch_align_recursion(const AlignRecParams &p, int n, hipStream_t st);

// ---- frame-synchronous beam search of the offline path (kernels_beam.hip, nasr_beam.h) ---------------------------------------------
// the evaluation of a round: launch_decode_candidates over p.dlist, then k_dec_joint_tiled in its LP + ALT form over p.rowmap whatever the
// row count (one kernel form, so a sub-batch gives the bits an utterance gives alone); no commit.  p.alt_k = 8, 17 parts per row
void launch_decode_rows(const DecParams &p, hipStream_t st);
// a boosted beam call (NASR_FLAG_BEAM_BOOST): the tiled joint's BEAMB form -- the lists by logit + bonus(state of the row's slot), the raw logits kept
void launch_decode_rows_boost(const DecParams &p, hipStream_t st);
struct BeamUtt { int enc_row, T; long long node0, out0; };      // first packed encoder row, frames, first node of its pool, first output entry
struct BeamParams {
    const BeamUtt *utt; int n;   // live utterances of the sub-batch, one workgroup each; hypothesis j of utterance k is batch row k * W + j
    int W, N, S, prune;
    nasr_beam::Beam *beam;       // [n]
    nasr_beam::Node *nodes;      // the pools, utterance k at utt[k].node0
    const float *encproj;        // [M][640] packed rows of the sub-batch
    float *enc;                  // [n * W][640] the current frame's row of every batch row (the joint's encproj, T = 1)
    RowDesc *rows;               // [n * W] the slot of every batch row
    DecCtrl *ctrl; float *h, *c; // [n * 3 W] decoder slots
    const nasr_lp::Part *lp_part; const unsigned long long *alt_key;   // what the joint left: [n * W][17], [n * W][17][8]
    int *cnt_next, *cnt_zero;    // (n_dirty, n_rows) of the next evaluation / of the one that just ran
    int *dlist; unsigned *rowmap;
    int *err;
    int32_t *out_n, *out_len; double *out_score;   // [n], [n][8], [n][8]
    int32_t *out_tok, *out_frame; float *out_lp;   // utterance k, rank r at utt[k].out0 + r * T * S
    // shallow fusion (nasr_engine_set_lm; lm_on = 0: none of this is read): the tables in device memory, the weights, the LM outputs
    int lm_on; float lm_weight, lm_bonus;
    nasr_lm::View lm;
    double *out_lm, *out_lm_final, *out_total;     // [n][8] each
    // phrase boosting (NASR_FLAG_BEAM_BOOST; boost_on = 0: none of this is read): the engine's tables, the beam's own per-slot automaton states
    // (the boosted joint form reads them), the raw logits it left, and the outputs.  With boost_on, out_total is written with or without an LM
    int boost_on;
    const float *boost_bonus; const int32_t *boost_next;
    int *boost_state;            // [n * 3 W]
    const float *raw_logits;     // [n * W][1040]
    double *out_boost;           // [n][8]
};
void launch_beam_init(const BeamParams &p, hipStream_t st);
void launch_beam_select(const BeamParams &p, hipStream_t st);
void launch_beam_final(const BeamParams &p, hipStream_t st);

// ---- fused small-M kernels (M <= 16): prologue + weight-streaming GEMM + epilogue in one launch ----
enum Pro { PRO_LN = 0, PRO_PLAIN = 1, PRO_ATTN = 2, PRO_DWCONV = 3 };
struct FusedParams {
    GemmParams g;                 // W (packed bf16), M, N, K, splits, epi + outputs (A unused unless PRO_PLAIN)
    int pro;
    // PRO_LN: a = LN( [LN_out]( x_in + scale * sum_s part[s] ) ); block (0,0) writes the updated x to x_out
    const float *x_in; float *x_out; const float *part; int part_splits; float scale;
    const float *lno_w, *lno_b;   // optional LayerNorm applied to the updated x first (norm_out of the previous layer)
    const float *ln_w, *ln_b;
    AttnParams at;                // PRO_ATTN (blockIdx.y = head; K range = that head's 128 columns)
    ConvParams cv;                // PRO_DWCONV
#ifdef NASR_STAMPS
    unsigned long long *stamps;   // diagnostic build: [launch slot][2 blocks][16] s_memrealtime values (10 ns ticks)
#endif
};
void launch_fused_skinny(const FusedParams &p, hipStream_t st);
constexpr int FUSED_GROUP = 4;
struct FusedParamsGroup { FusedParams p[FUSED_GROUP]; };
void launch_fused_skinny_group(const FusedParamsGroup &pp, int n, hipStream_t st);   // n problems of one kind, M <= 2; g.M == 0: skipped

void launch_prompt_add_relu(float *h, const float *w1p, const RowDesc *rows, int M, int T, int P, hipStream_t st);
void launch_relu(float *x, int64_t n, hipStream_t st);
void launch_fill_f32(float *p, float v, int64_t n, hipStream_t st);

// bf16 helpers -------------------------------------------------------------------------
__device__ __forceinline__ float bf16_to_f32(bf16_t v) {
    return __uint_as_float(((uint32_t)v) << 16);
}
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {   // RNE; NaN kept NaN
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((u >> 16) | 0x40);
    return (bf16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}


// ---- diarization side-car (reference src/diarize_{audio,vad,spk}.cpp) -----------------
constexpr int DIAR_NMEL = 80;
constexpr int VAD_WINDOW = 10080, VAD_T = 64, VAD_TVALID = 63;      // src/diarize_vad.h:86-89
constexpr int SPK_SEGMENT = 24000, SPK_T = 160, SPK_TVALID = 150;   // src/diarize_spk.h:102-104
constexpr int SPK_EMB = 192, SPK_C = 3072, SPK_ATT = 128;

struct DiarMelParams {            // one workgroup per (frame, window)
    const float *audio;           // all windows index into this buffer ...
    const int16_t *audio_s16;     // ... or into this one (s16 PCM, sample / 32768: the ASR stream's own buffers), if not null
    const long long *win_off;     // [W] sample offset of every window
    int n_win;                    // samples per window (10080 / 24000)
    int T_pad, t_valid;           // frames written per window (64 / 160), of which valid (63 / 150)
    int cpitch;                   // channel pitch of the output rows (80, or 96 = zero padded for the K % 32 GEMM)
    float *mel;                   // [W][T_pad][cpitch]
    const float *window;          // [512] padded Hann
    const float *fbT;             // [257][80]
    const int *fb_band;           // [80][2]
    const float *cos_t, *sin_t;   // [512]
};
void launch_diar_logmel(const DiarMelParams &p, int W, bool per_feature_normalize, hipStream_t st);
// single frames: frame f = local frame `t` of the window [base, base + n) of the staged audio -> out[f][80]
struct DiarFrameDesc { long long base; int n; int t; };
void launch_diar_frames(const DiarMelParams &p, const DiarFrameDesc *frames, int n_frames, float *out, hipStream_t st);

struct VadSub { const float *dw, *pw, *scale, *bias; int kernel, dil, cin, cout; const bf16_t *pw16; };   // dw == nullptr: pointwise only; pw16: bf16 / half fragment tiles (NASR_DIAR_VAD_BF16 / _F16), else null
struct VadNet {                   // MarbleNet, src/diarize_vad.cpp:25-32: 6 blocks, 9 sub-convs, 3 residual paths
    VadSub sub[9];
    VadSub res[3];                // blocks 1..3
    const float *dec_w, *dec_b;   // [2][128], [2]
};
// one workgroup per window -> P(speech) [W]; lens_mel [W] valid frames (masked convs).  The 64 mel rows of window w:
// rows 2..61 = shared[win_row[w].x + t] (frames that overlapping windows have in common, computed once per stream),
// rows 0, 1, 62 = edge[3 w + {0, 1, 2}] (they see the window's own zero padding / pre-emphasis start), row 63 = 0
void launch_vad_marblenet(const VadNet &net, const float *shared, const float *edge, const int *win_row, const int *lens_mel,
                          float *prob, int W, hipStream_t st);
void launch_vad_marblenet_bf16(const VadNet &net, const float *shared, const float *edge, const int *win_row, const int *lens_mel,
                               float *prob, int W, hipStream_t st);       // the same network on the bf16 MFMA, bf16 activation planes
void launch_vad_marblenet_f16(const VadNet &net, const float *shared, const float *edge, const int *win_row, const int *lens_mel,
                              float *prob, int W, hipStream_t st);        // ... on the f16 MFMA, IEEE-half planes (pw16 = half tiles)
void init_diar_kernel_attributes();

// TitaNet-L on segment tiles (round 6, kernels_spk.hip; the bf16 engine's path): the pointwise convs as GEMMs whose tile is ONE sub-segment
// (160 rows) x 256 channels, with what follows the conv along the time axis done in the epilogue while the tile is in LDS
enum { SG_DW = 0, SG_Y = 1, SG_RES = 2, SG_ASP = 3 };
struct SpkGemmParams {
    const bf16_t *A; int lda;        // [S * 160][lda] bf16, rows >= lens masked to zero by whoever wrote them
    const bf16_t *W;                 // packed 16 x 32 tiles [N / 16][K / 32] (launch_pack_weight_bf16), folded BN scale inside
    int S, N, K, mode;
    const float *bias;               // [N] folded BN bias / conv bias
    const int *lens;                 // [S] valid frames
    const float *dw_w; int dw_k;     // SG_DW / SG_RES: taps [dw_k][N] of the NEXT depthwise conv (SG_RES: dw_k <= 1 = none)
    bf16_t *a_out; int lda_out;      // ... its output = the next GEMM's A operand
    float *y_out, *colmean;          // SG_Y: [S * 160][N] f32, [S][N] masked mean over time (SE gate input)
    const float *y_in, *z;           // SG_RES: Y of the block, SE gate pre-activation [S][N]
    bf16_t *x_out;                   // SG_RES: the block's output, masked, [S * 160][N]
    const bf16_t *x_in;              // SG_ASP: encoder output [S * 160][N]
    const float *bn_s, *bn_b; float *pool;   // SG_ASP: folded BN of the embedding layer [2 N], pool [S][2 N]
#ifdef SG_STAMPS
    unsigned long long *stamps;      // diagnostic build (tests/micro/spk_gemm_probe.hip): 8 real-time stamps (100 MHz) per workgroup
#endif
};
int launch_spk_gemm(const SpkGemmParams &p, hipStream_t st);      // -1: operands the kernel's indexing does not cover (nothing launched)
const char *spk_gemm_check(const SpkGemmParams &p);
enum { ST_DW = 0, ST_STATS = 1 };
struct SpkTileParams {               // relu(mask(Y) * sigmoid(z)) of a block without residual -> X bf16, then the next depthwise conv or the masked statistics
    const float *y_in, *z; const int *lens; int S, C, mode;
    bf16_t *x_out;
    const float *dw_w; int dw_k; bf16_t *a_out; int lda_out;
    float *mean, *stdv; int stat_ld;     // ST_STATS: [S][stat_ld] each (the two may be halves of one [S][2 C] buffer: stat_ld = 2 C)
};
int launch_spk_tile(const SpkTileParams &p, hipStream_t st);
void init_spk_kernel_attributes();
struct GatherDesc { const void *src; long long dst_off, bytes; };          // bytes: a multiple of 2 (s16 or f32 samples)
void launch_gather_audio(const GatherDesc *tab_dev, int B, long long max_bytes, char *dst, hipStream_t st);
// per-feature normalisation + block 0's depthwise conv (k = 3): log-mel [S][160][cpitch] -> bf16 A operand [S * 160][lda_out >= 128]
int launch_spk_front(const float *mel, int cpitch, const float *dw_w, const int *lens, bf16_t *a_out, int lda_out, int S, hipStream_t st);
// out[m][n] = W[n] . x[m] + b[n] (optional ReLU) for a few rows and long K: f32 MFMA, weights in pack_mfma_f32 order, K split over workgroups
int spk_fc_slices(int M, int K, int N);
int launch_spk_fc(const float *x, int ldx, const float *wpk, const float *bias, float *out, float *part, int M, int K, int N, int relu, hipStream_t st);

// TitaNet-L pieces (src/diarize_spk.cpp:320-515); activations [S * 160][C] f32, channels innermost
void launch_spk_depthwise(const float *x, int x_pitch, const float *w, int kernel, int C, int Cpad, const int *lens, float *a_out,
                          int S, hipStream_t st);                             // masked 'same' depthwise conv -> GEMM A operand (f32 engine)
void launch_spk_mask_cvt(const float *x, int C, const int *lens, float *a_out, int S, hipStream_t st);
void launch_spk_colmean(const float *y, int C, const int *lens, float *mean, int S, hipStream_t st);   // masked mean over time (SE)
void launch_spk_combine(const float *y, const float *z, const float *r, int C, const int *lens, float *out, int S, hipStream_t st);
void launch_spk_stats(const float *x, int C, const int *lens, float *mean, float *stdv, int S, hipStream_t st);
void launch_spk_att_const(const float *mean, const float *stdv, const float *w1, const float *b1, float *c, int C, int A, int S, hipStream_t st);
void launch_spk_att_post(const float *g, const float *c, const float *bn_scale, const float *bn_bias, void *a_out, int out_bf16,
                         int A, int S, hipStream_t st);
void launch_spk_asp(const float *x, const float *logits, int C, const int *lens, const float *bn_scale, const float *bn_bias,
                    float *pool, int S, hipStream_t st);
int set_error(const char *msg);      // fills nasr_last_error() of the calling thread, returns -1

// ---- streams an engine has lent to another client of the library (nasr_engine_lend_stream -> nasr_diar_set_stream) ----------------
// Round-2 advisor / round-3 verdict: the engine owns a lent stream and destroyed it in nasr_engine_destroy whatever the borrower was
// doing.  The library now counts borrowers: an engine that goes first says so loudly (stderr + nasr_last_error) and leaves the stream
// to its borrowers -- the last one to let go destroys it.  Nothing dangles in either order.
void lent_stream_register(hipStream_t s);        // the engine lends s
bool lent_stream_acquire(hipStream_t s);         // a borrower starts using s (false: not a lent stream, the caller's own)
void lent_stream_release(hipStream_t s);         // a borrower is done with s; destroys s if its engine is gone and nobody else holds it
int  lent_stream_engine_gone(hipStream_t s);     // the lender is being destroyed: borrowers still holding s (0: the engine destroys s itself)


}  // namespace nasr
