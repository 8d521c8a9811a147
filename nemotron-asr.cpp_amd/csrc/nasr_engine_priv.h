// nasr_engine_priv.h -- what the translation units of the engine share (round 4: nasr_engine.hip was 2 900 lines holding pools, step
// driver, pipeline, graph cache and ABI).  nasr_engine.hip = weights, pools, engine / stream life cycle; nasr_encoder.hip = the
// chunk step (encoder + decode launch sequences); nasr_pipeline.hip = hipGraph steps, lanes, pipelined and grouped steps;
// nasr_abi.hip = the step driver and the remaining entry points of include/nemotron_asr_amd.h.  Internal functions live in
// namespace nasr_eng (nothing but the extern "C" ABI is meant to be bound from outside).  The host arithmetic of a push is
// nasr_step_plan.h (pure: namespace nasr_step); what the synchronous, pipelined and grouped graph steps share around their launches
// is declared below: fill_step_descs, mirror_step, finish_step_decode, decode_until_idle, gp_capture, capture_decode_graph,
// step_mel_params, lru_victim; the staging helpers grow_device and PinBlock.
#pragma once
#include "nasr_internal.h"
#include "nasr_decode_set.h"
#include "nasr_step_plan.h"
#include "nasr_fork_plan.h"
#include "nasr_snapshot.h"
#include "nemotron_asr_amd.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <shared_mutex>
#include <string>
#include <vector>

using namespace nasr;
using namespace nasr_step;

namespace nasr_eng {
int fail(const char *fmt, ...);                 // fills nasr_last_error() of the calling thread, returns -1
}
using namespace nasr_eng;
#define HIPCHK(x)                                                                           \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Several engines may live in one process, one host thread each (the socket server: one lane per GPU).  HIP stream
// capture, even in thread-local mode, is broken by what other threads do meanwhile ("operation failed due to a
// previous error during capture" when another thread copies or allocates).  Every entry point that talks to HIP
// therefore holds this lock shared; building a step graph (rare: once per (B, T, G)) takes it exclusively.
void api_lock_shared();                          // also used by nasr_diar.hip
void api_unlock_shared();
namespace nasr_eng {
void api_capture_begin();                        // shared -> exclusive (the caller is inside an ApiGuard)
void api_capture_end();
struct ApiGuard {
    ApiGuard() { api_lock_shared(); }
    ~ApiGuard() { api_unlock_shared(); }
};
struct CaptureExclusive {       // held by a thread that is inside an ApiGuard
    CaptureExclusive() { api_capture_begin(); }
    ~CaptureExclusive() { api_capture_end(); }
};
#ifdef NASR_STAMPS
extern unsigned long long *g_stamp_buf;
extern int g_stamp_pipe;
constexpr int STAMP_PER_SLOT = 8 * 24, STAMP_SLOTS = 5;
#endif
}  // namespace nasr_eng

// ---------------------------------------------------------------------------------------
struct nasr_engine;
struct OfflineState;                 // nasr_offline_state.h: buffers of the offline path, allocated on its first call
namespace nasr_eng {
void prof_flush(nasr_engine *e);
void offline_destroy(nasr_engine *e);
}
struct LayerW {
    float *ln_ff1_w, *ln_ff1_b, *ln_att_w, *ln_att_b, *ln_conv_w, *ln_conv_b, *ln_ff2_w, *ln_ff2_b, *ln_out_w, *ln_out_b;
    void *ff1_w1, *ff1_w2, *wqkv, *wo, *pw1, *pw2, *ff2_w1, *ff2_w2;   // packed bf16 or f32 [N][K]
    float *wpos_f32;                                                    // [1024][1024] f32 (load-time pos projection)
    float *bias_u, *bias_v, *dw, *cln_w, *cln_b;
    void *posproj[TMAX + 1];                                            // per T: [70+2T-1][1024] act dtype
};

struct Prof {
    struct Rec { int cat; hipEvent_t a, b; double bytes, flops; };
    bool on = false;
    std::vector<std::string> names;
    std::vector<nasr_kernel_stat> stats;
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    int cat(const char *n) {
        for (size_t i = 0; i < names.size(); i++) if (names[i] == n) return (int)i;
        names.push_back(n);
        nasr_kernel_stat s;
        memset(&s, 0, sizeof(s));
        snprintf(s.name, sizeof(s.name), "%s", n);
        stats.push_back(s);
        return (int)names.size() - 1;
    }
};

// A stream is the record of what it is (nasr_snap::Mirror: the host mirror of the stream manager state, reference nemo_stream_context --
// the one declaration create, reset, fork, save and restore share) plus what is not state
struct nasr_stream : nasr_snap::Mirror {
    nasr_engine *e = nullptr;
    int slot = 0, T = 1;                           // T = 1 + R
    int last_T = 0, last_row = 0, last_ws = 0;     // rows of the last chunk and the workspace set they are in (for taps)
    bool alive = false;
    // engine option "frame_history": the first frame this stream may show of its slot's ring (nasr_hist::retained).  0 from create and both
    // resets; a fork and a restored stream start at the frames their source had decoded -- the history does not travel, so it is not part
    // of the record above
    int64_t hist_valid_from = 0;
    // audio input conversion (nasr_resample.h): recomputed from the record's format by nasr_stream_set_audio_format and a restore
    nasr_rs::Plan aud_plan = {16000, 1, 1, 0, 1};
    const float *aud_table = nullptr;              // device coefficients of sample_rate (the engine's cache owns them)
    nasr_audio_format fmt() const { return {sample_rate, encoding, channels, channel}; }
};
static_assert(NASR_AUDIO_S16 == 0, "Mirror::default_format");

// A rotating pinned block of a host hand-over: the streams' buffers are gathered into it and cross PCIe as ONE asynchronous copy.  A block
// is reused four calls later, so its last copy must have been executed by then (the grouped pipeline keeps eight calls in flight and
// nothing else orders the host's memcpy behind copy n - 4; in steady state the event is long complete).
struct PinBlock {
    char *p = nullptr; size_t cap = 0; hipEvent_t copied = nullptr; bool pending = false;   // copied: recorded behind the block's H2D copy
    int acquire(size_t bytes, size_t slack, hipStream_t st);      // waits for the block's last copy; grows it (with slack) behind st
    int copy_to(void *dev, size_t bytes, hipStream_t st);         // p -> dev on st, and the event behind it
};

struct nasr_engine {
    int device = 0, dtype = 0, max_streams = 0;
    nasr_hparams hp;
    bool bf16 = false;
    int esz = 4;
    hipStream_t st = nullptr;
    // front-end constants
    float *window = nullptr, *fbT = nullptr, *cos_t = nullptr, *sin_t = nullptr;
    int *fb_band = nullptr;
    float *w0t, *b0, *w2t, *b2, *b3, *w5t, *b5, *b6, *sub_out_b;
    void *w3, *w6, *sub_out_w;
    std::vector<LayerW> L;
    float *embed, *w_ih[2], *w_hh[2], *b_ih[2], *b_hh[2], *jenc_w, *jenc_b, *pred_w, *pred_b, *out_w, *out_b;
    float *pk1a = nullptr, *pk1p = nullptr, *pk1_b = nullptr, *pk2_w = nullptr, *pk2_b = nullptr;
    // state pools
    float *abuf, *last_sample, *mel_ring;
    std::vector<void *> kv_pool;     // per layer [slot][2][KVC][1024] act dtype
    std::vector<float *> cc_pool;    // per layer [slot][2][ks-1][1024]
    float **cc_ptrs_dev = nullptr;   // device copy of cc_pool (k_stream_reset walks the layers in one launch)
    void **kv_ptrs_dev = nullptr;    // device copy of kv_pool (same launch: the 70 window rows of a starting stream are zeroed)
    DecodeSet dec;                   // the greedy decode's working set (nasr_decode_set.h), max_streams slots x w_rows rows: engine_create and the decode options fill it (ensure_decode_set)
    // workspace (sized for max_streams x TMAX rows)
    float *x, *x2, *part, *q, *glu, *encproj, *sub_a, *hfuse;
    bool opt_fused = true, opt_graph = true;
    int opt_graph_cache = 16;        // option "graph_cache": step shapes (B, T, G, E) whose hipGraphs are kept, per slot; least recently used goes first
    std::map<int64_t, int64_t> graph_used;   // shape key -> tick of its last use
    int64_t graph_tick = 0, graph_evictions = 0;
    int64_t stream_forks = 0, stream_previews = 0;   // k_stream_fork launches (nasr_stream_fork and the forks of a preview) / nasr_engine_preview calls (counters of the same names)
    // stream snapshots (nasr_snapshot.h): the device staging buffer of k_stream_pack / k_stream_unpack (payload + checksum partials; allocated
    // by the first save or restore, sized by the snapshot bound) and the pinned block it crosses PCIe through; the fingerprints a blob carries
    char *snap_stage = nullptr; size_t snap_stage_cap = 0;
    PinBlock snap_pin;
    int64_t stream_saves = 0, stream_restores = 0;   // counters of the same names
    uint64_t fp_weights = 0;         // of the weight set, taken at nasr_engine_create (names, types, shapes, a bounded sample of the bytes)
    uint64_t boost_fp = 0, lm_fp = 0;   // of the boost set's tables (every nasr_engine_set_boost_phrases) / the n-gram model's tables (nasr_engine_set_lm)
    int opt_fork_piece_kb = 0;       // option "fork_piece_kb" (MEASUREMENT ONLY): KiB one workgroup of k_stream_fork moves at most; 0 = nasr_fork::PIECE_BYTES
    // hipGraph replay of the steady-state step: fixed descriptor buffers + one exec per (B, T)
    std::map<int64_t, hipGraphExec_t> graphs;
    int w_rows = 0;                  // workspace rows = max(max_streams x TMAX, MAXNEW)
    char *g_desc = nullptr;          // device mirror of the packed descriptor block (layout: graph_desc_layout)
    bool opt_multichunk = true;
    int opt_decode_graph_iters = 0;    // blind decode iterations a pipelined step's decode graph carries at most (option "decode_graph_iterations"); 0 = auto (nasr_step::pipe_decode_iterations)
    int opt_fused_cuts = 0;            // option "fused_cuts" (MEASUREMENT ONLY): the four-piece lane cut of the fused family, three launch indices of a 24-layer model in 10 bits each; 0 = nasr_step::FUSED_CUT4
    bool opt_decode_lane = true;       // the decode graphs get a lane of their own when a queue is free (option "decode_lane")
    int opt_gemm_cores = -1;           // -1: the engine's rule; 0 / 1: never / always the GEMM kernels of which two share a CU (option "gemm_cores")
    int opt_large_step_rows = 0;     // option "large_step_rows": the row count from which "large_step_pieces" applies (0 = the default of 5 600; round 4: 3 584)
    int opt_large_step_pieces = 3;   // option "large_step_pieces": most pieces of a pipelined step of 5 600 rows and more (0 = as many as "pipeline" says)
    int opt_t64_tiles = 64;          // option "t64_tiles": the split-K GEMMs with N = 1024 take 128 x 64 tiles up to this many 128 x 128 tiles (per engine, carried in GemmParams)
    int opt_tile_bands = -1;         // option "tile_bands": -1 = the rule (bands of column groups above 4 row chunks), 0 = never, 1 = always (same bits)
    int opt_wide_tiles = 1;          // option "wide_tiles": 256- / 224-row GEMM tiles from 1 792 rows where they fill the chip (k_gemm_wide; same bits); 256 = the 256-row form only, 0 = off
    bool opt_persist_gemm = false;   // option "persistent_gemm" = 1: GEMMs with >= 1.75 tiles of 128 x 128 per CU on the persistent tile loop (k_gemm_persist; same bits).  Off by default: alone on the chip with cache-resident operands it is 14-37 % faster at 7 168 rows, inside the engine (weights cold from HBM) 1 % -- profiles/r4_persistent_gemm.md
    int opt_wide_min_tiles = 0;      // option "wide_min_tiles": pipelined steps take the 224 x 256 tiles from this many tiles (0 = the default of 32)
    int opt_wide_min_rows = 0;       // option "wide_min_rows": ... and from this many rows (0 = the default of 1 344)
    int opt_gemm_prio = 0;           // option "gemm_prio": GemmParams::prio (probes of wave priority in the GEMM loops)
    bool opt_epilogue16 = true;      // option "epilogue16": SiLU rows, K / V ring rows and GLU pairs leave the GEMM epilogues as 16-byte stores (eight columns per thread; same values)
    bool opt_dwconv_stream = true;   // option "dwconv_stream": the depthwise conv with one workgroup per stream from 256 streams x 4 frames (k_dwconv_stream; same bits)
    int opt_chain = 0;               // option "chain" (OFF: measured 23 % SLOWER, profiles/r5_configs2_launch_structure.md section 3): 1 = in pipelined steps of 769 .. 1 343 rows the GEMM that reads a k_post's
                                     // rows carries that k_post as its head phase (GemmParams::chain: one launch fewer per LayerNorm, same bits); 2 = in synchronous steps too
    int opt_split_tasks = 0;         // option "split_tasks": residual GEMMs take ONE K slice from this many 128 x 128 output tiles (0 = the rule, 200; A/B runs)
    int opt_resid_epilogue = 1;       // option "resid_epilogue": residual GEMMs add to the residual stream in their own epilogue where one workgroup owns a tile's whole K sum
                                     // (k_gemm_t64w / launches without split-K): 1 = in pipelined steps (default), 2 = always, 0 = partial slabs + k_post everywhere (rounds 1-4); same bits
    int opt_ablate = 0;              // option "ablate" (MEASUREMENT ONLY, results are invalid): bit mask of launches left out of the unfused step -- 1 k_post, 2 attention,
                                     // 4 depthwise conv, 8 decode iterations, 16 front end (mel + subsampling), 32 every encoder GEMM: what each costs a pipelined step (profiles/r5_configs2_launch_structure.md, r5_ablation_b64_R13.json)
    bool opt_f32_mfma = true;        // f32 GEMMs above four rows on v_mfma_f32_32x32x2_f32 (bit-identical to the FMA tile kernel)
    char *gh = nullptr;                                                               // pinned host block
    int *gh_collect = nullptr;       // pinned landing zone of the token gather: [B][1 + COLLECT_STRIDE] + n_active
    int64_t graph_replays = 0, eager_steps = 0, decode_fallbacks = 0, decode_fallback_rounds = 0;
    // pipelined graph steps (option "pipeline" = E, 1..4): launch sequences of CONSECUTIVE steps run beside each other on
    // their own HIP streams -- see the comment at pipe_step().  Everything a step in flight owns exists once per slot:
    // workspace set, descriptor blocks, joint.enc buffer, token landing zone, graphs (their kernel arguments point into
    // the slot).  E + 1 steps are in flight; slot of a step = its sequence number mod NSLOT.
    static const int MAXSEG = 4, LSLOT = MAXSEG + 1;     // lanes mode: E + 1 steps in flight, slot = sequence number mod LSLOT
    int pipe_last_cut = 0;           // cut identity of the youngest step in flight: its piece count and its family (pipe_cut_id; pipe_step drains before a step that is cut differently)
    int64_t cut_drains = 0;          // ... and how often it had to (counter "cut_drains")
    static const int GP_C = 2, GP_Y = FUSED_GROUP, GP_S = GP_C * GP_Y;   // grouped mode ("pipeline" = 8): 2 chains x 4 problems per launch = 8 stages
    static const int NSLOT = GP_S + 3;                    // grouped mode: 8 steps in flight + the one being decoded + the one being collected + one spare
    struct WS { float *x, *x2, *part, *q, *glu, *sub_a, *hfuse; void *a, *hbuf, *ctx, *cbuf, *sub_b; unsigned *chain_flags; };
    WS ws[NSLOT];                    // ws[0] = the set the synchronous paths use (mirrored in x, x2, ... below)
    int opt_pipeline = 0;            // 0: synchronous steps; E >= 1: the encoder in E pieces + the decode, each piece one step behind the previous
    hipStream_t lane[MAXSEG] = {nullptr, nullptr, nullptr, nullptr};   // lane[k]: encoder piece k (lane[0] = st)
    int n_lanes = 1;                 // streams that run side by side (lane[0 .. n_lanes - 1], each on a hardware queue of its own): a step has at
                                     // most that many encoder pieces; its decode graph runs on the LAST of these streams -- a queue of its own while
                                     // the step has fewer pieces than there are streams, else right behind the last piece on that piece's lane
    std::vector<hipStream_t> lent;   // streams handed to another client (nasr_engine_lend_stream): still owned, destroyed with the engine
    int max_lanes = MAXSEG;          // option "lanes": the engine keeps at most this many (the others' hardware queues are left to other clients of the process)
    struct Pipe {
        bool ready = false;                               // buffers of this slot allocated
        char *g_desc = nullptr, *gh = nullptr;            // descriptor block of the encoder graphs (device / pinned)
        int *gh_collect = nullptr, *collect_dev = nullptr;
        int *g_dmeta = nullptr, *gh_dmeta = nullptr;      // k_collect meta of the decode graph [2 B] (device / pinned)
        float *encproj = nullptr;                         // [w_rows][640]: encoder graph -> decode graph
        hipEvent_t seg_done[MAXSEG] = {nullptr, nullptr, nullptr, nullptr};
        hipEvent_t dec_done = nullptr;
        bool dec_launched = false;
        std::map<int64_t, hipGraphExec_t> seg_graphs[MAXSEG], dec_graphs;     // key = (B, T, G, family, E)
        std::map<int64_t, int> dec_iters;                 // iterations dec_graphs[key] carries: where finish_step_decode's fallback goes on
        int stage = 0;                                    // encoder pieces launched so far (0 = slot free)
        int64_t seq = -1;                                 // sequence number of the step that occupies the slot
        std::vector<nasr_stream *> streams;
        int T = 0, G = 0, nseg = 0;
        int64_t key = 0;
    } pipe[NSLOT];
    // grouped pipeline ("pipeline" = 8, one or two rows per step on the fused path): the 8 steps in flight are at 8 stages of 3 layers;
    // chain c (HIP stream lane[c]) runs stages 4c .. 4c+3, each of its 24 launches per call carrying the same layer kind of FOUR steps
    struct GpEntry { int slot; int done; };            // a step in flight: its slot, the stages it has completed
    std::vector<GpEntry> gp_flight;                    // oldest first
    int64_t gp_calls = 0;
    int gp_next_slot = 0, gp_dec_pending = -1;          // slot whose decode graph is in flight (collected in the next call)
    hipEvent_t gp_ev[GP_C][2] = {{nullptr, nullptr}, {nullptr, nullptr}};       // chain c has finished the call of that parity
    bool gp_ev_set[GP_C][2] = {{false, false}, {false, false}};
    std::map<int64_t, hipGraphExec_t> gp_graphs[NSLOT][GP_C];                   // steady-state graphs by slot of the newest step
    int64_t gp_steps = 0, gp_graph_chains = 0, gp_eager_chains = 0;
    double host_launch_s = 0, host_wait_s = 0;     // NASR_STATS: host time inside hipGraphLaunch / waiting for the device (pipelined steps)
    int64_t pipe_seq = 0;            // steps launched through the pipeline so far
    bool pipe_ready = false;
    bool gemm_coresident = false;  // set while the graphs of a step with >= 2 launch chains are captured (run_gemm)
    size_t desc_bytes = 0, col_bytes = 0;
    int64_t pipe_steps = 0;
    void *a, *hbuf, *ctx, *cbuf, *sub_b;             // (with x, x2, part, q, glu, sub_a, hfuse: the CURRENT workspace set, see use_ws)
    unsigned *chain_flags = nullptr;                 // ... and its row-chunk counters of chained launches (a set's launches never overlap: one array per set)
    // option "token_logprobs": per-token log-probabilities from the decode kernels.  It picks the kernels that get captured into step graphs and
    // adds two buffers to `dec`, so it is taken only until the first decode has been enqueued (dec_started) or the first offline call has run
    bool opt_token_logprobs = false, dec_started = false;
    // option "phrase_boost" = the capacity of the automaton tables in states (0: off), nasr_boost.h.  Like "token_logprobs" it picks the kernels that
    // get captured and allocates fixed-capacity tables whose pointers never change: replacing the set rewrites their content only
    int opt_phrase_boost = 0, boost_cap = 0, boost_states = 0;      // capacity (0: off), capacity allocated; states of the current set (2 = the disabled state and the root: no phrase)
    float *boost_bonus = nullptr; int32_t *boost_next = nullptr;   // [capacity][1040] each
    nasr_boost::Automaton boost_host;   // the current set's tables on the host: a boosted beam call reads its hypotheses' per-token bonuses from them
    // nasr_engine_set_lm (nasr_lm.h): the compiled n-gram model on the host (the read-out of per-token values) and, in one device block, the
    // tables the beam kernels read.  Only beam calls see it
    nasr_lm::Model *lm = nullptr; void *lm_dev = nullptr;
    nasr_lm::View lm_view = {};      // device pointers
    float lm_weight = 0.0f, lm_bonus = 0.0f;
    // option "lm_fusion": shallow fusion in the greedy decode.  Like "phrase_boost" it picks the decode launches that get captured and
    // allocates what they read at fixed addresses: the block (the model's view + the greedy weights; the setters rewrite it), a state per slot, and per
    // slot the bias row (phrase bonus + lmbias) with the next-state row beside it
    int opt_lm_relook = 0;           // measurement switch "lm_commit_lookup" (1: the commit runs a second lookup instead of reading the next-state row)
    bool opt_lm_fusion = false; int opt_lm_fold = 1;      // lm_fold: measurement switch "lm_refresh_fold" (1: the refresh rides in k_dec_pred, 0: a launch of its own)
    nasr_lm::Greedy *lm_blk = nullptr;
    float glm_weight = 0.0f, glm_bonus = 0.0f;            // nasr_engine_set_greedy_lm_weights
    long long lm_generation = 0;     // counts nasr_engine_set_lm calls that changed the model: a beam call's LM read-out is tied to the model it ran with
    // option "token_alternatives" = K (0: off, 1 .. 8), nasr_topk.h: the K largest joint outputs with their log-probabilities where every token was
    // emitted.  Taken like "token_logprobs"; its kernels also leave the softmax parts, so lp_part / tok_logprob come with it
    int opt_token_alt = 0;                                         // K in use (dec.alt_k: K the buffers were allocated for)
    // option "frame_blank_logprobs": ln P(blank) at the last joint evaluation of every frame the decode has left.  Taken like "token_alternatives"
    // (LP kernels, so lp_part / tok_logprob come with it; the ring's life: DecodeSet::frame_blank)
    bool opt_frame_blank = false;
    // option "token_entropy" = round(1000 alpha) (0: off; nasr_entropy.h): the entropy of order alpha of the joint's softmax where every token was
    // emitted.  Taken like "frame_blank_logprobs" (the ENT forms of the LP kernels; ent_part / tok_entropy in `dec`)
    int opt_token_entropy = 0;
    // option "frame_history" = N (0: off; nasr_history.h): every step appends its encoder-projection rows to their slots' rings
    // [max_streams][N][640] f32, an engine buffer of its own -- not part of `dec`, so the fork plan and the snapshot format do not know it.  Taken
    // like "frame_blank_logprobs": it adds a launch that is captured into the step graphs
    int opt_frame_history = 0;
    float *hist_ring = nullptr;                        // the rings for opt_frame_history frames (set_history_option allocates and frees them; freed with the engine)
    int opt_history_append_rows = 0;                   // option "history_append_rows" (MEASUREMENT ONLY): 4 = k_history_append with four rows per workgroup; 0 = one (same bytes)
    int64_t history_calls = 0, history_frames = 0;     // counters of the same names: nasr_engine_history_* calls / frames they gathered
    int *collect_dev;               // [B][1+COLLECT_STRIDE]
    // descriptor staging
    char *pin = nullptr; size_t pin_cap = 0, pin_off = 0;
    char *ddesc = nullptr; size_t ddesc_cap = 0, ddesc_off = 0;
    int16_t *pcm_stage = nullptr; size_t pcm_stage_cap = 0;
    // host PCM hand-over: the streams' buffers are gathered into a pinned block and cross PCIe as ONE copy.  The copy is
    // asynchronous and a pipelined call returns before it has run, so the pinned blocks rotate (a block is reused four
    // calls later; up to pipeline + 1 = 5 steps are in flight, but the copy sits in piece 0 of its step, and the NEXT call launches piece 1 of that step only after the host has seen piece 0 complete).
    PinBlock pcm_pin[4];
    unsigned pcm_pin_next = 0;
    float *mel_stage = nullptr; size_t mel_stage_cap = 0;
    // audio input conversion: per-stream history [slot][2][nasr_rs::HIST_MAX] (allocated with the stream pool), one coefficient table per
    // rate in use (built and uploaded once), the raw staging area of nasr_engine_step_audio with its rotating pinned blocks (the
    // discipline of pcm_pin), and the debug copy behind NASR_TAP_PCM16
    float *aud_hist = nullptr;
    bool opt_audio_lds_table = true;        // option "audio_lds_table": k_audio_convert reads the coefficients of the L <= 2 rates from an LDS copy (same bits; 0.343 -> 0.253 ms per step at 512 streams x 48 kHz: profiles/audio_input.md)
    std::map<int, float *> aud_tables;
    char *raw_stage = nullptr; size_t raw_stage_cap = 0;
    PinBlock raw_pin[4];
    unsigned raw_pin_next = 0;
    int16_t *tap_pcm = nullptr; size_t tap_pcm_cap = 0;
    std::vector<int64_t> tap_pcm_off, tap_pcm_n;         // per slot: where the last call's samples are in tap_pcm, and how many
    // debug taps
    bool debug = false;
    float *tap_mel = nullptr; int tap_mel_cap = 0;      // [max_streams][tap_mel_cap][128] by batch row
    float *tap_sub = nullptr, *tap_layers = nullptr, *tap_enc = nullptr;  // [slot][...]
    std::vector<int> tap_mel_frames;                     // per slot: frames captured in last call
    std::vector<int> tap_mel_row;
    std::vector<nasr_stream *> slots;
    std::vector<void *> allocs;
    Prof prof;
    OfflineState *off = nullptr;     // offline path (nasr_engine_transcribe_mel): nullptr until its first call
    int opt_offline_rows = 16384;    // option "offline_rows": encoder rows per offline sub-batch
    int opt_align_cells = nasr_align::DEFAULT_CELLS;   // option "align_cells": lattice cells per launch of k_align_lattice (nasr_engine_align*)
};

constexpr int COLLECT_STRIDE = 256;
// what every frame-history entry answers on an engine without the option
constexpr const char *HISTORY_OFF = "no frame history: engine option \"frame_history\" is off (set it to the frames kept per stream before the first step or offline call)";


struct ProfScope {
    nasr_engine *e; int cat = -1; hipEvent_t a = nullptr; double bytes, flops;
    ProfScope(nasr_engine *e_, const char *name, double bytes_ = 0, double flops_ = 0) : e(e_), bytes(bytes_), flops(flops_) {
        if (!e->prof.on) return;
        Prof &pf = e->prof;
        if (pf.pending.size() >= 4096) prof_flush(e);
        cat = pf.cat(name);
        hipEvent_t b;
        if (pf.pool.size() >= 2) { a = pf.pool.back(); pf.pool.pop_back(); b = pf.pool.back(); pf.pool.pop_back(); }
        else { hipEventCreate(&a); hipEventCreate(&b); }
        evb = b;
        hipEventRecord(a, e->st);
    }
    ~ProfScope() {
        if (cat < 0) return;
        hipEventRecord(evb, e->st);
        e->prof.pending.push_back({cat, a, evb, bytes, flops});
    }
    hipEvent_t evb = nullptr;
};

namespace nasr_eng {
struct HostTimer {          // accumulates wall time of a scope into a double (diagnostics only: NASR_STATS)
    double &acc; std::chrono::steady_clock::time_point t0;
    explicit HostTimer(double &a) : acc(a), t0(std::chrono::steady_clock::now()) {}
    ~HostTimer() { acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};
struct GraphDescLayout { size_t rows, pcm, meta, vrows, total; };
float f16_to_f32(uint16_t h);
int64_t desc_numel(const nasr_weight_desc &d);
int to_f32(const nasr_weight_desc &d, std::vector<float> &out);
void transpose_9x256(const std::vector<float> &w /*[256][9]*/, std::vector<float> &t /*[9][256]*/);
void pack_f32_mfma(const std::vector<float> &w, int N, int K, bool lstm_order, std::vector<float> &out);
void host_pos_emb(int position, float *out);
int load_weights(nasr_engine *e, const nasr_weight_desc *w, int n_w);
int ensure_posproj(nasr_engine *e, int T);
int alloc_ws(nasr_engine *e, nasr_engine::WS &w);
void use_ws(nasr_engine *e, const nasr_engine::WS &w);
void engine_destroy_impl(nasr_engine *e);
int stream_zero_state(nasr_stream *s, bool keep_reference_state = false);
// a new stream in the lowest free slot whose device state and host mirror are src's (one k_stream_fork launch on the engine's stream); the
// caller holds an ApiGuard and has completed the steps in flight (pipe_drain)
int stream_fork(nasr_stream *src, nasr_stream **out);
void stream_register(const nasr_stream *s);      // the process-wide set of streams that exist (nasr_stream_fork refuses any other pointer)
void stream_unregister(const nasr_stream *s);
bool stream_is_live(const nasr_stream *s);
// what nasr_engine_finalize does between pipe_drain and its collect: the converter's tail, then one zero-padded step of what is buffered
int finalize_flush(nasr_engine *e, nasr_stream *const *streams, int B);
double gemm_bytes(const nasr_engine *e, int M, int N, int K, int wesz);
// out = A [M][K] (row stride lda) . W^T in one K slice, every other field zero: the caller sets the epilogue
inline GemmParams gemm_desc(const void *A, int lda, const void *W, int M, int N, int K) {
    GemmParams g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.W = W; g.M = M; g.N = N; g.K = K; g.lda = lda; g.splits = 1;
    return g;
}
int run_gemm(nasr_engine *e, GemmParams &g, bool f32_weights, const char *tag);
int pick_splits(const nasr_engine *e, int M, int N, int K);
// the GEMMs of the subsampling (the chunk step and the offline call; each launches its own conv0 + dw and depthwise conv):
// pointwise conv 3 (act -> f32, bias + ReLU) and 6 (act -> act, bias + ReLU) on M pixel rows, the out projection
// [frames][17 x 256] act -> x f32 on M frame rows; rows_per_batch > 0: GemmParams' row map of its A operand
void run_sub_pw3(nasr_engine *e, const void *in, float *out, int M);
void run_sub_pw6(nasr_engine *e, const void *in, void *out, int M);
void run_sub_out(nasr_engine *e, const void *in, float *x, int M, int rows_per_batch = 0, int batch_stride = 0, int row_offset = 0);
int run_layers_fused(nasr_engine *e, const RowDesc *rows, int B, int T, int G, int k0, int k1, std::vector<FusedParams> *rec = nullptr);
// The large-M conformer layers over packed rows: what the chunk step's unfused form and the offline call hand enqueue_layers.
// Rows [0, M) hold data (k_post, the depthwise conv); the GEMMs run on Mg >= M rows (the rows past M are scratch nobody reads).
struct LayerRun {
    float *x, *part, *glu;               // residual stream (f32), split-K partial slabs, pw1's GLU output
    void *a, *hbuf, *ctx, *cbuf;         // act dtype: LayerNorm output (the A operand of W1, QKV, pw1), FFN hidden, attention context, conv output
    int M, Mg;
    bool split_k;                        // the residual GEMMs may split K (pick_splits); false: one K slice
    bool chain;                          // a due k_post may ride as the head phase of the next GEMM that reads its rows
    std::function<void(int l, GemmParams &g)> qkv_out;   // layer l's QKV GEMM (A = a, its weights and shape set): where its output goes
    std::function<void(int l)> attention;                 // layer l's attention: the QKV GEMM's output -> ctx
    std::function<void(int l)> dwconv;                    // layer l's depthwise conv + LayerNorm + SiLU: glu -> cbuf
    std::function<int(int l)> tap;                        // debug: x after layer l (empty: none)
};
int enqueue_layers(nasr_engine *e, const LayerRun &r, int l0, int l1);
// prompt fusion (multilingual models) and the joint's encoder projection of rows [0, M) of x, the GEMMs on Mg >= M rows; row m
// takes the prompt of rows[m / rows_per_prompt].  tap (debug, may be empty): x is the encoder output, before the projection
int enqueue_encoder_tail(nasr_engine *e, float *x, float *hfuse, float *encproj, const RowDesc *rows, int M, int Mg, int rows_per_prompt,
                         const std::function<int()> &tap);
int enqueue_encoder(nasr_engine *e, const RowDesc *rows, const RowDesc *vrows, const int *tap_slots, int B, int T, int R, int G = 1, int seg = 0,
                           int nseg = 1, int part = 0);
void bind_dec_weights(const nasr_engine *e, DecParams &dp);     // the decoder's weights (prediction net, joint) into dp
DecFeatures dec_features(const nasr_engine *e);                 // the decode options in force (the opt_* fields)
void bind_decode(const nasr_engine *e, const DecodeSet &set, const DecFeatures &f, DecParams &dp);     // dec_set_bind with the engine's tables + bind_dec_weights; rows, B, T, encproj: the caller's
int ensure_decode_set(nasr_engine *e);                          // dec_set_ensure of e->dec for dec_features(e), through dalloc
void make_dec_params(nasr_engine *e, const RowDesc *rows, int B, int T, DecParams &dp);
// the head of every live step's decode sequence on st: launch_decode_begin, then -- option "frame_history" -- the step's rows into their rings
void enqueue_decode_begin(nasr_engine *e, const DecParams &dp, hipStream_t st);
// frames the stream's decode has left since create / reset, read from its slot (the caller has completed the steps in flight and holds an ApiGuard)
int stream_frames_done(const nasr_stream *s, int64_t *done);
void enqueue_decode_iters(nasr_engine *e, const DecParams &dp, int B, int n, int &it, hipStream_t st = nullptr);
// Rounds of decode iterations on st until no stream is active: `round` iterations, dp.n_active read into *landing, the round doubled (32 at
// most).  `it` = iterations enqueued so far; more than frames * MAX_SYMBOLS + 64 is the error "<what> did not terminate".  rounds: counted if given
int decode_until_idle(nasr_engine *e, const DecParams &dp, int B, hipStream_t st, int *landing, int it, int round, int frames,
                      int64_t *rounds = nullptr, const char *what = "decode");
void chunk_bookkeeping(nasr_stream *s, int row);
void fill_row_desc(RowDesc &rd, const nasr_stream *s, int n_dec);
int run_chunk(nasr_engine *e, const std::vector<nasr_stream *> &rows_s, const std::vector<int> &n_dec);
int drain_chunks(nasr_engine *e, nasr_stream *const *streams, int B);
int validate_batch(nasr_engine *e, nasr_stream *const *streams, int B);
int consume_collect(nasr_engine *e, const int *host, nasr_stream *const *streams, int B);
void deliver(nasr_stream *const *streams, int B, int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens);
int collect_tokens(nasr_engine *e, nasr_stream *const *streams, int B, int32_t *const *tokens_out,
                          const int32_t *tokens_cap, int32_t *n_tokens);
int ensure_debug_buffers(nasr_engine *e);
GraphDescLayout graph_desc_layout(int B, int G);
int build_step_graph(nasr_engine *e, int B, int T, int R, int G, hipGraphExec_t *out);
// the PcmDesc / RowDesc / virtual-row part of the pinned descriptor block gh of a graph step (graph_desc_layout), written in place
void fill_step_descs(char *gh, nasr_stream *const *streams, int B, int T, int G, const int16_t *const *pcm_dev, const int32_t *n_samples);
// host mirror of a queued graph step: the audio counts of gh's PcmDescs (audio), the G chunks under one conv-cache flip (chunks); ws_slot = last_ws
void mirror_step(nasr_stream *const *streams, int B, int T, int G, const char *gh, int ws_slot, bool audio = true, bool chunks = true);
MelParams step_mel_params(const nasr_engine *e, const PcmDesc *desc, int B, int T, int G);
int64_t lru_victim(const std::map<int64_t, hipGraphExec_t> &m, const std::map<int64_t, int64_t> &graph_used, int64_t key_tag);
// What follows a graph step's decode graph, whose k_collect left n_active behind gh_collect's B records: the chained-GEMM give-up flag, the
// eager completion on st from `iters` iterations on if the graph's budget fell short (and `fallback` allows it), then -- recollect -- k_collect again
struct StepDecode { const char *g_desc; float *encproj; const int *g_dmeta; int *collect_dev, *gh_collect; int B, T, G; };
int finish_step_decode(nasr_engine *e, const StepDecode &d, hipStream_t st, int iters, int round, bool fallback, bool recollect);
int pipe_blind_iterations(const nasr_engine *e, int B, int T, int G);
double spin_us(hipStream_t a, hipStream_t b);
int pick_lanes(nasr_engine *e);
void release_lanes(nasr_engine *e);
int ensure_pipe(nasr_engine *e, int p);
int build_pipe_graphs(nasr_engine *e, int p, int B, int T, int R, int G, int nseg, hipGraphExec_t *seg_out, hipGraphExec_t *dec_out, int *dec_iters);
int pipe_advance(nasr_engine *e, int p);
int pipe_finish_launch(nasr_engine *e, int p);
int pipe_finish(nasr_engine *e, int p);
int pipe_drain(nasr_engine *e);
int pipe_step(nasr_engine *e, nasr_stream *const *streams, int B, const int16_t *const *pcm_dev, const int32_t *n_samples, int G,
                     int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens);
bool gp_eligible(const nasr_engine *e, int B, int T, int G);
int gp_enqueue_chain(nasr_engine *e, int c, const int *slot_of_stage, int B, int T, int R, int G);
int gp_capture(nasr_engine *e, hipGraphExec_t *out, const std::function<int()> &body, hipStream_t st, const char *what);
int capture_decode_graph(nasr_engine *e, int p, int B, int T, int G, hipStream_t cs, int iters, const char *what, hipGraphExec_t *out);
int gp_call(nasr_engine *e, int new_slot, int64_t key, int B, int T, int R, int G);
int gp_finish_decode(nasr_engine *e);
int gp_drain(nasr_engine *e);
int gp_step(nasr_engine *e, nasr_stream *const *streams, int B, const int16_t *const *pcm_dev, const int32_t *n_samples, int G,
                   int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens);
int try_graph_step(nasr_engine *e, nasr_stream *const *streams, int B, const int16_t *const *pcm_dev,
                          const int32_t *n_samples, int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens);
int push_piece(nasr_engine *e, nasr_stream *const *streams, int B, const int16_t *const *base, const int32_t *n_samples,
                      int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens, uint32_t flags);
// what nasr_engine_step and nasr_engine_step_audio share once base[] points at every stream's 16 kHz s16 samples on the device
int step_tail(nasr_engine *e, nasr_stream *const *streams, int B, const int16_t *const *base, const int32_t *n_samples,
              int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens, uint32_t flags);
int ensure_audio_table(nasr_engine *e, const nasr_rs::Plan &p, const float **out);
void prof_flush(nasr_engine *e);
__global__ void k_collect(const int *slots, const int *tok_read, int B, const DecCtrl *ctrl, const int *tok_ring, int *out, int stride, const int *n_active);
inline bool streams_overlap(hipStream_t a, hipStream_t b, double alone_us) { return spin_us(a, b) < 1.5 * alone_us; }
inline bool dec_behind_last_piece(const nasr_engine *e, const nasr_engine::Pipe &P) { return P.nseg >= e->n_lanes; }
inline hipStream_t dec_stream(nasr_engine *e, const nasr_engine::Pipe &P) { return e->lane[e->n_lanes - 1]; }
template <typename Tp>
inline int stage_desc(nasr_engine *e, const std::vector<Tp> &host, const Tp **dev_out) {
    const size_t bytes = (host.size() * sizeof(Tp) + 255) & ~(size_t)255;
    if (bytes > e->pin_cap / 2) return fail("descriptor too large");
    if (e->pin_off + bytes > e->pin_cap || e->ddesc_off + bytes > e->ddesc_cap) {
        HIPCHK(hipStreamSynchronize(e->st));   // all earlier copies/kernels done: arenas reusable
        e->pin_off = 256;   // first 256 bytes: host landing zone of the decode 'n_active' read-back
        e->ddesc_off = 0;
    }
    char *hp = e->pin + e->pin_off, *dp = e->ddesc + e->ddesc_off;
    memcpy(hp, host.data(), host.size() * sizeof(Tp));
    HIPCHK(hipMemcpyAsync(dp, hp, host.size() * sizeof(Tp), hipMemcpyHostToDevice, e->st));
    e->pin_off += bytes;
    e->ddesc_off += bytes;
    *dev_out = (const Tp *)dp;
    return 0;
}
// grow-on-demand staging: room for `need` elements (+ slack), behind everything queued on the engine's stream
template <typename Tp>
inline int grow_device(nasr_engine *e, Tp **ptr, size_t *cap, size_t need, size_t slack) {
    if (need <= *cap) return 0;
    HIPCHK(hipStreamSynchronize(e->st));
    if (*ptr) hipFree(*ptr);
    *ptr = nullptr;
    *cap = 0;
    HIPCHK(hipMalloc((void **)ptr, (need + slack) * sizeof(Tp)));
    *cap = need + slack;
    return 0;
}
template <typename Tp>
inline int dalloc(nasr_engine *e, Tp **out, size_t n_elems) {
    void *p = nullptr;
    size_t bytes = std::max<size_t>(n_elems * sizeof(Tp), 16);
    HIPCHK(hipMalloc(&p, bytes));
    e->allocs.push_back(p);
    *out = (Tp *)p;
    return 0;
}
}  // namespace nasr_eng
