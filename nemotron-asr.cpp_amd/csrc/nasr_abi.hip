// nasr_abi.hip -- the step driver (graph step when eligible, eager sub-push loop otherwise) and the entry points of
// include/nemotron_asr_amd.h that are not life cycle: options, step / finalize / collect, counters, taps, profiling, device helpers.
// Which path a push takes and how it is cut is nasr_step_plan.h; the staging areas grow through grow_device, host buffers cross in PinBlocks.
#include "nasr_engine_priv.h"
#include "nasr_offline_plan.h"

namespace nasr_eng {
// builds the automaton on the host (nasr_boost.h) and, only if that succeeds, replaces the tables' content and puts every stream's history
// back to the root; the caller has completed the steps in flight
static int upload_boost_set(nasr_engine *e, int n_phrases, const int32_t *const *tokens, const int32_t *lens, const float *bonus) {
    nasr_boost::Automaton a;
    int bad = -1;
    const int rc = nasr_boost::build(n_phrases, tokens, lens, bonus, e->boost_cap, a, &bad);
    if (rc == nasr_boost::ERR_CAPACITY) return fail("boost phrases: %s of %d (engine option \"phrase_boost\"), at phrase %d", nasr_boost::status_text(rc), e->boost_cap, bad);
    if (rc) return fail("boost phrases: %s (phrase %d)", nasr_boost::status_text(rc), bad);
    HIPCHK(hipStreamSynchronize(e->st));
    const size_t n = nasr_boost::table_elems(a.n_states);
    HIPCHK(hipMemcpy(e->boost_bonus, a.bonus.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->boost_next, a.next.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
    std::vector<int> st((size_t)e->max_streams, nasr_boost::STATE_ROOT);
    for (int i = 0; i < e->max_streams; i++) if (e->slots[i] && !e->slots[i]->boost_enabled) st[(size_t)i] = nasr_boost::STATE_OFF;
    HIPCHK(hipMemcpy(e->dec.boost_state, st.data(), st.size() * sizeof(int), hipMemcpyHostToDevice));
    e->boost_states = a.n_states;
    e->boost_fp = nasr_snap::hash_bytes(nasr_snap::hash_bytes((uint64_t)a.n_states, a.bonus.data(), n * sizeof(float)), a.next.data(), n * sizeof(int32_t));   // a snapshot's boost_state means a row of THESE tables
    e->boost_host = std::move(a);
    return 0;
}

// builds the n-gram tables on the host (nasr_lm.h) and, only if that and the upload succeed, replaces the engine's model; the caller has
// completed the steps in flight.  One device block: states, unigrams, arcs
static int upload_lm(nasr_engine *e, const nasr_lm_desc *d) {
    if (d->flags != 0 || d->reserved != 0.0f) return fail("language model: flags and reserved must be 0");
    if (!nasr_beam::valid_weights(d->weight, d->token_bonus)) return fail("language model: weight and token_bonus must be finite in [0, 100]");
    HIPCHK(hipStreamSynchronize(e->st));                       // before anything is allocated: a failure here leaves nothing behind
    nasr_lm::Model *m = new nasr_lm::Model();
    std::string err;
    if (nasr_lm::build(d->order, d->n_ngrams, d->lengths, d->tokens, d->logprob, d->backoff, d->unk_logprob, *m, err)) {
        delete m;
        return fail("language model: %s", err.c_str());
    }
    auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t b_states = up16(m->states.size() * sizeof(nasr_lm::State)), b_uni = up16(m->uni.size() * sizeof(nasr_lm::Uni)), b_arcs = m->arcs.size() * sizeof(nasr_lm::Arc);
    char *dev = nullptr;
    if (hipMalloc((void **)&dev, b_arcs + b_uni + b_states) != hipSuccess) { (void)hipGetLastError(); delete m; return fail("language model: out of device memory"); }
    if (hipMemcpy(dev, m->arcs.data(), b_arcs, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dev + b_arcs, m->uni.data(), m->uni.size() * sizeof(nasr_lm::Uni), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dev + b_arcs + b_uni, m->states.data(), m->states.size() * sizeof(nasr_lm::State), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); hipFree(dev); delete m;
        return fail("language model: the upload failed");
    }
    delete e->lm;
    if (e->lm_dev) hipFree(e->lm_dev);
    e->lm = m; e->lm_dev = dev; e->lm_generation++;
    e->lm_fp = nasr_snap::hash_bytes(nasr_snap::hash_bytes(nasr_snap::hash_bytes(((uint64_t)(uint32_t)m->order << 32) | (uint32_t)m->start, m->states.data(), m->states.size() * sizeof(nasr_lm::State)),
                                                           m->uni.data(), m->uni.size() * sizeof(nasr_lm::Uni)), m->arcs.data(), b_arcs);      // a snapshot's lm_state and bias rows mean THIS model
    e->lm_view = m->view();
    e->lm_view.arcs = (const nasr_lm::Arc *)dev; e->lm_view.uni = (const nasr_lm::Uni *)(dev + b_arcs); e->lm_view.states = (const nasr_lm::State *)(dev + b_arcs + b_uni);
    e->lm_weight = d->weight; e->lm_bonus = d->token_bonus;
    return 0;
}

// engine option "lm_fusion": the bias rows (LM term + phrase bonus) of slots slot0 .. slot0 + n - 1 recomputed from their states, and waited for
static int refresh_lm_rows(nasr_engine *e, int slot0, int n) {
    launch_lm_rows(e->lm_blk, e->dec.lm_state, e->dec.lm_row, e->dec.lm_next, e->opt_phrase_boost ? e->boost_bonus : nullptr, e->opt_phrase_boost ? e->dec.boost_state : nullptr,
                   slot0, n, e->st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->st));
    return 0;
}

// engine option "lm_fusion": rewrites the block the decode kernels read from the engine's model and greedy weights and recomputes the bias rows
// of every slot in one launch -- after the states were put back to the model's start (restart: a new or detached model) or with the states
// kept (new weights, a new phrase set: the automaton states were reset by their own setter).  The caller has completed the steps in flight
static int refresh_greedy_lm(nasr_engine *e, bool restart) {
    if (!e->opt_lm_fusion) return 0;
    HIPCHK(hipStreamSynchronize(e->st));
    nasr_lm::Greedy g = {};
    g.lm = e->lm_view; g.attached = e->lm ? 1 : 0;
    g.weight = e->glm_weight; g.token_bonus = e->glm_bonus;
    HIPCHK(hipMemcpy(e->lm_blk, &g, sizeof(g), hipMemcpyHostToDevice));
    if (restart) {
        std::vector<int32_t> st((size_t)e->max_streams);
        for (int i = 0; i < e->max_streams; i++) st[(size_t)i] = nasr_lm::greedy_start(g, !e->slots[i] || e->slots[i]->lm_enabled);
        HIPCHK(hipMemcpy(e->dec.lm_state, st.data(), st.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return refresh_lm_rows(e, 0, e->max_streams);
}
}  // namespace nasr_eng

extern "C" int nasr_engine_set_lm(nasr_engine *e, const nasr_lm_desc *lm) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    // with "lm_fusion" the greedy decode reads the model too: the block is rewritten, every stream's LM state restarts and every bias row is recomputed
    if (lm) return upload_lm(e, lm) ? -1 : refresh_greedy_lm(e, true);
    HIPCHK(hipStreamSynchronize(e->st));
    nasr_lm::Model *old = e->lm; void *old_dev = e->lm_dev;
    e->lm_generation++;
    e->lm = nullptr; e->lm_dev = nullptr; e->lm_view = nasr_lm::View{}; e->lm_weight = e->lm_bonus = 0.0f;
    const int rc = refresh_greedy_lm(e, true);                 // the block forgets the tables before they are freed
    delete old;
    if (old_dev) hipFree(old_dev);
    return rc;
}

extern "C" int nasr_engine_set_greedy_lm_weights(nasr_engine *e, float weight, float token_bonus) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    if (!e->opt_lm_fusion) return fail("no greedy LM fusion: engine option \"lm_fusion\" is off (set it to 1 before the first step or offline call)");
    if (!nasr_beam::valid_weights(weight, token_bonus)) return fail("language model: weight and token_bonus must be finite in [0, 100]");
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    e->glm_weight = weight; e->glm_bonus = token_bonus;
    return refresh_greedy_lm(e, false);                        // the states stay; the rows follow the new weights
}

extern "C" int nasr_stream_set_lm(nasr_stream *s, int enable) {
    ApiGuard api_guard;
    if (!s) return fail("null stream");
    nasr_engine *e = s->e;
    if (!e->opt_lm_fusion) return fail("no greedy LM fusion: engine option \"lm_fusion\" is off (set it to 1 before the first step or offline call)");
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    HIPCHK(hipStreamSynchronize(e->st));
    nasr_lm::Greedy g = {};
    g.lm = e->lm_view; g.attached = e->lm ? 1 : 0;
    const int32_t state = nasr_lm::greedy_start(g, enable != 0);      // either way an empty history
    HIPCHK(hipMemcpy(e->dec.lm_state + s->slot, &state, sizeof(state), hipMemcpyHostToDevice));
    s->lm_enabled = enable != 0;
    return refresh_lm_rows(e, s->slot, 1);
}

extern "C" int nasr_engine_set_lm_weights(nasr_engine *e, float weight, float token_bonus) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    if (!e->lm) return fail("no language model attached (nasr_engine_set_lm)");
    if (!nasr_beam::valid_weights(weight, token_bonus)) return fail("language model: weight and token_bonus must be finite in [0, 100]");
    e->lm_weight = weight; e->lm_bonus = token_bonus;      // kernel parameters of the next beam call: nothing on the device changes
    return 0;
}

extern "C" int nasr_engine_set_boost_phrases(nasr_engine *e, int n_phrases, const int32_t *const *tokens, const int32_t *lens, const float *bonus) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    if (!e->opt_phrase_boost) return fail("no phrase boosting: engine option \"phrase_boost\" is off (set it to the state capacity before the first step or offline call)");
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    if (upload_boost_set(e, n_phrases, tokens, lens, bonus)) return -1;
    return refresh_greedy_lm(e, false);                        // "lm_fusion": the bias rows carry the phrase bonus
}

extern "C" int nasr_stream_set_boost(nasr_stream *s, int enable) {
    ApiGuard api_guard;
    if (!s) return fail("null stream");
    nasr_engine *e = s->e;
    if (!e->opt_phrase_boost) return fail("no phrase boosting: engine option \"phrase_boost\" is off (set it to the state capacity before the first step or offline call)");
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    HIPCHK(hipStreamSynchronize(e->st));
    const int state = enable ? nasr_boost::STATE_ROOT : nasr_boost::STATE_OFF;      // either way an empty history
    HIPCHK(hipMemcpy(e->dec.boost_state + s->slot, &state, sizeof(int), hipMemcpyHostToDevice));
    s->boost_enabled = enable != 0;
    return e->opt_lm_fusion ? refresh_lm_rows(e, s->slot, 1) : 0;      // the slot's bias row carries the phrase bonus
}

// The decode options.  Each picks the decode launches that get captured into the step graphs and adds what they read to e->dec (or, engine-wide: the
// automaton tables, the LM block) at addresses that never change, so that the setters behind them only ever rewrite content and captured graphs stay
// valid.  A later change would be a silent no-op for the graphs that exist (and the tokens already in the ring would have no value): they are taken
// until the first decode has been enqueued or the first offline call has run.  "lm_refresh_fold" (0 = the bias rows are refreshed by a launch of
// their own) and "lm_commit_lookup" (1 = k_dec_commit looks the emitted token up again) are measurement only (profiles/greedy_lm.md)
static const char *const DECODE_OPTIONS[] = {"token_logprobs", "phrase_boost", "lm_fusion", "lm_refresh_fold", "lm_commit_lookup", "token_alternatives", "frame_blank_logprobs", "token_entropy"};
static bool is_decode_option(const char *key) { return std::any_of(std::begin(DECODE_OPTIONS), std::end(DECODE_OPTIONS), [key](const char *k) { return !strcmp(key, k); }); }
static int set_decode_option(nasr_engine *e, const char *key, int value) {      // key is one of DECODE_OPTIONS; the caller holds an ApiGuard
    const auto is = [key](const char *k) { return !strcmp(key, k); };
    if ((is("token_logprobs") || is("lm_fusion") || is("frame_blank_logprobs")) && value != 0 && value != 1) return fail("%s must be 0 or 1", key);
    if (is("phrase_boost") && value != 0 && (value < nasr_boost::MIN_STATES || value > nasr_boost::MAX_STATES))
        return fail("phrase_boost must be 0 or the automaton's state capacity, %d .. %d", nasr_boost::MIN_STATES, nasr_boost::MAX_STATES);
    if (is("token_alternatives") && !nasr_topk::valid_k(value)) return fail("token_alternatives must be 0 .. %d", nasr_topk::KMAX);
    if (is("token_entropy") && !nasr_ent::valid_milli(value))
        return fail("token_entropy must be 0 or round(1000 alpha): %d (Shannon), or %d .. %d and %d .. %d (closer to 1 the order's 1 / (1 - alpha) outgrows the value's precision)",
                    nasr_ent::MILLI_SHANNON, nasr_ent::MILLI_MIN, nasr_ent::BAND_LO, nasr_ent::BAND_HI, nasr_ent::MILLI_MAX);
    if (e->dec_started || e->off) return fail("%s must be set before the first step or offline call (the decode kernels are already chosen)", key);
    if (is("phrase_boost") && value && e->boost_bonus && value != e->boost_cap) return fail("phrase_boost: the capacity is already %d states", e->boost_cap);
    HIPCHK(hipSetDevice(e->device));
    // the option's field, and what the options now in force need of e->dec; a failure leaves the field as it was
    const auto take = [e](auto &opt, auto v) { const auto before = opt; opt = v; if (ensure_decode_set(e)) { opt = before; return -1; } return 0; };
    if (is("token_logprobs")) return take(e->opt_token_logprobs, value != 0);
    if (is("token_alternatives")) return take(e->opt_token_alt, value);
    if (is("frame_blank_logprobs")) return take(e->opt_frame_blank, value != 0);
    if (is("token_entropy")) return take(e->opt_token_entropy, value);
    if (is("lm_refresh_fold")) return take(e->opt_lm_fold, value != 0 ? 1 : 0);
    if (is("lm_commit_lookup")) return take(e->opt_lm_relook, value != 0 ? 1 : 0);
    if (is("phrase_boost")) {
        const int before = e->opt_phrase_boost;
        if (take(e->opt_phrase_boost, value)) return -1;
        if (value && !e->boost_bonus) {                        // the automaton tables at a fixed capacity, holding the empty set: the disabled state and the root
            if (dalloc(e, &e->boost_bonus, nasr_boost::table_elems(value)) || dalloc(e, &e->boost_next, nasr_boost::table_elems(value))) { e->opt_phrase_boost = before; return -1; }
            e->boost_cap = value;
            if (upload_boost_set(e, 0, nullptr, nullptr, nullptr)) { e->opt_phrase_boost = 0; return -1; }
        }
        return e->opt_lm_fusion ? refresh_greedy_lm(e, false) : 0;      // "lm_fusion" set before this option: the rows gain (or lose) the phrase bonus
    }
    if (take(e->opt_lm_fusion, value != 0)) return -1;      // "lm_fusion": the block (the model's view + the greedy weights) and the rows of every slot
    if (value && ((!e->lm_blk && dalloc(e, &e->lm_blk, 1)) || refresh_greedy_lm(e, true))) { e->opt_lm_fusion = false; return -1; }
    return 0;
}

// "frame_history" = N: a capability like the decode options -- the append is captured into the step graphs with the rings' address -- so it is
// taken until the first decode has been enqueued or the first offline call has run.  Until then no launch knows the rings: another N replaces
// them and 0 frees them
static int set_history_option(nasr_engine *e, int value) {          // the caller holds an ApiGuard
    if (!nasr_hist::valid_frames(value))
        return fail("frame_history must be 0 or the frames kept per stream, %d .. %d in multiples of %d", nasr_hist::MIN_FRAMES, nasr_hist::MAX_FRAMES, nasr_hist::MIN_FRAMES);
    if (e->dec_started || e->off) return fail("frame_history must be set before the first step or offline call (the step's launches are already chosen)");
    HIPCHK(hipSetDevice(e->device));
    if (value != e->opt_frame_history) {
        float *ring = nullptr;
        if (value) HIPCHK(hipMalloc((void **)&ring, (size_t)nasr_hist::ring_bytes(e->max_streams, value)));
        if (e->hist_ring) hipFree(e->hist_ring);
        e->hist_ring = ring;
        e->opt_frame_history = value;
    }
    return 0;
}

extern "C" int nasr_engine_set_option(nasr_engine *e, const char *key, int value) {
    if (!e || !key) return fail("null argument");
    if (!strcmp(key, "fused")) {
        // the family of the small steps, and with it their lane cut: nothing cut the other way may be in flight (pipe_step would drain at the
        // next step anyway; here the option's caller pays, not the next call)
        if (e->opt_fused != (value != 0)) {
            ApiGuard api_guard;
            HIPCHK(hipSetDevice(e->device));
            if (pipe_drain(e)) return -1;
        }
        e->opt_fused = value != 0;
    }
    else if (!strcmp(key, "graph")) e->opt_graph = value != 0;
    else if (!strcmp(key, "graph_cache")) { if (value < 1) return fail("graph_cache must be >= 1"); e->opt_graph_cache = value; }
    else if (!strcmp(key, "multichunk")) e->opt_multichunk = value != 0;
    else if (!strcmp(key, "large_step_pieces")) { if (value < 0 || value > nasr_engine::MAXSEG) return fail("large_step_pieces must be 0 .. %d", (int)nasr_engine::MAXSEG); e->opt_large_step_pieces = value; }
    else if (!strcmp(key, "t64_tiles")) { if (value < 0) return fail("t64_tiles must be >= 0"); e->opt_t64_tiles = value; }      // like "fused": set before the first step
    else if (!strcmp(key, "tile_bands")) e->opt_tile_bands = value;
    else if (!strcmp(key, "wide_tiles")) e->opt_wide_tiles = value;              // like "fused": set before the first step
    else if (!strcmp(key, "persistent_gemm")) e->opt_persist_gemm = value != 0;      // like "fused": set before the first step
    else if (!strcmp(key, "gemm_cores")) { if (value < -1 || value > 1) return fail("gemm_cores must be -1, 0 or 1"); e->opt_gemm_cores = value; }
    else if (!strcmp(key, "decode_graph_iterations")) { if (value < 0) return fail("decode_graph_iterations must be >= 1, or 0 (auto)"); e->opt_decode_graph_iters = value; }
    else if (!strcmp(key, "fused_cuts")) {
        // measurement only: read when a step shape's piece graphs are captured, and steps in flight must all be cut alike
        int cut4[3];
        unpack_cut4(value, cut4);
        if (value != 0 && !valid_cut4(cut4, e->hp.n_layers)) return fail("fused_cuts: three launch indices of a 24-layer model, 10 bits each, that leave four non-empty pieces");
        if (e->pipe_steps || e->gp_steps) return fail("fused_cuts must be set before the first pipelined step");
        e->opt_fused_cuts = value;
    }
    else if (!strcmp(key, "decode_lane")) {
        // read by pick_lanes() only, and the lanes are picked once: later the option would be a silent no-op (round-4 advisor)
        if (e->pipe_ready) return fail("decode_lane must be set before the first pipelined step (the lanes are already picked)");
        e->opt_decode_lane = value != 0;
    }
    else if (is_decode_option(key)) { ApiGuard api_guard; if (set_decode_option(e, key, value)) return -1; }
    else if (!strcmp(key, "history_append_rows")) {          // measurement only: the grid of k_history_append (same bytes); before the first step
        if (value != 0 && value != 1 && value != 4) return fail("history_append_rows must be 0, 1 or 4");
        if (e->dec_started) return fail("history_append_rows must be set before the first step");
        e->opt_history_append_rows = value == 4 ? 4 : 0;
    }
    else if (!strcmp(key, "frame_history")) { ApiGuard api_guard; if (set_history_option(e, value)) return -1; }
    else if (!strcmp(key, "wide_min_tiles")) e->opt_wide_min_tiles = value;
    else if (!strcmp(key, "large_step_rows")) e->opt_large_step_rows = value;
    else if (!strcmp(key, "wide_min_rows")) e->opt_wide_min_rows = value;
    else if (!strcmp(key, "gemm_prio")) e->opt_gemm_prio = value;                    // probe: GemmParams::prio (measurement only)
    else if (!strcmp(key, "epilogue16")) e->opt_epilogue16 = value != 0;            // like "fused": set before the first step
    else if (!strcmp(key, "dwconv_stream")) e->opt_dwconv_stream = value != 0;      // like "fused": set before the first step
    else if (!strcmp(key, "chain")) { if (value < 0 || value > 2) return fail("chain must be 0, 1 or 2"); e->opt_chain = value; }      // like "fused": set before the first step
    else if (!strcmp(key, "split_tasks")) e->opt_split_tasks = value;                // like "fused": set before the first step
    else if (!strcmp(key, "resid_epilogue")) { if (value < 0 || value > 2) return fail("resid_epilogue must be 0, 1 or 2"); e->opt_resid_epilogue = value; }      // like "fused": set before the first step
    else if (!strcmp(key, "offline_rows")) { if (value < 1) return fail("offline_rows must be >= 1"); e->opt_offline_rows = value; }
    else if (!strcmp(key, "align_cells")) { if (value < nasr_align::MIN_CELLS) return fail("align_cells must be >= %d", nasr_align::MIN_CELLS); e->opt_align_cells = value; }
    else if (!strcmp(key, "audio_lds_table")) e->opt_audio_lds_table = value != 0;      // A/B switch of k_audio_convert (same bits)
    else if (!strcmp(key, "fork_piece_kb")) { if (value < 0 || value > 1024) return fail("fork_piece_kb must be 0 .. 1024"); e->opt_fork_piece_kb = value; }      // measurement only: the grid of k_stream_fork (same bytes)
    else if (!strcmp(key, "ablate")) e->opt_ablate = value;          // measurement only (see the header); before the first step
    else if (!strcmp(key, "f32_mfma")) e->opt_f32_mfma = value != 0;      // 0: f32 GEMMs above four rows on the FMA tile kernel (round 3's path); like "fused", set before the first step
    else if (!strcmp(key, "pipeline")) {
        ApiGuard api_guard;
        HIPCHK(hipSetDevice(e->device));
        if (pipe_drain(e)) return -1;
        if ((value < 0 || value > nasr_engine::MAXSEG) && value != nasr_engine::GP_S) return fail("pipeline must be 0 .. %d, or %d (grouped)", (int)nasr_engine::MAXSEG, (int)nasr_engine::GP_S);
        e->opt_pipeline = value;
    }
    else if (!strcmp(key, "lanes")) {
        // give hardware queues back: another GPU client of the process (the diarization side-car) whose stream is created AFTER
        // this call lands on a queue this engine no longer uses (the runtime hands a new stream the least-used queue)
        ApiGuard api_guard;
        HIPCHK(hipSetDevice(e->device));
        if (value < 1 || value > nasr_engine::MAXSEG) return fail("lanes must be 1 .. %d", (int)nasr_engine::MAXSEG);
        if (pipe_drain(e)) return -1;
        e->max_lanes = value;
        release_lanes(e);
    }
    else return fail("unknown option '%s'", key);
    return 0;
}

extern "C" int nasr_engine_set_debug(nasr_engine *e, int enable) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    if (enable && ensure_debug_buffers(e)) return -1;
    e->debug = enable != 0;
    return 0;
}

// returns 1 if the step was executed through the graph, 0 if not eligible, <0 on error
namespace nasr_eng {
int try_graph_step(nasr_engine *e, nasr_stream *const *streams, int B, const int16_t *const *pcm_dev,
                          const int32_t *n_samples, int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens) {
    const int T = streams[0]->T, R = streams[0]->R;
    std::vector<int> cnt((size_t)2 * B);          // [abuf_cnt B][mel_count B]
    for (int b = 0; b < B; b++) { cnt[(size_t)b] = streams[b]->abuf_cnt; cnt[(size_t)B + b] = streams[b]->mel_count; }
    const int G = graph_step_chunks(cnt.data(), cnt.data() + B, n_samples, B, T, e->w_rows, e->opt_multichunk);
    if (G == 0) return 0;
    if (e->opt_pipeline) {
        if (!e->pipe_ready && ensure_pipe(e, 0)) return -1;          // picks the lanes
        if (gp_eligible(e, B, T, G)) return gp_step(e, streams, B, pcm_dev, n_samples, G, tokens_out, tokens_cap, n_tokens);
        if (gp_drain(e)) return -1;
        return pipe_step(e, streams, B, pcm_dev, n_samples, G, tokens_out, tokens_cap, n_tokens);
    }
    if (pipe_drain(e)) return -1;
    const int64_t key = ((int64_t)B << 32) | ((int64_t)T << 16) | (int64_t)G;
    auto it = e->graphs.find(key);
    e->graph_used[key] = ++e->graph_tick;
    if (it == e->graphs.end()) {
        HIPCHK(hipStreamSynchronize(e->st));
        while ((int)e->graphs.size() >= e->opt_graph_cache) {          // bounded cache, least recently used shape first
            const int64_t victim = lru_victim(e->graphs, e->graph_used, 0);
            hipGraphExecDestroy(e->graphs[victim]);
            e->graphs.erase(victim);
            e->graph_used.erase(victim);
            e->graph_evictions++;
        }
        hipGraphExec_t ex = nullptr;
        {
            CaptureExclusive alone;
            if (build_step_graph(e, B, T, R, G, &ex)) return -1;
        }
        it = e->graphs.emplace(key, ex).first;
    }
    fill_step_descs(e->gh, streams, B, T, G, pcm_dev, n_samples);
    int *gh_meta = (int *)(e->gh + graph_desc_layout(B, G).meta);
    for (int b = 0; b < B; b++) { gh_meta[b] = streams[b]->slot; gh_meta[B + b] = streams[b]->tok_read; }
    HIPCHK(hipGraphLaunch(it->second, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    e->graph_replays++;
    mirror_step(streams, B, T, G, e->gh, 0, true, false);          // the audio counts before the decode's outcome is looked at ...
    // ... which the eager completion (rounds from 4 iterations at one frame) leaves in the token ring: collect_tokens
    const int fell_back = finish_step_decode(e, StepDecode{e->g_desc, e->encproj, nullptr, e->collect_dev, e->gh_collect, B, T, G}, e->st,
                                             decode_blind_iterations(T * G), T * G > 1 ? 8 : 4, true, false);
    if (fell_back < 0) return -1;
    mirror_step(streams, B, T, G, e->gh, 0, false, true);          // ... the chunk bookkeeping after
    if (fell_back) return collect_tokens(e, streams, B, tokens_out, tokens_cap, n_tokens) ? -1 : 1;
    if (consume_collect(e, e->gh_collect, streams, B)) return -1;
    deliver(streams, B, tokens_out, tokens_cap, n_tokens);
    return 1;
}

// one piece of a push (device-resident PCM): the graph-replayed launch sequence when eligible, else the eager
// sub-push loop (mel -> chunk by chunk) -- then the new tokens of every stream
int push_piece(nasr_engine *e, nasr_stream *const *streams, int B, const int16_t *const *base, const int32_t *n_samples,
                      int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens, uint32_t flags) {
    std::vector<int64_t> off(B, 0);
    if (e->opt_graph && !e->debug && !e->prof.on && !(flags & NASR_FLAG_NO_SYNC)) {
        const int gr = try_graph_step(e, streams, B, base, n_samples, tokens_out, tokens_cap, n_tokens);
        if (gr < 0) return -1;
        if (gr == 1) return 0;
    }
    if (pipe_drain(e)) return -1;
    e->eager_steps++;
    // sub-pushes of at most MAX_PUSH samples keep the audio buffer and the mel ring bounded
    for (;;) {
        std::vector<PcmDesc> pd;
        int max_frames = 0, max_n = 0;
        std::vector<int> who;
        for (int b = 0; b < B; b++) {
            const int64_t rem = n_samples[b] - off[b];
            if (rem <= 0) continue;
            nasr_stream *s = streams[b];
            PcmDesc d;
            memset(&d, 0, sizeof(d));
            d.pcm = base[b] + off[b];
            d.slot = s->slot;
            fill_pcm_counts(d, (int)std::min<int64_t>(rem, MAX_PUSH), s->abuf_cnt, s->abuf_par, s->mel_start, s->mel_count);
            pd.push_back(d);
            who.push_back(b);
            max_frames = std::max(max_frames, d.n_frames);
            max_n = std::max(max_n, d.n);
        }
        if (pd.empty()) break;
        const PcmDesc *dpd;
        if (stage_desc(e, pd, &dpd)) return -1;
        MelParams mp;
        memset(&mp, 0, sizeof(mp));
        mp.desc = dpd; mp.B = (int)pd.size(); mp.max_frames = max_frames; mp.abuf = e->abuf; mp.last_sample = e->last_sample;
        mp.mel_ring = e->mel_ring; mp.window = e->window; mp.fbT = e->fbT; mp.fb_band = e->fb_band; mp.cos_t = e->cos_t; mp.sin_t = e->sin_t;
        if (e->debug) { mp.tap = e->tap_mel; mp.tap_cap = e->tap_mel_cap; }
        {
            ProfScope ps(e, "k_mel", 0, 0);
            launch_mel(mp, max_n, e->st);
        }
        for (size_t i = 0; i < pd.size(); i++) {
            nasr_stream *s = streams[who[i]];
            off[who[i]] += pd[i].n;
            apply_pcm_counts(pd[i], s->abuf_cnt, s->abuf_par, s->mel_count);
            if (e->debug) { e->tap_mel_frames[s->slot] = pd[i].n_frames; e->tap_mel_row[s->slot] = (int)i; }
        }
        if (drain_chunks(e, streams, B)) return -1;
    }
    if (flags & NASR_FLAG_NO_SYNC) {
        if (n_tokens) for (int b = 0; b < B; b++) n_tokens[b] = 0;
        return 0;
    }
    return collect_tokens(e, streams, B, tokens_out, tokens_cap, n_tokens);
}

}  // namespace nasr_eng
int PinBlock::acquire(size_t bytes, size_t slack, hipStream_t st) {
    if (pending) { HIPCHK(hipEventSynchronize(copied)); pending = false; }
    if (bytes <= cap) return 0;
    HIPCHK(hipStreamSynchronize(st));
    if (p) hipHostFree(p);
    p = nullptr;
    cap = bytes + slack;
    HIPCHK(hipHostMalloc((void **)&p, cap, hipHostMallocDefault));
    return 0;
}
int PinBlock::copy_to(void *dev, size_t bytes, hipStream_t st) {
    if (bytes == 0) return 0;
    HIPCHK(hipMemcpyAsync(dev, p, bytes, hipMemcpyHostToDevice, st));
    if (!copied) HIPCHK(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
    HIPCHK(hipEventRecord(copied, st));
    pending = true;
    return 0;
}
namespace nasr_eng {

// s16 16 kHz mono in: host buffers are gathered into the device staging area (device buffers are read in place), then the step
static int step_s16(nasr_engine *e, nasr_stream *const *streams, int B, const int16_t *const *pcm, const int32_t *n_samples,
                    int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens, uint32_t flags) {
    std::vector<const int16_t *> base(B, nullptr);
    size_t total = 0;
    for (int b = 0; b < B; b++) {
        if (n_samples[b] < 0) return fail("negative n_samples");
        if (n_samples[b] > 0 && !pcm[b]) return fail("null pcm for stream %d", b);
        total += (size_t)n_samples[b];
    }
    if (!(flags & NASR_FLAG_PCM_DEVICE)) {
        // hand-over of host buffers: one gather into the device staging area
        if (grow_device(e, &e->pcm_stage, &e->pcm_stage_cap, total, 65536)) return -1;
        PinBlock &pin = e->pcm_pin[e->pcm_pin_next++ & 3];
        if (pin.acquire(total * 2, 65536 * 2, e->st)) return -1;
        size_t o = 0;
        for (int b = 0; b < B; b++) {
            if (n_samples[b] > 0) memcpy(pin.p + o * 2, pcm[b], (size_t)n_samples[b] * 2);
            base[b] = e->pcm_stage + o;
            o += (size_t)n_samples[b];
        }
        ProfScope ps(e, "h2d_pcm", (double)total * 2);
        if (pin.copy_to(e->pcm_stage, total * 2, e->st)) return -1;
    } else {
        for (int b = 0; b < B; b++) base[b] = pcm[b];
    }
    return step_tail(e, streams, B, base.data(), n_samples, tokens_out, tokens_cap, n_tokens, flags);
}

// debug: keeps what this call hands the front end (NASR_TAP_PCM16); the tap of every stream that is not in the call is forgotten
static int record_pcm_tap(nasr_engine *e, nasr_stream *const *streams, int B, const int16_t *const *base, const int32_t *n_samples) {
    size_t total = 0;
    for (int b = 0; b < B; b++) total += (size_t)n_samples[b];
    if (grow_device(e, &e->tap_pcm, &e->tap_pcm_cap, total, 65536)) return -1;
    std::fill(e->tap_pcm_n.begin(), e->tap_pcm_n.end(), 0);
    size_t o = 0;
    for (int b = 0; b < B; b++) {
        e->tap_pcm_off[streams[b]->slot] = (int64_t)o;
        e->tap_pcm_n[streams[b]->slot] = n_samples[b];
        if (n_samples[b] > 0) HIPCHK(hipMemcpyAsync(e->tap_pcm + o, base[b], (size_t)n_samples[b] * 2, hipMemcpyDeviceToDevice, e->st));
        o += (size_t)n_samples[b];
    }
    return 0;
}

int step_tail(nasr_engine *e, nasr_stream *const *streams, int B, const int16_t *const *base, const int32_t *n_samples,
              int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens, uint32_t flags) {
    if (e->debug) for (int b = 0; b < B; b++) { e->tap_mel_frames[streams[b]->slot] = 0; e->tap_mel_row[streams[b]->slot] = b; }
    if (e->debug && record_pcm_tap(e, streams, B, base, n_samples)) return -1;
    for (int b = 0; b < B; b++) streams[b]->samples_in += n_samples[b];
    // A push longer than one launch sequence can take (MAXNEW encoder frames per stream, w_rows rows in all) is
    // cut into pieces of whole chunks; each piece is a multi-chunk step when the streams are aligned.
    const int T = streams[0]->T;
    const int64_t piece = piece_samples(T, B, e->w_rows);
    bool multi = false;
    for (int b = 0; b < B; b++) multi = multi || n_samples[b] > piece;
    if (!multi) return push_piece(e, streams, B, base, n_samples, tokens_out, tokens_cap, n_tokens, flags);
    std::vector<int64_t> off(B, 0);
    std::vector<int32_t> acc(B, 0), np(B), cap_left(B), got(B);
    std::vector<const int16_t *> ptr(B);
    std::vector<int32_t *> outp(B);
    for (;;) {
        bool any = false;
        for (int b = 0; b < B; b++) {
            const int64_t rem = n_samples[b] - off[b];
            np[b] = (int32_t)std::min<int64_t>(rem, piece);
            any = any || np[b] > 0;
            ptr[b] = base[b] + off[b];
            const int32_t cap = tokens_out && tokens_out[b] && tokens_cap ? tokens_cap[b] : 0;
            const int32_t used = std::min(acc[b], cap);
            outp[b] = cap > 0 ? tokens_out[b] + used : nullptr;
            cap_left[b] = cap - used;
        }
        if (!any) break;
        if (push_piece(e, streams, B, ptr.data(), np.data(), outp.data(), cap_left.data(), got.data(), flags)) return -1;
        for (int b = 0; b < B; b++) { off[b] += np[b]; acc[b] += got[b]; }
    }
    if (n_tokens) for (int b = 0; b < B; b++) n_tokens[b] = acc[b];
    return 0;
}

// ---- audio input conversion (nasr_resample.h, kernels_audio.hip) --------------------------------------------------------------------
// the coefficient table of a rate: built in double on the host and uploaded the first time a stream or a one-shot conversion names the rate
int ensure_audio_table(nasr_engine *e, const nasr_rs::Plan &p, const float **out) {
    auto it = e->aud_tables.find(p.fin);
    if (it == e->aud_tables.end()) {
        for (long long n = 0; n < (long long)p.M * nasr_rs::BLOCK; n += nasr_rs::BLOCK)        // the spans repeat with period M blocks
            if (nasr_rs::block_span(p, n) > nasr_rs::SPAN_CAP) return fail("internal: %d Hz needs %lld staged frames per workgroup", p.fin, nasr_rs::block_span(p, n));
        if (p.hist > nasr_rs::HIST_MAX) return fail("internal: %d Hz needs a history of %d frames", p.fin, p.hist);
        std::vector<float> c;
        nasr_rs::build_table(p, c);
        float *d = nullptr;
        if (dalloc(e, &d, c.size())) return -1;
        HIPCHK(hipMemcpy(d, c.data(), c.size() * 4, hipMemcpyHostToDevice));
        it = e->aud_tables.emplace(p.fin, d).first;
    }
    *out = it->second;
    return 0;
}

static void fill_audio_desc(const nasr_engine *e, AudioDesc &d, const nasr_rs::Plan &p, const nasr_audio_format &f, const float *table) {
    memset(&d, 0, sizeof(d));
    d.lds_table = e->opt_audio_lds_table && 2 * p.half + 1 <= LDS_TABLE_MAX ? 1 : 0;
    d.table = table; d.enc = f.encoding; d.channels = f.channels; d.channel = f.channel; d.L = p.L; d.M = p.M; d.half = p.half;
}
static double audio_flops(const nasr_rs::Plan &p, double n_out) { return n_out * 2.0 * (double)(2 * p.half / p.L + 1); }

// descs[b].n_out samples of every stream b into e->pcm_stage, packed in order: ONE launch on the engine's stream.  pcm_stage is written here
// where nasr_engine_step's H2D copy writes it, and under the same ordering: every reader of pcm_stage -- k_preemph, the first kernel of a
// step -- is enqueued on e->st (eagerly, as the head of the synchronous step graph, in piece 0 of a pipelined step whose lane 0 IS e->st, in
// chain 0 of the grouped pipeline, again lane 0), so stream order puts this launch behind the previous call's readers and in front of this call's
static int run_audio_convert(nasr_engine *e, std::vector<AudioDesc> &descs, std::vector<const int16_t *> &base, double in_bytes, double flops) {
    size_t total = 0;
    long long max_out = 0;
    for (auto &d : descs) { total += (size_t)d.n_out; max_out = std::max(max_out, d.n_out); }
    if (grow_device(e, &e->pcm_stage, &e->pcm_stage_cap, total, 65536)) return -1;
    size_t o = 0;
    for (size_t b = 0; b < descs.size(); b++) {
        descs[b].out = e->pcm_stage + o;
        base[b] = e->pcm_stage + o;
        o += (size_t)descs[b].n_out;
    }
    const AudioDesc *dd;
    if (stage_desc(e, descs, &dd)) return -1;
    ProfScope ps(e, "audio_convert", in_bytes + (double)total * 2, flops);
    launch_audio_convert(dd, (int)descs.size(), max_out, e->st);
    HIPCHK(hipGetLastError());
    return 0;
}

// nasr_engine_finalize: the samples that waited for input which will not come, through the front end like any push (eager, tokens stay
// on the device until the caller's collect)
int audio_flush(nasr_engine *e, nasr_stream *const *streams, int B) {
    if (e->debug) for (int b = 0; b < B; b++) e->tap_pcm_n[streams[b]->slot] = 0;      // NASR_TAP_PCM16: a finalize that flushes nothing hands over nothing
    bool any = false;
    for (int b = 0; b < B; b++) any = any || (!streams[b]->default_format() && nasr_rs::out_total(streams[b]->aud_plan, streams[b]->aud_in) > streams[b]->aud_out);
    if (!any) return 0;
    std::vector<AudioDesc> descs((size_t)B);
    std::vector<const int16_t *> base((size_t)B, nullptr);
    std::vector<int32_t> n16((size_t)B, 0);
    double flops = 0;
    for (int b = 0; b < B; b++) {
        nasr_stream *s = streams[b];
        fill_audio_desc(e, descs[b], s->aud_plan, s->fmt(), s->aud_table);
        const long long n = s->default_format() ? 0 : nasr_rs::out_total(s->aud_plan, s->aud_in) - s->aud_out;
        descs[b].hist = e->aud_hist + (size_t)s->slot * 2 * nasr_rs::HIST_MAX; descs[b].par = s->aud_par;
        descs[b].n_before = s->aud_in; descs[b].n_push = 0; descs[b].out_first = s->aud_out; descs[b].n_out = n > 0 ? n : 0;
        n16[b] = (int32_t)descs[b].n_out;
        flops += audio_flops(s->aud_plan, (double)descs[b].n_out);
    }
    if (run_audio_convert(e, descs, base, 0, flops)) return -1;
    for (int b = 0; b < B; b++) streams[b]->aud_out += n16[b];
    return step_tail(e, streams, B, base.data(), n16.data(), nullptr, nullptr, nullptr, NASR_FLAG_NO_SYNC);
}

// the flags a step entry does not take
static int refuse_offline_flags(uint32_t flags) {
    if (flags & NASR_FLAG_NO_BOOST) return fail("NASR_FLAG_NO_BOOST belongs to the offline entries; a stream is switched with nasr_stream_set_boost");
    if (flags & NASR_FLAG_NO_LM) return fail("NASR_FLAG_NO_LM belongs to the offline entries; a stream is switched with nasr_stream_set_lm");
    return 0;
}

}  // namespace nasr_eng
extern "C" int nasr_engine_step(nasr_engine *e, nasr_stream *const *streams, int B, const int16_t *const *pcm,
                                const int32_t *n_samples, int32_t *const *tokens_out, const int32_t *tokens_cap,
                                int32_t *n_tokens, uint32_t flags) {
    ApiGuard api_guard;
    if (validate_batch(e, streams, B)) return -1;
    if (refuse_offline_flags(flags)) return -1;
    if (!pcm || !n_samples) return fail("null pcm / n_samples");
    for (int b = 0; b < B; b++)
        if (!streams[b]->default_format())
            return fail("stream %d has an audio format of its own (%d Hz, encoding %d, %d channel(s)): push it with nasr_engine_step_audio", b,
                        streams[b]->sample_rate, streams[b]->encoding, streams[b]->channels);
    HIPCHK(hipSetDevice(e->device));
    return step_s16(e, streams, B, pcm, n_samples, tokens_out, tokens_cap, n_tokens, flags);
}

static int check_audio_format(const nasr_audio_format *f) {
    if (!f) return fail("null audio format");
    nasr_rs::Plan p;
    if (!nasr_rs::make_plan(f->sample_rate, &p)) return fail("unsupported sample rate %d (8000, 11025, 16000, 22050, 24000, 32000, 44100 or 48000)", f->sample_rate);
    if (f->encoding < NASR_AUDIO_S16 || f->encoding > NASR_AUDIO_ALAW) return fail("unsupported audio encoding %d", f->encoding);
    if (f->channels < 1 || f->channels > nasr_rs::MAX_CHANNELS) return fail("unsupported channel count %d (1 .. %d)", f->channels, nasr_rs::MAX_CHANNELS);
    if (f->channel < -1 || f->channel >= f->channels) return fail("channel %d out of range (-1 = mean, 0 .. %d)", f->channel, f->channels - 1);
    return 0;
}

extern "C" int64_t nasr_audio_out_ready(const nasr_audio_format *f, int64_t n_frames_in) {
    if (check_audio_format(f)) return -1;
    if (n_frames_in < 0) return fail("negative frame count");
    nasr_rs::Plan p;
    nasr_rs::make_plan(f->sample_rate, &p);
    return nasr_rs::out_ready(p, n_frames_in);
}
extern "C" int64_t nasr_audio_out_total(const nasr_audio_format *f, int64_t n_frames_in) {
    if (check_audio_format(f)) return -1;
    if (n_frames_in < 0) return fail("negative frame count");
    nasr_rs::Plan p;
    nasr_rs::make_plan(f->sample_rate, &p);
    return nasr_rs::out_total(p, n_frames_in);
}

extern "C" int nasr_stream_set_audio_format(nasr_stream *s, const nasr_audio_format *f) {
    ApiGuard api_guard;
    if (!s) return fail("null stream");
    if (check_audio_format(f)) return -1;
    if (s->samples_in != 0 || s->aud_in != 0) return fail("the audio format is set before a stream's first audio (or right after a reset): this one has taken %lld input frames",
                                                          (long long)(s->aud_in ? s->aud_in : s->samples_in));
    nasr_engine *e = s->e;
    HIPCHK(hipSetDevice(e->device));
    nasr_rs::Plan p;
    nasr_rs::make_plan(f->sample_rate, &p);
    const float *table = nullptr;
    if (ensure_audio_table(e, p, &table)) return -1;
    s->sample_rate = f->sample_rate; s->encoding = f->encoding; s->channels = f->channels; s->channel = f->channel;
    s->aud_plan = p; s->aud_table = table;
    return 0;
}

extern "C" int nasr_engine_step_audio(nasr_engine *e, nasr_stream *const *streams, int B, const void *const *audio,
                                      const int32_t *n_frames, int32_t *const *tokens_out, const int32_t *tokens_cap,
                                      int32_t *n_tokens, uint32_t flags) {
    ApiGuard api_guard;
    if (validate_batch(e, streams, B)) return -1;
    if (refuse_offline_flags(flags)) return -1;
    if (!audio || !n_frames) return fail("null audio / n_frames");
    HIPCHK(hipSetDevice(e->device));
    bool all_default = true;
    for (int b = 0; b < B; b++) all_default = all_default && streams[b]->default_format();
    if (all_default) return step_s16(e, streams, B, (const int16_t *const *)audio, n_frames, tokens_out, tokens_cap, n_tokens, flags);
    std::vector<AudioDesc> descs((size_t)B);
    std::vector<size_t> raw_off((size_t)B, 0), raw_bytes((size_t)B, 0);
    size_t raw_total = 0;
    double flops = 0;
    for (int b = 0; b < B; b++) {
        nasr_stream *s = streams[b];
        if (n_frames[b] < 0) return fail("negative n_frames");
        if (n_frames[b] > 0 && !audio[b]) return fail("null audio for stream %d", b);
        if ((flags & NASR_FLAG_PCM_DEVICE) && ((uintptr_t)audio[b] % (size_t)nasr_rs::bytes_per_sample(s->encoding)))
            return fail("stream %d: device audio must be naturally aligned (2 bytes for s16, 4 for f32)", b);
        if (!s->aud_table && ensure_audio_table(e, s->aud_plan, &s->aud_table)) return -1;      // a default-format stream beside the others
        const long long n_out = std::max<long long>(0, nasr_rs::out_ready(s->aud_plan, s->aud_in + n_frames[b]) - s->aud_out);
        if (n_out > INT32_MAX) return fail("stream %d: the push completes more than 2^31 samples", b);
        fill_audio_desc(e, descs[b], s->aud_plan, s->fmt(), s->aud_table);
        descs[b].hist = e->aud_hist + (size_t)s->slot * 2 * nasr_rs::HIST_MAX; descs[b].par = s->aud_par;
        descs[b].n_before = s->aud_in; descs[b].n_push = n_frames[b]; descs[b].out_first = s->aud_out; descs[b].n_out = n_out;
        raw_bytes[b] = (size_t)n_frames[b] * s->channels * nasr_rs::bytes_per_sample(s->encoding);
        raw_off[b] = raw_total;
        raw_total += (raw_bytes[b] + 15) & ~(size_t)15;
        flops += audio_flops(s->aud_plan, (double)n_out);
    }
    if (!(flags & NASR_FLAG_PCM_DEVICE)) {
        // hand-over of host buffers as in nasr_engine_step: one gather into a rotating pinned block, one copy into the raw staging area
        if (grow_device(e, &e->raw_stage, &e->raw_stage_cap, raw_total, 65536)) return -1;
        PinBlock &pin = e->raw_pin[e->raw_pin_next++ & 3];
        if (pin.acquire(raw_total, 65536, e->st)) return -1;
        for (int b = 0; b < B; b++) {
            if (raw_bytes[b] > 0) memcpy(pin.p + raw_off[b], audio[b], raw_bytes[b]);
            descs[b].in = e->raw_stage + raw_off[b];
        }
        ProfScope ps(e, "h2d_pcm", (double)raw_total);
        if (pin.copy_to(e->raw_stage, raw_total, e->st)) return -1;
    } else {
        for (int b = 0; b < B; b++) descs[b].in = audio[b];
    }
    std::vector<const int16_t *> base((size_t)B, nullptr);
    std::vector<int32_t> n16((size_t)B, 0);
    if (run_audio_convert(e, descs, base, (double)raw_total, flops)) return -1;
    for (int b = 0; b < B; b++) {
        nasr_stream *s = streams[b];
        n16[b] = (int32_t)descs[b].n_out;
        s->aud_in += n_frames[b];
        s->aud_out += n16[b];
        if (n_frames[b] > 0) s->aud_par ^= 1;
    }
    return step_tail(e, streams, B, base.data(), n16.data(), tokens_out, tokens_cap, n_tokens, flags & ~(uint32_t)NASR_FLAG_PCM_DEVICE);
}

extern "C" int64_t nasr_engine_convert_audio(nasr_engine *e, const nasr_audio_format *f, const void *audio, int64_t n_frames,
                                             int16_t *out, int64_t cap, uint32_t flags) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    if (check_audio_format(f)) return -1;
    if (n_frames < 0 || n_frames > INT32_MAX) return fail("n_frames out of range");
    if (n_frames > 0 && (!audio || !out)) return fail("null audio / out");
    if ((flags & NASR_FLAG_PCM_DEVICE) && (((uintptr_t)audio % (size_t)nasr_rs::bytes_per_sample(f->encoding)) || ((uintptr_t)out & 1)))
        return fail("device audio / out must be naturally aligned (2 bytes for s16, 4 for f32)");
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    nasr_rs::Plan p;
    nasr_rs::make_plan(f->sample_rate, &p);
    const long long n_out = nasr_rs::out_total(p, n_frames);
    if (n_out > cap) return fail("output buffer too small (%lld > %lld)", n_out, (long long)cap);
    if (n_out == 0) return 0;
    const float *table = nullptr;
    if (ensure_audio_table(e, p, &table)) return -1;
    const bool on_device = (flags & NASR_FLAG_PCM_DEVICE) != 0;
    const size_t in_bytes = (size_t)n_frames * f->channels * nasr_rs::bytes_per_sample(f->encoding);
    void *din = nullptr, *dout = nullptr;
    int rc = 0;
    auto done = [&](int r) { if (!on_device) { if (din) hipFree(din); if (dout) hipFree(dout); } return r; };
    if (!on_device) {
        if (hipMalloc(&din, in_bytes) != hipSuccess || hipMalloc(&dout, (size_t)n_out * 2) != hipSuccess) return done(fail("hipMalloc failed (one-shot audio conversion)"));
        if (hipMemcpyAsync(din, audio, in_bytes, hipMemcpyHostToDevice, e->st) != hipSuccess) return done(fail("hipMemcpyAsync failed (one-shot audio conversion)"));
    }
    std::vector<AudioDesc> descs(1);
    fill_audio_desc(e, descs[0], p, *f, table);
    descs[0].in = on_device ? audio : din; descs[0].out = on_device ? out : (int16_t *)dout;
    descs[0].n_push = n_frames; descs[0].n_out = n_out;
    const AudioDesc *dd;
    if (stage_desc(e, descs, &dd)) return done(-1);
    {
        ProfScope ps(e, "audio_convert", (double)in_bytes + (double)n_out * 2, audio_flops(p, (double)n_out));
        launch_audio_convert(dd, 1, n_out, e->st);
        if (hipGetLastError() != hipSuccess) return done(fail("k_audio_convert launch failed (one-shot audio conversion)"));
    }
    if (!on_device && hipMemcpyAsync(out, dout, (size_t)n_out * 2, hipMemcpyDeviceToHost, e->st) != hipSuccess) rc = fail("hipMemcpyAsync failed (one-shot audio conversion)");
    if (hipStreamSynchronize(e->st) != hipSuccess) rc = fail("one-shot audio conversion failed on the device");
    return done(rc ? -1 : (int64_t)n_out);
}

extern "C" int nasr_engine_step_mel(nasr_engine *e, nasr_stream *const *streams, int B, const float *const *mel,
                                    const int32_t *n_frames, int32_t *const *tokens_out, const int32_t *tokens_cap,
                                    int32_t *n_tokens, uint32_t flags) {
    ApiGuard api_guard;
    if (validate_batch(e, streams, B)) return -1;
    if (refuse_offline_flags(flags)) return -1;
    if (!mel || !n_frames) return fail("null mel / n_frames");
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    std::vector<int> off(B, 0);
    const int piece = 8 * streams[0]->T;   // one shift at a time keeps the ring bounded
    for (;;) {
        std::vector<PcmDesc> pd;
        std::vector<int> who;
        for (int b = 0; b < B; b++) {
            if (n_frames[b] < 0 || (n_frames[b] > 0 && !mel[b])) return fail("bad mel input for stream %d", b);
            const int rem = n_frames[b] - off[b];
            if (rem <= 0) continue;
            PcmDesc d;
            memset(&d, 0, sizeof(d));
            d.slot = streams[b]->slot;
            d.n_frames = std::min(rem, piece);
            d.mel_wpos = (streams[b]->mel_start + streams[b]->mel_count) & (MEL_RING - 1);
            pd.push_back(d);
            who.push_back(b);
        }
        if (pd.empty()) break;
        const size_t need = pd.size() * (size_t)piece * NMEL;
        if (grow_device(e, &e->mel_stage, &e->mel_stage_cap, need, 0)) return -1;
        for (size_t i = 0; i < pd.size(); i++)
            HIPCHK(hipMemcpyAsync(e->mel_stage + i * (size_t)piece * NMEL, mel[who[i]] + (size_t)off[who[i]] * NMEL,
                                  (size_t)pd[i].n_frames * NMEL * 4, hipMemcpyHostToDevice, e->st));
        const PcmDesc *dpd;
        if (stage_desc(e, pd, &dpd)) return -1;
        launch_mel_put(e->mel_stage, dpd, (int)pd.size(), piece, e->mel_ring, e->st);
        for (size_t i = 0; i < pd.size(); i++) {
            off[who[i]] += pd[i].n_frames;
            streams[who[i]]->mel_count += pd[i].n_frames;
        }
        if (drain_chunks(e, streams, B)) return -1;
        HIPCHK(hipStreamSynchronize(e->st));   // host mel staging is reused next round
    }
    if (flags & NASR_FLAG_NO_SYNC) {
        if (n_tokens) for (int b = 0; b < B; b++) n_tokens[b] = 0;
        return 0;
    }
    return collect_tokens(e, streams, B, tokens_out, tokens_cap, n_tokens);
}

namespace nasr_eng {
int finalize_flush(nasr_engine *e, nasr_stream *const *streams, int B) {
    if (audio_flush(e, streams, B)) return -1;          // streams with an audio format of their own: the converter's tail goes through the front end first
    // src/nemo-stream.cpp:1234-1258: frames > 9 -> n_valid = (frames-9)/8 outputs of one zero-padded step
    std::vector<nasr_stream *> rows;
    std::vector<int> nd;
    std::vector<PcmDesc> pd;
    int max_pad = 0;
    for (int b = 0; b < B; b++) {
        nasr_stream *s = streams[b];
        const int chunk_mel = PRE_CACHE + 8 * s->T;
        if (s->mel_count <= PRE_CACHE) continue;
        const int n_valid = (s->mel_count - PRE_CACHE) / 8;
        if (n_valid <= 0) continue;
        if (s->mel_count < chunk_mel) {
            PcmDesc d;
            memset(&d, 0, sizeof(d));
            d.slot = s->slot;
            d.n_frames = chunk_mel - s->mel_count;
            d.mel_wpos = (s->mel_start + s->mel_count) & (MEL_RING - 1);
            pd.push_back(d);
            max_pad = std::max(max_pad, d.n_frames);
            s->mel_count = chunk_mel;
        }
        rows.push_back(s);
        nd.push_back(std::min(n_valid, s->T));
    }
    if (!pd.empty()) {
        const PcmDesc *dpd;
        if (stage_desc(e, pd, &dpd)) return -1;
        launch_mel_zero(dpd, (int)pd.size(), max_pad, e->mel_ring, e->st);
    }
    if (!rows.empty() && run_chunk(e, rows, nd)) return -1;
    return 0;
}
}  // namespace nasr_eng

extern "C" int nasr_engine_finalize(nasr_engine *e, nasr_stream *const *streams, int B, int32_t *const *tokens_out,
                                    const int32_t *tokens_cap, int32_t *n_tokens) {
    ApiGuard api_guard;
    if (validate_batch(e, streams, B)) return -1;
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    if (finalize_flush(e, streams, B)) return -1;
    return collect_tokens(e, streams, B, tokens_out, tokens_cap, n_tokens);
}

// the steps in flight are completed, every stream is forked into a free slot, the forks take the finalize path as one batch, their new tokens
// are read and their slots released: the streams themselves (device state, host mirror, queued tokens) are not touched
extern "C" int nasr_engine_preview(nasr_engine *e, nasr_stream *const *streams, int B, int32_t *const *tokens_out, const int32_t *tokens_cap,
                                   int32_t *n_tokens, int32_t *const *frames_out) {
    ApiGuard api_guard;
    if (validate_batch(e, streams, B)) return -1;
    if (!n_tokens) return fail("nasr_engine_preview: null n_tokens");
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    int n_free = 0;
    for (int i = 0; i < e->max_streams; i++) n_free += e->slots[i] == nullptr;
    if (n_free < B) return fail("nasr_engine_preview: %d free slot(s) missing: %d stream(s) need as many, %d of max_streams=%d are free", B - n_free, B, n_free, e->max_streams);
    std::vector<nasr_stream *> forks;
    // a debug engine stages NASR_TAP_MEL (by batch row) and NASR_TAP_PCM16 per call: what the sources' last call left there is set aside and
    // put back, so that their taps read after the preview what they read before it (debug only: two allocations and four copies)
    struct TapSave { void *mel = nullptr, *pcm = nullptr; size_t mel_bytes = 0, pcm_bytes = 0; std::vector<int> frames, row; std::vector<int64_t> off, n; } taps;
    if (e->debug && e->tap_mel) {
        taps.mel_bytes = (size_t)B * e->tap_mel_cap * NMEL * 4; taps.pcm_bytes = e->tap_pcm_cap * 2;
        taps.frames = e->tap_mel_frames; taps.row = e->tap_mel_row; taps.off = e->tap_pcm_off; taps.n = e->tap_pcm_n;
        HIPCHK(hipStreamSynchronize(e->st));
        HIPCHK(hipMalloc(&taps.mel, taps.mel_bytes));
        if (hipMemcpy(taps.mel, e->tap_mel, taps.mel_bytes, hipMemcpyDeviceToDevice) != hipSuccess) { hipFree(taps.mel); return fail("nasr_engine_preview: saving the mel tap failed"); }
        if (taps.pcm_bytes && (hipMalloc(&taps.pcm, taps.pcm_bytes) != hipSuccess || hipMemcpy(taps.pcm, e->tap_pcm, taps.pcm_bytes, hipMemcpyDeviceToDevice) != hipSuccess)) {
            hipFree(taps.mel); if (taps.pcm) hipFree(taps.pcm);
            return fail("nasr_engine_preview: saving the PCM16 tap failed");
        }
    }
    const auto release = [&](int rc) {
        if (rc) pipe_drain(e);                             // a failed call: nothing in flight may still name a fork
        hipStreamSynchronize(e->st);
        for (nasr_stream *f : forks) { e->slots[f->slot] = nullptr; stream_unregister(f); delete f; }
        if (taps.mel) {                                    // tap_pcm only ever grows: the saved bytes fit
            hipMemcpy(e->tap_mel, taps.mel, taps.mel_bytes, hipMemcpyDeviceToDevice);
            if (taps.pcm) hipMemcpy(e->tap_pcm, taps.pcm, taps.pcm_bytes, hipMemcpyDeviceToDevice);
            e->tap_mel_frames = taps.frames; e->tap_mel_row = taps.row; e->tap_pcm_off = taps.off; e->tap_pcm_n = taps.n;
            hipFree(taps.mel); if (taps.pcm) hipFree(taps.pcm);
        }
        return rc;
    };
    for (int b = 0; b < B; b++) {
        nasr_stream *f = nullptr;
        if (stream_fork(streams[b], &f)) return release(-1);
        forks.push_back(f);
    }
    // what the sources had decoded before (queued on the host, or still on the device behind a NO_SYNC step) is not part of the tail
    if (collect_tokens(e, forks.data(), B, nullptr, nullptr, nullptr)) return release(-1);
    if (finalize_flush(e, forks.data(), B)) return release(-1);
    std::vector<std::vector<int32_t>> toks((size_t)B, std::vector<int32_t>(TOK_CAP));
    std::vector<int32_t *> tptr((size_t)B);
    std::vector<int32_t> tcap((size_t)B, TOK_CAP), tn((size_t)B, 0);
    for (int b = 0; b < B; b++) tptr[b] = toks[b].data();
    if (collect_tokens(e, forks.data(), B, tptr.data(), tcap.data(), tn.data())) return release(-1);      // synchronises the engine's stream
    for (int b = 0; b < B; b++) {
        n_tokens[b] = tn[b];
        const int n_out = tokens_cap ? std::min(tn[b], std::max(tokens_cap[b], 0)) : 0;
        if (tokens_out && tokens_out[b]) for (int i = 0; i < n_out; i++) tokens_out[b][i] = toks[b][(size_t)i];
        if (!frames_out || !frames_out[b] || n_out <= 0) continue;
        // only the tail's entries of the fork's frame ring: one copy, two where they wrap (tok_read = the fork's token count once its tail is collected)
        const int *ring = e->dec.tok_frame + (size_t)forks[b]->slot * TOK_CAP;
        const int first = (forks[b]->tok_read - tn[b]) & (TOK_CAP - 1), n1 = std::min(n_out, TOK_CAP - first);
        if (hipMemcpy(frames_out[b], ring + first, (size_t)n1 * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
            (n_out > n1 && hipMemcpy(frames_out[b] + n1, ring, (size_t)(n_out - n1) * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess))
            return release(fail("nasr_engine_preview: reading the token frames failed"));
    }
    e->stream_previews++;
    return release(0);
}

extern "C" int nasr_engine_collect(nasr_engine *e, nasr_stream *const *streams, int B, int32_t *const *tokens_out,
                                   const int32_t *tokens_cap, int32_t *n_tokens) {
    ApiGuard api_guard;
    if (validate_batch(e, streams, B)) return -1;
    HIPCHK(hipSetDevice(e->device));
    return collect_tokens(e, streams, B, tokens_out, tokens_cap, n_tokens);
}

// ---- the read-out rings of the device decode: token frames, token log-probabilities, per-frame blank log-probabilities, top-K alternatives.
// One read for the four getters: the steps in flight completed and the slot's DecCtrl fetched (ring_ctrl), the range clamped to what the
// device has produced or found older than the ring (nasr_step::ring_window), the slot's ring copied and un-wrapped (ring_copy).  The getters
// keep what differs: the option that gates them, what counts as produced, and what "older than the ring" returns
namespace nasr_eng {
static int ring_ctrl(const nasr_stream *s, DecCtrl &c) {
    nasr_engine *e = s->e;
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    HIPCHK(hipStreamSynchronize(e->st));
    HIPCHK(hipMemcpy(&c, e->dec.ctrl + s->slot, sizeof(c), hipMemcpyDeviceToHost));
    return 0;
}
// items first .. first + count - 1 of the slot's ring of cap items (a power of two) of `stride` elements each -> out; returns count
template <typename Tp>
static int ring_copy(const nasr_stream *s, const Tp *rings, int cap, int stride, int64_t first, int count, Tp *out) {
    if (count <= 0) return 0;
    std::vector<Tp> ring((size_t)cap * stride);
    HIPCHK(hipMemcpy(ring.data(), rings + (size_t)s->slot * ring.size(), ring.size() * sizeof(Tp), hipMemcpyDeviceToHost));
    for (int i = 0; i < count; i++) memcpy(out + (size_t)i * stride, ring.data() + (size_t)((first + i) & (cap - 1)) * stride, (size_t)stride * sizeof(Tp));
    return count;
}
// the clamped range of a per-token ring, or the refusal of one whose first token has left it
static int token_window(const DecCtrl &c, int64_t first, int count) {
    count = ring_window(first, count, c.n_tok, TOK_CAP);
    return count == RING_TOO_OLD ? fail("token %lld is older than the %d-token device ring", (long long)first, TOK_CAP) : count;
}
}  // namespace nasr_eng

extern "C" int nasr_stream_get_token_frames(const nasr_stream *s, int64_t first, int32_t count, int32_t *frames_out) {
    ApiGuard api_guard;
    if (!s || (count > 0 && !frames_out)) return fail("null argument");
    if (first < 0 || count < 0) return fail("negative token range");
    DecCtrl c;
    if (ring_ctrl(s, c) || (count = token_window(c, first, count)) < 0) return -1;
    return ring_copy(s, s->e->dec.tok_frame, TOK_CAP, 1, first, count, frames_out);
}

extern "C" int nasr_stream_get_token_logprobs(const nasr_stream *s, int64_t first, int32_t count, float *out) {
    ApiGuard api_guard;
    if (!s || (count > 0 && !out)) return fail("null argument");
    if (first < 0 || count < 0) return fail("negative token range");
    if (!s->e->opt_token_logprobs) return fail("no token log-probabilities: engine option \"token_logprobs\" is off (set it to 1 before the first step)");
    DecCtrl c;
    if (ring_ctrl(s, c) || (count = token_window(c, first, count)) < 0) return -1;
    return ring_copy(s, s->e->dec.tok_logprob, TOK_CAP, 1, first, count, out);
}

extern "C" int nasr_stream_get_token_entropies(const nasr_stream *s, int64_t first, int32_t count, float *out) {
    ApiGuard api_guard;
    if (!s || (count > 0 && !out)) return fail("null argument");
    if (first < 0 || count < 0) return fail("negative token range");
    if (!s->e->opt_token_entropy) return fail("no token entropies: engine option \"token_entropy\" is off (set it to round(1000 alpha) before the first step)");
    DecCtrl c;
    if (ring_ctrl(s, c) || (count = token_window(c, first, count)) < 0) return -1;
    return ring_copy(s, s->e->dec.tok_entropy, TOK_CAP, 1, first, count, out);
}

extern "C" int nasr_stream_get_frame_blank_logprobs(const nasr_stream *s, int64_t first, int32_t count, float *out) {
    ApiGuard api_guard;
    if (!s) return fail("null argument");
    if (first < 0 || count < 0) return fail("negative frame range");
    if (!s->e->opt_frame_blank) return fail("no per-frame blank log-probabilities: engine option \"frame_blank_logprobs\" is off (set it to 1 before the first step)");
    DecCtrl c;
    if (ring_ctrl(s, c)) return -1;
    const int64_t n_frames = (int64_t)c.frame0 + c.t;          // frames the decode has left since create / reset
    if (!out) return (int)n_frames;
    count = ring_window(first, count, n_frames, FRAME_CAP);
    if (count == RING_TOO_OLD) return 0;                       // the range starts before the most recent FRAME_CAP frames: nothing of it can be written from its first frame on
    return ring_copy(s, s->e->dec.frame_blank, FRAME_CAP, 1, first, count, out);
}

// ---- engine option "frame_history" (nasr_history.h): the kept range of a stream and the parity read-out of its rows
extern "C" int nasr_stream_history_range(const nasr_stream *s, int64_t *first_out, int32_t *count_out) {
    ApiGuard api_guard;
    if (!s || !first_out || !count_out) return fail("null argument");
    if (!s->e->opt_frame_history) return fail("%s", HISTORY_OFF);
    DecCtrl c;
    if (ring_ctrl(s, c)) return -1;
    const nasr_hist::Range r = nasr_hist::retained(s->hist_valid_from, (int64_t)c.frame0 + c.t, s->e->opt_frame_history);
    *first_out = r.first; *count_out = r.count;
    return 0;
}

extern "C" int nasr_stream_get_history(const nasr_stream *s, int64_t first, int32_t count, float *out) {
    ApiGuard api_guard;
    if (!s || (count > 0 && !out)) return fail("null argument");
    if (first < 0 || count < 0) return fail("negative frame range");
    nasr_engine *e = s->e;
    const int N = e->opt_frame_history;
    if (!N) return fail("%s", HISTORY_OFF);
    DecCtrl c;
    if (ring_ctrl(s, c)) return -1;
    if (count == 0 || !nasr_hist::window_kept(nasr_hist::retained(s->hist_valid_from, (int64_t)c.frame0 + c.t, N), first, count)) return 0;
    // the window's runs in the slot's ring: one copy, two where it crosses the wrap
    const nasr_hist::Runs r = nasr_hist::ring_runs(first, count, N);
    const float *ring = e->hist_ring + (size_t)s->slot * N * nasr_hist::ROW_FLOATS;
    HIPCHK(hipMemcpy(out, ring + (size_t)r.row0 * nasr_hist::ROW_FLOATS, (size_t)r.n0 * nasr_hist::ROW_BYTES, hipMemcpyDeviceToHost));
    if (r.n1 > 0) HIPCHK(hipMemcpy(out + (size_t)r.n0 * nasr_hist::ROW_FLOATS, ring, (size_t)r.n1 * nasr_hist::ROW_BYTES, hipMemcpyDeviceToHost));
    return count;
}

extern "C" int nasr_stream_get_token_alternatives(const nasr_stream *s, int64_t first, int32_t count, int32_t *ids_out, float *logprobs_out) {
    ApiGuard api_guard;
    if (!s || (count > 0 && (!ids_out || !logprobs_out))) return fail("null argument");
    if (first < 0 || count < 0) return fail("negative token range");
    const int K = s->e->opt_token_alt;
    if (!K) return fail("no token alternatives: engine option \"token_alternatives\" is off (set it to K = 1 .. 8 before the first step)");
    DecCtrl c;
    if (ring_ctrl(s, c) || (count = token_window(c, first, count)) < 0) return -1;
    if (ring_copy(s, s->e->dec.alt_id, TOK_CAP, K, first, count, ids_out) < 0) return -1;
    return ring_copy(s, s->e->dec.alt_lp, TOK_CAP, K, first, count, logprobs_out);
}

// host-side counters.  Walks the graph caches without a lock: call it from the thread that steps the engine (as every entry point that
// takes an engine or a stream: one thread per engine; the server's worker prints them at exit)
extern "C" int nasr_engine_get_counter(const nasr_engine *e, const char *name, int64_t *value) {
    if (!e || !name || !value) return fail("null argument");
    int64_t execs = (int64_t)e->graphs.size(), shapes = (int64_t)e->graphs.size();
    std::map<int64_t, int> keys;
    for (int p = 0; p < nasr_engine::NSLOT; p++) {
        for (auto &m : e->pipe[p].seg_graphs) for (auto &kv : m) { execs += kv.second != nullptr; keys[kv.first] = 1; }
        for (auto &kv : e->pipe[p].dec_graphs) execs += kv.second != nullptr;
    }
    shapes += (int64_t)keys.size();
    for (auto &per_slot : e->gp_graphs) for (auto &m : per_slot) execs += (int64_t)m.size();
    if (!strcmp(name, "graph_execs")) *value = execs;
    else if (!strcmp(name, "graph_shapes")) *value = shapes;
    else if (!strcmp(name, "graph_evictions")) *value = e->graph_evictions;
    else if (!strcmp(name, "graph_replays")) *value = e->graph_replays;
    else if (!strcmp(name, "decode_fallbacks")) *value = e->decode_fallbacks;              // graph steps whose decode was completed eagerly ...
    else if (!strcmp(name, "decode_fallback_rounds")) *value = e->decode_fallback_rounds;  // ... and the host round trips that took
    else if (!strcmp(name, "eager_steps")) *value = e->eager_steps;
    else if (!strcmp(name, "pipelined_steps")) *value = e->pipe_steps;
    else if (!strcmp(name, "grouped_steps")) *value = e->gp_steps;
    else if (!strcmp(name, "stream_forks")) *value = e->stream_forks;                       // k_stream_fork launches: nasr_stream_fork calls and the forks of every preview
    else if (!strcmp(name, "stream_previews")) *value = e->stream_previews;                 // nasr_engine_preview calls that succeeded
    else if (!strcmp(name, "stream_saves")) *value = e->stream_saves;                       // nasr_stream_save calls that wrote a blob (one k_stream_pack launch each)
    else if (!strcmp(name, "stream_restores")) *value = e->stream_restores;                 // nasr_stream_restore calls that made a stream (refused ones are not counted)
    else if (!strcmp(name, "history_calls")) *value = e->history_calls;                     // nasr_engine_history_* calls that succeeded
    else if (!strcmp(name, "history_frames")) *value = e->history_frames;                   // frames those calls gathered out of the rings
    else if (!strcmp(name, "cut_drains")) *value = e->cut_drains;                          // pipelined steps that first completed the steps in flight: cut differently (piece count, family)
    else if (!strcmp(name, "boost_states")) *value = e->opt_phrase_boost ? e->boost_states : 0;      // automaton states of the current boost set
    else if (!strcmp(name, "lm_ngrams")) *value = e->lm ? e->lm->n_ngrams : 0;                        // the attached language model (0: none)
    else if (!strcmp(name, "lm_states")) *value = e->lm ? (int64_t)e->lm->states.size() : 0;
    else if (!strcmp(name, "lm_max_probe")) *value = e->lm ? e->lm->max_probe : 0;
    else if (!strcmp(name, "lanes")) *value = e->pipe_ready ? e->n_lanes : 0;      // HIP streams found to overlap (0: not picked yet)
    else return fail("unknown counter '%s'", name);
    return 0;
}

// host mirror only: no pipeline drain, no stream synchronisation, no copy (the per-call path of a server)
extern "C" int nasr_stream_get_progress(const nasr_stream *s, nasr_stream_stats *out) {
    if (!s || !out) return fail("null argument");
    memset(out, 0, sizeof(*out));
    out->samples_in = s->samples_in;
    out->chunks = s->chunks;
    out->decode_iterations = -1;               // device counters: nasr_stream_get_stats
    out->tokens = -1;
    out->cache_valid_len = s->valid_len;
    out->mel_frames_buffered = s->mel_count;
    out->reserved = (int32_t)s->tok_queue.size();   // tokens decoded but not yet handed to the caller
    return 0;
}

extern "C" int nasr_stream_get_stats(const nasr_stream *s, nasr_stream_stats *out) {
    ApiGuard api_guard;
    if (!s || !out) return fail("null argument");
    nasr_engine *e = s->e;
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    DecCtrl c;
    HIPCHK(hipStreamSynchronize(e->st));
    HIPCHK(hipMemcpy(&c, e->dec.ctrl + s->slot, sizeof(c), hipMemcpyDeviceToHost));
    memset(out, 0, sizeof(*out));
    out->samples_in = s->samples_in;
    out->chunks = s->chunks;
    out->decode_iterations = c.iterations;
    out->tokens = c.n_tok;
    out->cache_valid_len = s->valid_len;
    out->mel_frames_buffered = s->mel_count;
    return 0;
}

extern "C" int64_t nasr_stream_get_tap(nasr_stream *s, int which, int index, float *out, int64_t cap) {
    ApiGuard api_guard;
    if (!s || !out) return fail("null argument");
    nasr_engine *e = s->e;
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    HIPCHK(hipStreamSynchronize(e->st));
    const size_t slot = (size_t)s->slot;
    const int T = s->last_T;
    auto need_debug = [&]() { return e->tap_sub != nullptr; };
    switch (which) {
    case NASR_TAP_MEL: {
        if (!need_debug()) return fail("debug taps not enabled");
        const int n = std::min(e->tap_mel_frames[slot], e->tap_mel_cap);
        if ((int64_t)n * NMEL > cap) return fail("tap buffer too small");
        HIPCHK(hipMemcpy(out, e->tap_mel + (size_t)e->tap_mel_row[slot] * e->tap_mel_cap * NMEL, (size_t)n * NMEL * 4, hipMemcpyDeviceToHost));
        return (int64_t)n * NMEL;
    }
    case NASR_TAP_SUBSAMPLED:
    case NASR_TAP_ENCODER_OUT:
    case NASR_TAP_LAYER_OUT: {
        if ((int64_t)T * D > cap) return fail("tap buffer too small");
        if (which == NASR_TAP_ENCODER_OUT && !(e->debug && need_debug())) {
            // without debug buffers: valid until the next chunk step of this engine
            if (e->hp.num_prompts > 0 || T == 0) return fail("encoder-out tap needs debug mode here");
            HIPCHK(hipMemcpy(out, e->ws[s->last_ws].x + (size_t)s->last_row * T * D, (size_t)T * D * 4, hipMemcpyDeviceToHost));
            return (int64_t)T * D;
        }
        if (!need_debug()) return fail("debug taps not enabled");
        const float *src = which == NASR_TAP_SUBSAMPLED ? e->tap_sub + slot * TMAX * D
                         : which == NASR_TAP_ENCODER_OUT ? e->tap_enc + slot * TMAX * D
                         : e->tap_layers + (slot * e->hp.n_layers + (size_t)index) * TMAX * D;
        if (which == NASR_TAP_LAYER_OUT && (index < 0 || index >= e->hp.n_layers)) return fail("layer index out of range");
        HIPCHK(hipMemcpy(out, src, (size_t)T * D * 4, hipMemcpyDeviceToHost));
        return (int64_t)T * D;
    }
    case NASR_TAP_K_CACHE:
    case NASR_TAP_V_CACHE: {
        if (index < 0 || index >= e->hp.n_layers) return fail("layer index out of range");
        if ((int64_t)LCTX * D > cap) return fail("tap buffer too small");
        const int v = which == NASR_TAP_V_CACHE ? 1 : 0;
        std::vector<char> raw((size_t)KVC * D * e->esz);
        HIPCHK(hipMemcpy(raw.data(), (char *)e->kv_pool[index] + (slot * 2 + v) * KVC * D * e->esz, raw.size(), hipMemcpyDeviceToHost));
        for (int j = 0; j < LCTX; j++) {   // logical order: ring[(kv_head + j) % KVC]
            const int ring = (s->kv_head + j) % KVC;
            if (j < LCTX - s->valid_len) {     // not cached yet: the reference's tensor holds its initial zeros there (src/nemo-stream.cpp:320-325); here the
                for (int d = 0; d < D; d++) out[(size_t)j * D + d] = 0.0f;      // ring may hold an earlier stream's rows, which no kernel ever weighs (the mask)
                continue;
            }
            for (int d = 0; d < D; d++) {
                if (e->bf16) {
                    uint32_t u = (uint32_t)((const uint16_t *)raw.data())[(size_t)ring * D + d] << 16;
                    memcpy(&out[(size_t)j * D + d], &u, 4);
                } else out[(size_t)j * D + d] = ((const float *)raw.data())[(size_t)ring * D + d];
            }
        }
        return (int64_t)LCTX * D;
    }
    case NASR_TAP_CONV_CACHE: {
        if (index < 0 || index >= e->hp.n_layers) return fail("layer index out of range");
        const size_t ks1 = (size_t)e->hp.kernel_size - 1;
        if ((int64_t)(ks1 * D) > cap) return fail("tap buffer too small");
        HIPCHK(hipMemcpy(out, e->cc_pool[index] + (slot * 2 + s->cc_par) * ks1 * D, ks1 * D * 4, hipMemcpyDeviceToHost));
        return (int64_t)(ks1 * D);
    }
    case NASR_TAP_PCM16: {
        if (!e->debug) return fail("debug taps not enabled");
        const int64_t n = e->tap_pcm_n[slot];
        if (n > cap) return fail("tap buffer too small");
        std::vector<int16_t> h((size_t)n);
        if (n > 0) HIPCHK(hipMemcpy(h.data(), e->tap_pcm + e->tap_pcm_off[slot], (size_t)n * 2, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; i++) out[i] = (float)h[(size_t)i];
        return n;
    }
    case NASR_TAP_DEC_STATE: {
        if (cap < 4 * HID + 1) return fail("tap buffer too small");
        DecCtrl c;
        HIPCHK(hipMemcpy(&c, e->dec.ctrl + slot, sizeof(c), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out, e->dec.h + (slot * 2 + c.cur) * 2 * HID, 2 * HID * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out + 2 * HID, e->dec.c + (slot * 2 + c.cur) * 2 * HID, 2 * HID * 4, hipMemcpyDeviceToHost));
        out[4 * HID] = (float)c.prev_token;
        return 4 * HID + 1;
    }
    }
    return fail("unknown tap %d", which);
}

// test hook: every K/V ring row of the stream's slot, in every layer, := value (see the header)
extern "C" int nasr_stream_debug_fill_kv(nasr_stream *s, float value) {
    ApiGuard api_guard;
    if (!s) return fail("null stream");
    nasr_engine *e = s->e;
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    const size_t n = (size_t)2 * KVC * D;
    std::vector<char> host(n * e->esz);
    for (size_t i = 0; i < n; i++) {
        const float v = (i & 1) ? -value : value;
        if (e->bf16) { uint32_t u; memcpy(&u, &v, 4); ((uint16_t *)host.data())[i] = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16); }
        else ((float *)host.data())[i] = v;
    }
    HIPCHK(hipStreamSynchronize(e->st));
    for (int l = 0; l < e->hp.n_layers; l++)
        HIPCHK(hipMemcpy((char *)e->kv_pool[l] + (size_t)s->slot * n * e->esz, host.data(), host.size(), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int nasr_engine_profile(nasr_engine *e, int enable) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    prof_flush(e);
    if (enable) for (auto &s : e->prof.stats) { s.launches = 0; s.total_ms = 0; s.bytes = 0; s.flops = 0; }
    e->prof.on = enable != 0;
    return 0;
}

extern "C" int nasr_engine_profile_read(nasr_engine *e, nasr_kernel_stat *out, int cap) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    HIPCHK(hipSetDevice(e->device));
    prof_flush(e);
    int n = 0;
    for (auto &s : e->prof.stats) {
        if (s.launches == 0) continue;
        if (out && n < cap) out[n] = s;
        n++;
    }
    return n;
}

extern "C" void *nasr_engine_hip_stream(nasr_engine *e) { return e ? (void *)e->st : nullptr; }

// hands the LAST of the engine's side-by-side streams (its hardware queue) to another GPU client of the process, e.g. the
// diarization side-car (nasr_diar_set_stream): the engine keeps one stream fewer (one encoder piece fewer at most) and still
// owns the stream -- the borrower must be done with it before nasr_engine_destroy
extern "C" int nasr_engine_lend_stream(nasr_engine *e, void **out) {
    ApiGuard api_guard;
    if (!e || !out) return fail("null argument");
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;
    if (!e->pipe_ready) {
        if (pick_lanes(e)) return -1;
        e->pipe_ready = true;
        release_lanes(e);
    }
    if (e->n_lanes < 2) return fail("no side-by-side stream to lend (the engine found %d)", e->n_lanes);
    e->n_lanes--;
    e->lent.push_back(e->lane[e->n_lanes]);          // destroyed with the engine, unless a borrower still holds it then
    lent_stream_register(e->lane[e->n_lanes]);
    *out = (void *)e->lane[e->n_lanes];
    e->lane[e->n_lanes] = nullptr;
    return 0;
}

extern "C" int nasr_device_alloc(nasr_engine *e, void **out, int64_t bytes) {
    ApiGuard api_guard;
    if (!e || !out || bytes <= 0) return fail("bad argument");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMalloc(out, (size_t)bytes));
    return 0;
}
extern "C" int nasr_device_free(nasr_engine *e, void *p) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipFree(p));
    return 0;
}
extern "C" int nasr_device_upload(nasr_engine *e, void *dst, const void *src, int64_t bytes) {
    ApiGuard api_guard;
    if (!e || !dst || !src) return fail("bad argument");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice));
    return 0;
}
extern "C" int nasr_engine_synchronize(nasr_engine *e) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;                       // the decode graph in flight, if any (its tokens stay queued)
    HIPCHK(hipStreamSynchronize(e->st));
    return 0;
}

