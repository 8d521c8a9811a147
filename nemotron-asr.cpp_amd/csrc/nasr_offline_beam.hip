// nasr_offline_beam.hip -- frame-synchronous beam search, N-best transcripts with scores (nasr_engine_transcribe_beam*): the beam mode of an
// offline call (nasr_offline_state.h: offline_call) and the hypotheses' read-outs.  Rules: nasr_beam.h; kernels: kernels_beam.hip.
#include "nasr_offline_state.h"

namespace nasr_eng {

// the search over one sub-batch whose encoder projection is in o->encproj: T_max * (S + 1) rounds enqueued blind, five launches each (the
// decode's two LSTM layers, joint.pred and tiled joint, then k_beam_select), no host round trip inside
static int beam_batch(nasr_engine *e, OfflineState *o, const OffBatch &ob, int W, int N, int S) {
    hipStream_t st = e->st;
    const bool boost = o->beam_boost, totals = boost || e->lm;   // boosted: the BOOST kernel forms, their buffers and the final key with or without an LM
    std::vector<int> live;
    std::vector<BeamUtt> ud;
    long long nodes = 0, outs = 0;
    int maxT = 0;
    for (int k = 0; k < ob.n; k++) {
        const int b = ob.first + k;
        if (ob.T[k] == 0) {                                   // no frame: the empty hypothesis, score 0 (with an LM: its EOS term alone)
            OfflineState::BeamHyp h{0.0, {}, {}, {}};
            if (e->lm) {
                const nasr_lm::View v = e->lm->view();
                int32_t next = 0;
                nasr_beam::Hyp z;
                z.score = 0.0; z.len = 0;
                z.lm = h.lm_final = v.has_eos ? nasr_lm::lookup(v, v.start, nasr_lm::EOS, &next) : 0.0;
                h.total = nasr_beam::total_of<true>(z, e->lm_weight, e->lm_bonus);
            }
            if (boost) h.total = nasr_beam::boosted_total(h.total, 0.0);       // no token: boost 0
            o->beam_res[b].assign(1, h);
            continue;
        }
        BeamUtt u;
        u.enc_row = ob.off[k]; u.T = ob.T[k]; u.node0 = nodes; u.out0 = outs;
        nodes += nasr_beam::node_bound(u.T, W, S);
        outs += (long long)N * u.T * S;
        maxT = std::max(maxT, u.T);
        ud.push_back(u); live.push_back(k);
    }
    const int n = (int)live.size();
    if (n == 0) return 0;
    const size_t rows = (size_t)n * W, slots = (size_t)n * nasr_beam::n_slots(W);
    if (grow(e, o, o->bm_utt, n * sizeof(BeamUtt)) || grow(e, o, o->bm_beam, n * sizeof(nasr_beam::Beam)) ||
        grow(e, o, o->bm_nodes, (size_t)nodes * sizeof(nasr_beam::Node)) || grow(e, o, o->bm_enc, rows * JNT * 4) ||
        grow(e, o, o->bm_rows, rows * sizeof(RowDesc)) || grow(e, o, o->bm_ctrl, slots * sizeof(DecCtrl)) ||
        grow(e, o, o->bm_h, slots * 4 * HID * 4) || grow(e, o, o->bm_c, slots * 4 * HID * 4) || grow(e, o, o->bm_predg, slots * JNT * 4) ||
        grow(e, o, o->bm_key, rows * 8) || grow(e, o, o->bm_part, rows * nasr_lp::WG_PARTS * sizeof(nasr_lp::Part)) ||
        grow(e, o, o->bm_alt, rows * nasr_lp::WG_PARTS * nasr_beam::KTOP * 8) || grow(e, o, o->bm_cnt, 8 * 4) ||
        grow(e, o, o->bm_dlist, rows * 4) || grow(e, o, o->bm_rowmap, rows * 4) || grow(e, o, o->bm_out_n, n * 4) ||
        grow(e, o, o->bm_out_len, (size_t)n * nasr_beam::WMAX * 4) || grow(e, o, o->bm_out_score, (size_t)n * nasr_beam::WMAX * 8) ||
        grow(e, o, o->bm_out_tok, (size_t)outs * 4) || grow(e, o, o->bm_out_frame, (size_t)outs * 4) || grow(e, o, o->bm_out_lp, (size_t)outs * 4) ||
        (totals && grow(e, o, o->bm_out_lm, (size_t)n * nasr_beam::WMAX * 8 * 3)) ||
        (boost && (grow(e, o, o->bm_bstate, slots * 4) || grow(e, o, o->bm_raw, rows * nasr_boost::COLS * 4) ||
                   grow(e, o, o->bm_out_boost, (size_t)n * nasr_beam::WMAX * 8))))
        return -1;
    HIPCHK(hipMemcpyAsync(o->bm_utt.p, ud.data(), n * sizeof(BeamUtt), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(o->bm_rows.p, 0, rows * sizeof(RowDesc), st));
    HIPCHK(hipMemsetAsync(o->bm_key.p, 0, rows * 8, st));
    HIPCHK(hipMemsetAsync(o->bm_cnt.p, 0, 8 * 4, st));
    int *cnt = o->bm_cnt.as<int>();
    BeamParams bp;
    memset(&bp, 0, sizeof(bp));
    bp.utt = o->bm_utt.as<const BeamUtt>(); bp.n = n; bp.W = W; bp.N = N; bp.S = S; bp.prune = 1;
    bp.beam = o->bm_beam.as<nasr_beam::Beam>(); bp.nodes = o->bm_nodes.as<nasr_beam::Node>(); bp.encproj = o->encproj.as<float>(); bp.enc = o->bm_enc.as<float>();
    bp.rows = o->bm_rows.as<RowDesc>(); bp.ctrl = o->bm_ctrl.as<DecCtrl>(); bp.h = o->bm_h.as<float>(); bp.c = o->bm_c.as<float>();
    bp.lp_part = o->bm_part.as<const nasr_lp::Part>(); bp.alt_key = o->bm_alt.as<const unsigned long long>();
    bp.dlist = o->bm_dlist.as<int>(); bp.rowmap = o->bm_rowmap.as<unsigned>(); bp.err = cnt + 4;
    bp.out_n = o->bm_out_n.as<int32_t>(); bp.out_len = o->bm_out_len.as<int32_t>(); bp.out_score = o->bm_out_score.as<double>();
    bp.out_tok = o->bm_out_tok.as<int32_t>(); bp.out_frame = o->bm_out_frame.as<int32_t>(); bp.out_lp = o->bm_out_lp.as<float>();
    if (e->lm) {                                               // shallow fusion: the prune only where its proof holds (nasr_beam.h)
        bp.lm_on = 1; bp.lm = e->lm_view; bp.lm_weight = e->lm_weight; bp.lm_bonus = e->lm_bonus;
        bp.prune = nasr_beam::prune_allowed(e->lm_bonus, e->lm->all_nonpositive) ? 1 : 0;
    }
    if (totals) { bp.out_lm = o->bm_out_lm.as<double>(); bp.out_lm_final = bp.out_lm + (size_t)n * nasr_beam::WMAX; bp.out_total = bp.out_lm_final + (size_t)n * nasr_beam::WMAX; }
    if (boost) {                                               // a non-empty set pays positive bonuses: unpruned (nasr_beam.h)
        bp.boost_on = 1; bp.boost_bonus = e->boost_bonus; bp.boost_next = e->boost_next; bp.boost_state = o->bm_bstate.as<int>();
        bp.raw_logits = o->bm_raw.as<const float>(); bp.out_boost = o->bm_out_boost.as<double>();
        bp.prune = nasr_beam::prune_allowed(e->lm ? e->lm_bonus : 0.0f, e->lm ? e->lm->all_nonpositive != 0 : true, e->boost_states) ? 1 : 0;
    }
    DecParams dp;
    memset(&dp, 0, sizeof(dp));
    dp.rows = bp.rows; dp.B = (int)rows; dp.T = 1; dp.ctrl = bp.ctrl; dp.h = bp.h; dp.c = bp.c; dp.encproj = bp.enc;
    bind_dec_weights(e, dp);
    dp.predg = o->bm_predg.as<float>(); dp.key = o->bm_key.as<unsigned long long>(); dp.n_active = cnt + 5;
    dp.dlist = bp.dlist; dp.rowmap = bp.rowmap; dp.lp_part = o->bm_part.as<nasr_lp::Part>(); dp.alt_key = o->bm_alt.as<unsigned long long>(); dp.alt_k = nasr_beam::KTOP;
    if (boost) { dp.boost_bonus = bp.boost_bonus; dp.boost_next = bp.boost_next; dp.boost_state = bp.boost_state; dp.raw_logits = o->bm_raw.as<float>(); }
    bp.cnt_next = cnt; bp.cnt_zero = cnt + 2;
    ProfScope ps(e, "beam_search", 0, 0);                      // one scope for the whole search: thousands of rounds would each cost an event pair
    launch_beam_init(bp, st);
    const long long R = nasr_beam::rounds(maxT, S);
    for (long long r = 0; r < R; r++) {
        const int par = (int)(r & 1);
        dp.n_dirty = cnt + 2 * par; dp.n_rows = cnt + 2 * par + 1;
        if (boost) launch_decode_rows_boost(dp, st); else launch_decode_rows(dp, st);
        bp.cnt_zero = cnt + 2 * par; bp.cnt_next = cnt + 2 * (par ^ 1);
        launch_beam_select(bp, st);
    }
    launch_beam_final(bp, st);
    std::vector<int32_t> hn(n), hlen((size_t)n * nasr_beam::WMAX), htok((size_t)outs), hfr((size_t)outs);
    std::vector<double> hsc((size_t)n * nasr_beam::WMAX), hlm(totals ? (size_t)n * nasr_beam::WMAX * 3 : 0), hbo(boost ? (size_t)n * nasr_beam::WMAX : 0);
    std::vector<float> hlp((size_t)outs);
    int herr[1] = {0};
    HIPCHK(hipMemcpyAsync(hn.data(), bp.out_n, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hlen.data(), bp.out_len, hlen.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hsc.data(), bp.out_score, hsc.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(htok.data(), bp.out_tok, htok.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hfr.data(), bp.out_frame, hfr.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hlp.data(), bp.out_lp, hlp.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(herr, bp.err, 4, hipMemcpyDeviceToHost, st));
    if (e->lm) HIPCHK(hipMemcpyAsync(hlm.data(), bp.out_lm, hlm.size() * 8, hipMemcpyDeviceToHost, st));
    else if (boost) HIPCHK(hipMemcpyAsync(hlm.data() + (size_t)2 * n * nasr_beam::WMAX, bp.out_total, (size_t)n * nasr_beam::WMAX * 8, hipMemcpyDeviceToHost, st));
    if (boost) HIPCHK(hipMemcpyAsync(hbo.data(), bp.out_boost, hbo.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (herr[0]) return fail("beam search: the trie of an utterance outgrew its bound");
    for (int k = 0; k < n; k++) {
        const int b = ob.first + live[k];
        if (hn[k] < 1 || hn[k] > N) return fail("beam search left utterance %d unfinished", b);
        const long long cap = (long long)ud[k].T * S;
        for (int r = 0; r < hn[k]; r++) {
            const int len = hlen[(size_t)k * nasr_beam::WMAX + r];
            if (len < 0 || len > cap) return fail("beam search: hypothesis %d of utterance %d has %d tokens", r, b, len);
            const size_t at = (size_t)(ud[k].out0 + r * cap);
            OfflineState::BeamHyp h;
            h.score = hsc[(size_t)k * nasr_beam::WMAX + r];
            if (e->lm) h.lm_final = hlm[((size_t)n + k) * nasr_beam::WMAX + r];
            if (totals) h.total = hlm[((size_t)2 * n + k) * nasr_beam::WMAX + r];
            h.tokens.assign(htok.begin() + at, htok.begin() + at + len);
            if (boost) {                                       // the per-token bonuses are fixed now, from the set the search ran with
                h.boost = hbo[(size_t)k * nasr_beam::WMAX + r];
                int state = nasr_boost::STATE_ROOT;
                for (int32_t tk : h.tokens) {
                    h.bonuses.push_back(nasr_boost::bonus_of(e->boost_host.bonus.data(), state, tk));
                    state = nasr_boost::next_of(e->boost_host.next.data(), state, tk);
                }
            }
            h.frames.assign(hfr.begin() + at, hfr.begin() + at + len);
            h.lps.assign(hlp.begin() + at, hlp.begin() + at + len);
            o->beam_res[b].push_back(std::move(h));
        }
    }
    return 0;
}

// every beam call forgets the hypotheses of the call before, also one that fails on its parameters
static void beam_forget(nasr_engine *e) {
    if (e->off) { e->off->beam_valid = false; e->off->beam_res.clear(); }
}

static int beam_check_params(const nasr_beam_params *params, int *W, int *N, int *S) {
    if (!params) return fail("null beam parameters");
    *W = params->beam; *N = params->nbest == 0 ? params->beam : params->nbest; *S = params->max_symbols == 0 ? nasr_beam::S_DEFAULT : params->max_symbols;
    if (*W < 1 || *W > nasr_beam::WMAX) return fail("beam = %d outside 1 .. %d", params->beam, nasr_beam::WMAX);
    if (*N < 1 || *N > *W) return fail("nbest = %d outside 1 .. beam = %d", params->nbest, *W);
    if (*S < 1 || *S > nasr_beam::SMAX) return fail("max_symbols = %d outside 1 .. %d (0: the default, %d)", params->max_symbols, nasr_beam::SMAX, nasr_beam::S_DEFAULT);
    if (params->reserved != 0) return fail("the reserved field of nasr_beam_params must be 0");
    return 0;
}

// NASR_FLAG_BEAM_BOOST of a beam entry: it needs engine option "phrase_boost" and excludes NASR_FLAG_NO_BOOST
static int beam_check_flags(nasr_engine *e, uint32_t flags) {
    if (!(flags & NASR_FLAG_BEAM_BOOST)) return 0;
    if (!e->opt_phrase_boost) return fail("NASR_FLAG_BEAM_BOOST needs engine option \"phrase_boost\" (set it to the state capacity before the first step or offline call)");
    if (flags & NASR_FLAG_NO_BOOST) return fail("NASR_FLAG_BEAM_BOOST and NASR_FLAG_NO_BOOST exclude each other");
    return 0;
}

// the beam mode.  Its early checks run for every call: bad parameters fail with B == 0 too, and a refused call has forgotten the hypotheses before
static OffMode beam_mode(nasr_engine *e, const char *who, const nasr_beam_params *params, int32_t *n_hyps, uint32_t flags) {
    struct Run { int W = 0, N = 0, S = 0; };
    auto r = std::make_shared<Run>();
    OffMode m;
    m.who = who; m.counts = n_hyps;
    m.early = [=]() {
        beam_forget(e);
        return beam_check_params(params, &r->W, &r->N, &r->S) || beam_check_flags(e, flags) ? -1 : 0;
    };
    m.setup = [=](OfflineState *o, int B) {
        o->beam_res.assign(B, {});
        o->beam_lm = e->lm != nullptr; o->beam_lm_generation = e->lm_generation;
        o->beam_boost = (flags & NASR_FLAG_BEAM_BOOST) != 0;
        return 0;
    };
    m.batch = [=](OfflineState *o, const OffBatch &ob) { return beam_batch(e, o, ob, r->W, r->N, r->S); };
    m.failed = [](OfflineState *o) { o->beam_res.clear(); };
    m.finish = [=](OfflineState *o, int B) {
        o->beam_valid = true;
        for (int b = 0; b < B; b++) n_hyps[b] = (int32_t)o->beam_res[b].size();
        return 0;
    };
    return m;
}

// hypothesis `rank` of utterance u of the last beam call, or nullptr with the error set; ready (may be empty) is checked between the two
static const OfflineState::BeamHyp *beam_hyp(nasr_engine *e, int u, int rank, const std::function<int(OfflineState *)> &ready = nullptr) {
    if (!e) { fail("null engine"); return nullptr; }
    OfflineState *o = e->off;
    if (!o || !o->beam_valid || u < 0 || u >= (int)o->beam_res.size()) {
        fail("no beam hypotheses of utterance %d (they are those of the last offline call, which must be a beam call)", u);
        return nullptr;
    }
    if (ready && ready(o)) return nullptr;
    if (rank < 0 || rank >= (int)o->beam_res[u].size()) { fail("utterance %d has %d hypotheses, no rank %d", u, (int)o->beam_res[u].size(), rank); return nullptr; }
    return &o->beam_res[u][rank];
}
}  // namespace nasr_eng

extern "C" int nasr_engine_transcribe_beam_mel(nasr_engine *e, int B, const float *const *mel, const int32_t *n_frames, const int32_t *prompt_index,
                                               const nasr_beam_params *params, int32_t *n_hyps, uint32_t flags) {
    ApiGuard api_guard;
    return offline_call(e, B, mel_input(mel, n_frames), prompt_index, flags, beam_mode(e, "nasr_engine_transcribe_beam_mel", params, n_hyps, flags));
}

extern "C" int nasr_engine_transcribe_beam(nasr_engine *e, int B, const int16_t *const *pcm, const int32_t *n_samples, const int32_t *prompt_index,
                                           const nasr_beam_params *params, int32_t *n_hyps, uint32_t flags) {
    ApiGuard api_guard;
    return offline_call(e, B, pcm_input(pcm, n_samples), prompt_index, flags, beam_mode(e, "nasr_engine_transcribe_beam", params, n_hyps, flags));
}

extern "C" int nasr_engine_history_beam(nasr_engine *e, nasr_stream *const *streams, int B, const int64_t *first, const int32_t *count,
                                        const nasr_beam_params *params, int32_t *n_hyps, uint32_t flags) {
    ApiGuard api_guard;
    return offline_call(e, B, history_input(streams, first, count), nullptr, flags, beam_mode(e, "nasr_engine_history_beam", params, n_hyps, flags));
}

extern "C" int nasr_engine_beam_hypothesis(nasr_engine *e, int u, int rank, int32_t *tokens_out, int32_t *frames_out, float *token_logprobs_out,
                                           int32_t cap, double *score_out) {
    ApiGuard api_guard;
    const OfflineState::BeamHyp *h = beam_hyp(e, u, rank);
    if (!h) return -1;
    if (tokens_out) read_out(h->tokens, tokens_out, cap);
    if (frames_out) read_out(h->frames, frames_out, cap);
    if (token_logprobs_out) read_out(h->lps, token_logprobs_out, cap);
    if (score_out) *score_out = h->score;
    return (int)h->tokens.size();
}

// the language-model side of a hypothesis of the last beam call, which must have run with an LM attached: lm_final (the EOS term included
// when the model has one) and the final key, both as the device computed them; the per-token values are recomputed here by the same
// nasr_lm::lookup over the returned tokens (the trie node does not carry them)
extern "C" int nasr_engine_beam_hypothesis_lm(nasr_engine *e, int u, int rank, double *lm_logprob_out, double *total_out, float *token_lm_logprobs_out,
                                              int32_t cap) {
    ApiGuard api_guard;
    const OfflineState::BeamHyp *h = beam_hyp(e, u, rank, [&](OfflineState *o) {
        if (!o->beam_lm || !e->lm) return fail("the last beam call ran without a language model (nasr_engine_set_lm)");
        if (o->beam_lm_generation != e->lm_generation)
            return fail("the language model was replaced after the last beam call (nasr_engine_set_lm): its hypotheses have no LM read-out any more");
        return 0;
    });
    if (!h) return -1;
    if (lm_logprob_out) *lm_logprob_out = h->lm_final;
    if (total_out) *total_out = h->total;
    const int n = std::min<int>((int)h->tokens.size(), std::max(cap, 0));
    if (token_lm_logprobs_out) {
        const nasr_lm::View v = e->lm->view();
        int32_t state = v.start;
        for (int i = 0; i < n; i++) token_lm_logprobs_out[i] = (float)nasr_lm::lookup(v, state, h->tokens[(size_t)i], &state);
    }
    return (int)h->tokens.size();
}

// the boost side of a hypothesis of the last beam call, which must have been boosted (NASR_FLAG_BEAM_BOOST): the sum of its tokens' bonuses and the
// ranking key, both as the device computed them; the per-token bonuses were fixed when the call fetched its results, from the set it ran with
extern "C" int nasr_engine_beam_hypothesis_boost(nasr_engine *e, int u, int rank, double *boost_out, double *total_out, float *token_bonus_out, int32_t cap) {
    ApiGuard api_guard;
    const OfflineState::BeamHyp *h = beam_hyp(e, u, rank, [](OfflineState *o) {
        return o->beam_boost ? 0 : fail("the last beam call ran without phrase boosting (NASR_FLAG_BEAM_BOOST)");
    });
    if (!h) return -1;
    if (boost_out) *boost_out = h->boost;
    if (total_out) *total_out = h->total;
    if (token_bonus_out) read_out(h->bonuses, token_bonus_out, cap);
    return (int)h->tokens.size();
}
