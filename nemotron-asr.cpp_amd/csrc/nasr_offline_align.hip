// nasr_offline_align.hip -- forced alignment and transcript scoring on the RNN-T lattice (nasr_engine_align*): the align mode of an offline
// call (nasr_offline_state.h: offline_call) and the lattice read-out.  Rules: nasr_align.h; kernels: kernels_align.hip.
#include "nasr_offline_state.h"

namespace nasr_eng {
struct AlignOut { std::vector<double> loglik, best; std::vector<std::vector<int32_t>> frames; std::vector<std::vector<float>> lps; };

// the lattices of one sub-batch whose encoder projection is in o->encproj: teacher-forced prediction network, joint over every cell,
// both recursions and the backtrace, all on the device
static int align_batch(nasr_engine *e, OfflineState *o, const OffBatch &ob, const int32_t *const *tokens, const int32_t *n_tokens, AlignOut &out) {
    hipStream_t st = e->st;
    const double ninf = nasr_align::neg_inf_d();
    std::vector<int> live;                                   // utterances with at least one encoder frame: decoder slot k = live[k]
    std::vector<nasr_align::Utt> ud;
    std::vector<int32_t> tok;
    long long cells = 0;
    int g_rows = 0, max_u = 0;
    for (int k = 0; k < ob.n; k++) {
        const int b = ob.first + k, U = n_tokens[b];
        if (ob.T[k] == 0) {                                  // no frame: only the empty transcript has a path
            out.loglik[b] = out.best[b] = U == 0 ? 0.0 : ninf;
            out.frames[b].assign(U, -1);
            out.lps[b].assign(U, nasr_lp::neg_inf());
            continue;
        }
        nasr_align::Utt u;
        u.enc_row = ob.off[k]; u.g_row = g_rows; u.T = ob.T[k]; u.U = U; u.cell0 = cells; u.tok0 = (int)tok.size(); u.pad = 0;
        ud.push_back(u); live.push_back(k);
        tok.insert(tok.end(), tokens[b], tokens[b] + U);
        cells += nasr_align::n_cells(u.T, U);
        g_rows += U + 1;
        max_u = std::max(max_u, U);
    }
    const int n = (int)live.size();
    if (n == 0) return 0;
    if (!o->al_utt) {
        if (off_alloc(o, (void **)&o->al_utt, nasr_plan::OFFLINE_MAX_UTTS * sizeof(nasr_align::Utt)) ||
            off_alloc(o, (void **)&o->al_scores, nasr_plan::OFFLINE_MAX_UTTS * 2 * sizeof(double))) return -1;
    }
    std::vector<nasr_align::Tile> tiles;
    std::vector<int> lfirst;
    nasr_align::plan_launches(ud.data(), n, e->opt_align_cells, tiles, lfirst);
    const size_t ntok = std::max<size_t>(tok.size(), 1);
    if (grow(e, o, o->al_g, (size_t)g_rows * JNT * 4) || grow(e, o, o->al_lpb, (size_t)cells * 4) || grow(e, o, o->al_lpt, (size_t)cells * 4) ||
        grow(e, o, o->al_bp, (size_t)cells) || grow(e, o, o->al_tiles, tiles.size() * sizeof(nasr_align::Tile)) || grow(e, o, o->al_tok, ntok * 4) ||
        grow(e, o, o->al_frames, ntok * 4) || grow(e, o, o->al_tlp, ntok * 4)) return -1;
    float *al_g = o->al_g.as<float>(), *al_lpb = o->al_lpb.as<float>(), *al_lpt = o->al_lpt.as<float>(), *al_tlp = o->al_tlp.as<float>();
    int32_t *al_tok = o->al_tok.as<int32_t>(), *al_frames = o->al_frames.as<int32_t>();
    nasr_align::Tile *al_tiles = o->al_tiles.as<nasr_align::Tile>();
    std::vector<RowDesc> rd(n);
    for (int k = 0; k < n; k++) { memset(&rd[k], 0, sizeof(RowDesc)); rd[k].slot = k; rd[k].prompt = -1; }
    // (the host vectors live until the stream is synchronised below)
    HIPCHK(hipMemcpyAsync(o->al_utt, ud.data(), (size_t)n * sizeof(nasr_align::Utt), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(al_tiles, tiles.data(), tiles.size() * sizeof(nasr_align::Tile), hipMemcpyHostToDevice, st));
    if (!tok.empty()) HIPCHK(hipMemcpyAsync(al_tok, tok.data(), tok.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(o->drows, rd.data(), (size_t)n * sizeof(RowDesc), hipMemcpyHostToDevice, st));
    // ---- g[u] of every utterance: the decode's own LSTM / joint.pred launches over the utterances that still have a position u --------
    launch_off_dec_reset(n, o->dec.h, o->dec.c, o->dec.ctrl, st);
    DecParams dp;
    bind_decode(e, o->dec, DecFeatures(), dp);              // the base part only: teacher forcing runs none of the options' launches
    dp.rows = o->drows; dp.B = n; dp.T = 1;
    AlignPredParams pp;
    memset(&pp, 0, sizeof(pp));
    pp.utt = o->al_utt; pp.n = n; pp.tok = al_tok; pp.ctrl = o->dec.ctrl; pp.dlist = o->dec.dlist; pp.n_dirty = dp.n_dirty; pp.predg = o->dec.predg; pp.g = al_g;
    {
        ProfScope ps(e, "k_align_pred", 0, 0);
        for (int u = 0; u <= max_u + 1; u++) {
            pp.u = u;
            launch_align_pred_step(pp, st);
            if (u <= max_u) launch_decode_candidates(dp, st);
        }
    }
    // ---- the joint over every cell, "align_cells" cells per launch ---------------------------------------------------------------------
    AlignParams ap;
    memset(&ap, 0, sizeof(ap));
    ap.utt = o->al_utt; ap.encproj = o->encproj.as<float>(); ap.g = al_g; ap.tok = al_tok; ap.out_w = dp.out_w; ap.out_b = dp.out_b;
    ap.lp_blank = al_lpb; ap.lp_token = al_lpt;
    for (size_t i = 0; i + 1 < lfirst.size(); i++) {
        const int cnt = lfirst[i + 1] - lfirst[i];
        double c = 0;
        for (int j = lfirst[i]; j < lfirst[i + 1]; j++) c += nasr_align::tile_cells(ud[tiles[j].utt].T, ud[tiles[j].utt].U, tiles[j].t0, tiles[j].u0);
        ProfScope ps(e, "k_align_lattice", (double)cnt * 1040 * JNT * 4, c * 2.0 * JNT * VOCAB);
        ap.tiles = al_tiles + lfirst[i];
        launch_align_lattice(ap, cnt, st);
    }
    // ---- forward and Viterbi recursions, backtrace ------------------------------------------------------------------------------------
    AlignRecParams rp;
    memset(&rp, 0, sizeof(rp));
    rp.utt = o->al_utt; rp.lp_blank = al_lpb; rp.lp_token = al_lpt; rp.bp = o->al_bp.as<unsigned char>(); rp.scores = o->al_scores; rp.frames = al_frames; rp.tok_lp = al_tlp;
    {
        ProfScope ps(e, "k_align_recursion", (double)cells * 9, 0);
        launch_align_recursion(rp, n, st);
    }
    std::vector<double> sc((size_t)n * 2);
    std::vector<int32_t> fr(tok.size());
    std::vector<float> lp(tok.size());
    HIPCHK(hipMemcpyAsync(sc.data(), o->al_scores, sc.size() * 8, hipMemcpyDeviceToHost, st));
    if (!tok.empty()) {
        HIPCHK(hipMemcpyAsync(fr.data(), al_frames, fr.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(lp.data(), al_tlp, lp.size() * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (int k = 0; k < n; k++) {
        const int b = ob.first + live[k];
        out.loglik[b] = sc[(size_t)2 * k]; out.best[b] = sc[(size_t)2 * k + 1];
        out.frames[b].assign(fr.begin() + ud[k].tok0, fr.begin() + ud[k].tok0 + ud[k].U);
        out.lps[b].assign(lp.begin() + ud[k].tok0, lp.begin() + ud[k].tok0 + ud[k].U);
        if (e->debug) {
            const size_t nc = (size_t)nasr_align::n_cells(ud[k].T, ud[k].U);
            o->lat_b[b].resize(nc); o->lat_t[b].resize(nc);
            HIPCHK(hipMemcpy(o->lat_b[b].data(), al_lpb + ud[k].cell0, nc * 4, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(o->lat_t[b].data(), al_lpt + ud[k].cell0, nc * 4, hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

// the align mode: a transcript per utterance in; the two scores, the best path's frames and its tokens' ln P out (the lattices too with debug on)
static OffMode align_mode(nasr_engine *e, const char *who, const int32_t *const *tokens, const int32_t *n_tokens, double *loglik_out, double *best_out,
                          int32_t *const *frames_out, float *const *token_logprobs_out) {
    auto out = std::make_shared<AlignOut>();
    OffMode m;
    m.who = who; m.counts = n_tokens;
    m.check = [=](int B) {
        for (int b = 0; b < B; b++) {
            const int U = n_tokens[b];
            if (U < 0 || U > NASR_ALIGN_MAX_TOKENS)
                return fail("utterance %d: a transcript of %d tokens, outside 0 .. NASR_ALIGN_MAX_TOKENS = %d", b, U, NASR_ALIGN_MAX_TOKENS);
            if (U > 0 && (!tokens || !tokens[b])) return fail("utterance %d: null transcript", b);
            for (int i = 0; i < U; i++)
                if (tokens[b][i] < 0 || tokens[b][i] >= BLANK)
                    return fail("utterance %d: token %d of its transcript is %d; only ids 0 .. %d can be aligned (%d is blank)", b, i, tokens[b][i], BLANK - 1, BLANK);
        }
        return 0;
    };
    m.setup = [=](OfflineState *o, int B) {
        if (e->debug) { o->lat_b.assign(B, {}); o->lat_t.assign(B, {}); }
        out->loglik.assign(B, 0.0); out->best.assign(B, 0.0); out->frames.assign(B, {}); out->lps.assign(B, {});
        return 0;
    };
    m.batch = [=](OfflineState *o, const OffBatch &ob) { return align_batch(e, o, ob, tokens, n_tokens, *out); };
    m.finish = [=](OfflineState *o, int B) {
        o->lat_valid = e->debug;
        for (int b = 0; b < B; b++) {
            if (loglik_out) loglik_out[b] = out->loglik[b];
            if (best_out) best_out[b] = out->best[b];
            if (frames_out && frames_out[b]) memcpy(frames_out[b], out->frames[b].data(), out->frames[b].size() * 4);
            if (token_logprobs_out && token_logprobs_out[b]) memcpy(token_logprobs_out[b], out->lps[b].data(), out->lps[b].size() * 4);
        }
        return 0;
    };
    return m;
}
}  // namespace nasr_eng

extern "C" int nasr_engine_align_mel(nasr_engine *e, int B, const float *const *mel, const int32_t *n_frames, const int32_t *prompt_index,
                                     const int32_t *const *tokens, const int32_t *n_tokens, double *loglik_out, double *best_out,
                                     int32_t *const *frames_out, float *const *token_logprobs_out, uint32_t flags) {
    ApiGuard api_guard;
    return offline_call(e, B, mel_input(mel, n_frames), prompt_index, flags,
                        align_mode(e, "nasr_engine_align_mel", tokens, n_tokens, loglik_out, best_out, frames_out, token_logprobs_out));
}

extern "C" int nasr_engine_align(nasr_engine *e, int B, const int16_t *const *pcm, const int32_t *n_samples, const int32_t *prompt_index,
                                 const int32_t *const *tokens, const int32_t *n_tokens, double *loglik_out, double *best_out,
                                 int32_t *const *frames_out, float *const *token_logprobs_out, uint32_t flags) {
    ApiGuard api_guard;
    return offline_call(e, B, pcm_input(pcm, n_samples), prompt_index, flags,
                        align_mode(e, "nasr_engine_align", tokens, n_tokens, loglik_out, best_out, frames_out, token_logprobs_out));
}

extern "C" int nasr_engine_history_align(nasr_engine *e, nasr_stream *const *streams, int B, const int64_t *first, const int32_t *count,
                                         const int32_t *const *tokens, const int32_t *n_tokens, double *loglik_out, double *best_out,
                                         int32_t *const *frames_out, float *const *token_logprobs_out, uint32_t flags) {
    ApiGuard api_guard;
    return offline_call(e, B, history_input(streams, first, count), nullptr, flags,
                        align_mode(e, "nasr_engine_history_align", tokens, n_tokens, loglik_out, best_out, frames_out, token_logprobs_out));
}

extern "C" int64_t nasr_engine_align_lattice(nasr_engine *e, int u, float *lp_blank_out, float *lp_token_out, int64_t cap) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    OfflineState *o = e->off;
    if (!o || !o->lat_valid || u < 0 || u >= (int)o->lat_b.size())
        return fail("no lattice of utterance %d (the last offline call must be an align call made with nasr_engine_set_debug(e, 1))", u);
    const int64_t have = (int64_t)o->lat_b[u].size();
    if (!lp_blank_out && !lp_token_out) return have;         // size query
    const int64_t n = std::min<int64_t>(have, std::max<int64_t>(cap, 0));
    if (lp_blank_out) memcpy(lp_blank_out, o->lat_b[u].data(), (size_t)n * 4);
    if (lp_token_out) memcpy(lp_token_out, o->lat_t[u].data(), (size_t)n * 4);
    return n;
}
