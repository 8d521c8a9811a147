// nasr_offline.hip -- offline full-context transcription of whole utterances, batched (nasr_engine_transcribe_mel).
// Replaces nemo_transcribe_audio / nemo_encode (reference src/nemo-ggml.cpp:1600-1737): the preprocessor output of a whole
// utterance -> ConvSubsampling without drop-2 -> 24 conformer layers whose attention sees every frame of the utterance
// (build_rel_pos_mha :668-755, no mask, no cache; the depthwise conv starts from a zero history) -> prompt fusion -> greedy
// RNN-T decode (:1231-).  The utterances of a call are packed densely (M = sum T_b rows, no padding) and cut into sub-batches
// of at most "offline_rows" rows (nasr_offline_plan.h); every kernel's result for a row depends on its own utterance only, so
// a sub-batch gives the bits the utterance gives alone.  Nothing of the streaming state is touched: the path has its own
// buffers (allocated on the first call), its own decoder slots and token rings, and never captures a graph.
// This file: the encoder of a sub-batch, the PCM-to-mel stage, the driver of an offline call (offline_call), the greedy mode and the taps.
#include "nasr_offline_state.h"

namespace nasr_eng {

int off_alloc(OfflineState *o, void **p, size_t bytes) {
    HIPCHK(hipMalloc(p, std::max<size_t>(bytes, 16)));
    o->bufs.push_back(*p);
    return 0;
}
static void off_free(OfflineState *o, void *p) {
    if (!p) return;
    for (auto &b : o->bufs) if (b == p) { hipFree(p); b = nullptr; }
}

void offline_destroy(nasr_engine *e) {
    if (!e->off) return;
    for (void *p : e->off->bufs) if (p) hipFree(p);
    delete e->off;
    e->off = nullptr;
}

// linear_pos of the sinusoid rows of relative positions 2047 .. -2047, once per engine (the reference slices the T-centred
// 2T - 1 rows of the same table, src/nemo-ggml.cpp:17-32, :229-233, :700-705)
static int ensure_offline_pos(nasr_engine *e, OfflineState *o) {
    if (!o->pos.empty()) return 0;
    const size_t n = (size_t)OFFLINE_NREL * D;
    std::vector<float> emb(n);
    for (int r = 0; r < OFFLINE_NREL; r++) host_pos_emb((OFFLINE_MAX_T - 1) - r, &emb[(size_t)r * D]);
    float *demb = nullptr, *dout = nullptr;
    HIPCHK(hipMalloc((void **)&demb, n * 4));
    HIPCHK(hipMalloc((void **)&dout, n * 4));
    HIPCHK(hipMemcpy(demb, emb.data(), n * 4, hipMemcpyHostToDevice));
    for (auto &L : e->L) {
        GemmParams g;
        memset(&g, 0, sizeof(g));
        g.A = demb; g.W = L.wpos_f32; g.M = OFFLINE_NREL; g.N = D; g.K = D; g.lda = D;
        g.epi = EPI_PART_F32; g.out_f32 = dout; g.ldo = D; g.splits = 1;
        g.f32_fma_tile = e->opt_f32_mfma ? 0 : 1;
        launch_gemm_f32(g, e->st);
        void *pp;
        if (off_alloc(o, &pp, n * e->esz)) return -1;
        if (e->bf16) launch_f32_to_bf16(dout, (bf16_t *)pp, (int64_t)n, e->st);
        else HIPCHK(hipMemcpyAsync(pp, dout, n * 4, hipMemcpyDeviceToDevice, e->st));
        o->pos.push_back(pp);
    }
    HIPCHK(hipStreamSynchronize(e->st));
    hipFree(demb);
    hipFree(dout);
    return 0;
}

// the decode slots of a sub-batch and what the greedy decode's windows need, once per engine
static int ensure_dec_slots(nasr_engine *e, OfflineState *o) {
    if (o->dec.ctrl) return 0;
    const size_t U = nasr_plan::OFFLINE_MAX_UTTS, W = OFF_DEC_WIN;
    int rc = dec_set_ensure(o->dec, dec_features(e), (int)U, (int)(U * W), [o](const char *, void **p, size_t bytes) { return off_alloc(o, p, bytes); }, fail);
    rc |= off_alloc(o, (void **)&o->win, U * W * JNT * 4);
    rc |= off_alloc(o, (void **)&o->drows, U * sizeof(RowDesc));
    rc |= off_alloc(o, (void **)&o->dwin, U * sizeof(int4));
    rc |= off_alloc(o, (void **)&o->sdesc, U * sizeof(OffSubDesc));
    if (rc) return -1;
    HIPCHK(hipMemset(o->dec.n_active, 0, 16));
    return 0;
}

// row buffers for `rows` packed rows (grown, never shrunk) and the decode slots
static int ensure_rows(nasr_engine *e, OfflineState *o, int rows) {
    if (rows <= o->rows_cap) return 0;
    HIPCHK(hipStreamSynchronize(e->st));
    const size_t M = (size_t)std::max(rows, 64), es = e->esz;
    const struct { OffBuf *b; size_t bytes; } row_bufs[] = {
        {&o->x, M * D * 4}, {&o->glu, M * D * 4}, {&o->hfuse, e->hp.num_prompts > 0 ? M * 2048 * 4 : 16}, {&o->encproj, M * JNT * 4},
        {&o->a, M * D * es}, {&o->hbuf, M * FF * es}, {&o->qkv, M * 3 * D * es}, {&o->ctx, M * D * es}, {&o->cbuf, M * D * es},
        {&o->tpos, M * 4}, {&o->items, M * sizeof(int4)} /* at most one attention work item per row */, {&o->prow, M * sizeof(RowDesc)}};
    for (auto &r : row_bufs) { off_free(o, r.b->p); *r.b = OffBuf(); }
    int rc = 0;
    for (auto &r : row_bufs) { rc |= off_alloc(o, &r.b->p, r.bytes); r.b->cap = r.bytes; }
    if (rc) return -1;
    o->rows_cap = (int)M;
    if (!o->zero_bias) {
        if (off_alloc(o, (void **)&o->zero_bias, 3 * D * 4)) return -1;
        HIPCHK(hipMemset(o->zero_bias, 0, 3 * D * 4));
    }
    return ensure_dec_slots(e, o);
}

int grow(nasr_engine *e, OfflineState *o, OffBuf &b, size_t bytes) {
    if (bytes <= b.cap) return 0;
    HIPCHK(hipStreamSynchronize(e->st));
    off_free(o, b.p);
    b = OffBuf();
    if (off_alloc(o, &b.p, bytes)) return -1;
    b.cap = bytes;
    return 0;
}

// the encoder of one sub-batch up to the joint's encoder projection: what transcription and alignment share
static int run_offline_encoder(nasr_engine *e, OfflineState *o, const float *const *mel, const int32_t *n_mel, const int32_t *prompt_index,
                               const std::vector<int> &Tall, int first, int n, OffBatch &ob) {
    hipStream_t st = e->st;
    const int act = e->bf16 ? 1 : 0, nL = e->hp.n_layers, ks = e->hp.kernel_size;
    // ---- plan of the sub-batch: packed rows, front-end images, attention work items -----------------------------
    std::vector<int> &off = ob.off, &T = ob.T;
    off.assign(n, 0); T.assign(n, 0);
    ob.first = first; ob.n = n; ob.M = 0; ob.maxT = 0;
    std::vector<OffSubDesc> sd(n);
    int M = 0, mel_rows = 0, h2_rows = 0, h3_rows = 0, max_h2 = 0, maxT = 0;
    for (int k = 0; k < n; k++) {
        const int b = first + k;
        T[k] = Tall[b]; off[k] = M; M += T[k]; maxT = std::max(maxT, T[k]);
        sd[k].mel_off = mel_rows; sd[k].n_mel = n_mel[b]; sd[k].out_row = h2_rows; sd[k].pad = 0;
        mel_rows += n_mel[b];
        h2_rows += nasr_plan::sub_h2(n_mel[b]);
        h3_rows += T[k];
        max_h2 = std::max(max_h2, nasr_plan::sub_h2(n_mel[b]));
    }
    ob.M = M; ob.maxT = maxT;
    if (M == 0) return 0;                                    // every utterance too short for one mel frame: nothing runs
    if (ensure_rows(e, o, M)) return -1;
    const int qb = off_attn_qb(act);
    std::vector<int4> items;
    std::vector<int> tpos(M);
    std::vector<RowDesc> prow(M);
    for (int k = 0; k < n; k++) {
        for (int q0 = 0; q0 < T[k]; q0 += qb) items.push_back(make_int4(off[k], T[k], q0, 0));
        for (int t = 0; t < T[k]; t++) {
            tpos[off[k] + t] = t;
            RowDesc &rd = prow[off[k] + t];
            memset(&rd, 0, sizeof(rd));
            rd.prompt = prompt_index ? prompt_index[first + k] : -1;
        }
    }
    HIPCHK(hipMemcpy(o->items.as<int4>(), items.data(), items.size() * sizeof(int4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o->tpos.as<int>(), tpos.data(), (size_t)M * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o->prow.as<RowDesc>(), prow.data(), (size_t)M * sizeof(RowDesc), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o->sdesc, sd.data(), (size_t)n * sizeof(OffSubDesc), hipMemcpyHostToDevice));
    // Every GEMM of the path runs on at least OFF_MIN_ROWS rows (the rows past M are scratch whose results nobody reads) and without
    // split-K: the GEMM form -- and with it the summation order of every output row -- is then the same whatever the rows of the other
    // utterances, which is what makes a batch bit-identical to its utterances alone (the skinny kernel below 33 rows and split-K sum
    // differently; the large-M variants give the same bits, tests/micro/gemm_variant_identity.py).
    auto gm = [](int rows) { return std::max(rows, OFF_MIN_ROWS); };
    const int Mg = gm(M);
    if (grow(e, o, o->part, (size_t)Mg * D * 4)) return -1;
    // front-end images: conv0+dw output [H2][33][256] act, pw3 output f32, dw output [H3][17][256] act, pw6 output act
    const size_t img = std::max({(size_t)gm(h2_rows * 33), (size_t)gm(h3_rows * 17), (size_t)Mg * 17}) * SUBC * 4;
    if (grow(e, o, o->sub_a, img) || grow(e, o, o->sub_b, img)) return -1;
    if (grow(e, o, o->mel, (size_t)std::max(mel_rows, 1) * NMEL * 4)) return -1;
    for (int k = 0; k < n; k++)
        if (n_mel[first + k] > 0)
            HIPCHK(hipMemcpyAsync(o->mel.as<float>() + (size_t)sd[k].mel_off * NMEL, mel[first + k], (size_t)n_mel[first + k] * NMEL * 4, hipMemcpyDefault, st));   // host (mel entry) or device (PCM entry)
    // debug taps of this sub-batch
    if (e->debug) {
        off_free(o, o->t_sub); off_free(o, o->t_lay); off_free(o, o->t_enc);
        if (off_alloc(o, (void **)&o->t_sub, (size_t)M * D * 4) || off_alloc(o, (void **)&o->t_lay, (size_t)nL * M * D * 4) ||
            off_alloc(o, (void **)&o->t_enc, (size_t)M * D * 4)) return -1;
    }
    // ---- subsampling over every whole utterance (no drop-2) ------------------------------------------------------
    {
        ProfScope ps(e, "k_off_conv0_dw", (double)mel_rows * NMEL * 4 + (double)h2_rows * 33 * SUBC * e->esz, 2.0 * h2_rows * 33 * SUBC * 90);
        launch_off_conv0_dw(o->sdesc, n, max_h2, o->mel.as<float>(), e->w0t, e->b0, e->w2t, e->b2, o->sub_b.p, act, st);
    }
    run_sub_pw3(e, o->sub_b.p, o->sub_a.as<float>(), gm(h2_rows * 33));
    {
        ProfScope ps(e, "k_sub_dw", (double)h2_rows * 33 * SUBC * 4, 2.0 * h3_rows * 17 * SUBC * 9);
        int r3 = 0;
        for (int k = 0; k < n; k++) {
            const int h2 = nasr_plan::sub_h2(n_mel[first + k]);
            if (h2 == 0) continue;
            launch_sub_dw(o->sub_a.as<float>() + (size_t)sd[k].out_row * 33 * SUBC, 1, h2, 33, e->w5t, e->b5,
                          o->sub_b.as<char>() + (size_t)r3 * 17 * SUBC * e->esz, act, st);
            r3 += T[k];
        }
    }
    run_sub_pw6(e, o->sub_b.p, o->sub_a.p, gm(h3_rows * 17));
    run_sub_out(e, o->sub_a.p, o->x.as<float>(), Mg);
    if (e->debug) HIPCHK(hipMemcpyAsync(o->t_sub, o->x.as<float>(), (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));

    // ---- conformer layers over all M rows ------------------------------------------------------------------------
    LayerRun r;
    r.x = o->x.as<float>(); r.part = o->part.as<float>(); r.glu = o->glu.as<float>(); r.a = o->a.p; r.hbuf = o->hbuf.p; r.ctx = o->ctx.p; r.cbuf = o->cbuf.p;
    r.M = M; r.Mg = Mg;
    r.split_k = false;
    r.chain = false;
    // q | k | v of every row (no ring: the offline layer has no cache)
    r.qkv_out = [&](int, GemmParams &g) { g.epi = EPI_BIAS_ACT; g.out_act = o->qkv.p; g.ldo_act = 3 * D; g.bias = o->zero_bias; };
    r.attention = [&](int l) {
        const LayerW &L = e->L[l];
        OffAttnParams ap;
        ap.qkv = o->qkv.p; ap.pos = o->pos[l]; ap.bias_u = L.bias_u; ap.bias_v = L.bias_v; ap.items = o->items.as<int4>(); ap.ctx = o->ctx.p;
        double sq = 0;
        for (int k = 0; k < n; k++) sq += (double)T[k] * T[k];
        ProfScope ps(e, "k_off_attention", (double)M * 4 * D * e->esz, sq * NH * DH * 6.0);
        launch_off_attention(ap, (int)items.size(), act, st);
    };
    r.dwconv = [&](int l) {
        const LayerW &L = e->L[l];
        ProfScope ps(e, "k_off_dwconv", (double)M * D * (4 + e->esz), 2.0 * M * D * ks);
        launch_off_dwconv(o->glu.as<float>(), o->tpos.as<int>(), M, L.dw, ks, L.cln_w, L.cln_b, o->cbuf.p, act, st);
    };
    if (e->debug) r.tap = [&](int l) -> int {
        HIPCHK(hipMemcpyAsync(o->t_lay + (size_t)l * M * D, o->x.as<float>(), (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
        return 0;
    };
    if (enqueue_layers(e, r, 0, nL)) return -1;
    // ---- prompt fusion (one prompt per row), the joint's encoder projection ------------------------------------------
    if (enqueue_encoder_tail(e, o->x.as<float>(), o->hfuse.as<float>(), o->encproj.as<float>(), o->prow.as<RowDesc>(), M, Mg, 1, [&]() -> int {
            if (e->debug) HIPCHK(hipMemcpyAsync(o->t_enc, o->x.as<float>(), (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
            return 0;
        }))
        return -1;
    return 0;
}

// debug taps of a sub-batch, by utterance
static int fetch_offline_taps(nasr_engine *e, OfflineState *o, const OffBatch &ob) {
    const int nL = e->hp.n_layers, M = ob.M;
    HIPCHK(hipStreamSynchronize(e->st));
    for (int k = 0; k < ob.n; k++) {
        const int b = ob.first + k;
        const size_t rows = (size_t)ob.T[k] * D, o0 = (size_t)ob.off[k] * D;
        o->tap_sub[b].resize(rows); o->tap_enc[b].resize(rows);
        HIPCHK(hipMemcpy(o->tap_sub[b].data(), o->t_sub + o0, rows * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(o->tap_enc[b].data(), o->t_enc + o0, rows * 4, hipMemcpyDeviceToHost));
        o->tap_lay[b].assign(nL, std::vector<float>(rows));
        for (int l = 0; l < nL; l++)
            HIPCHK(hipMemcpy(o->tap_lay[b][l].data(), o->t_lay + (size_t)l * M * D + o0, rows * 4, hipMemcpyDeviceToHost));
    }
    return 0;
}

// the greedy mode's batch step: the decode of the sub-batch whose encoder projection is in o->encproj; tokens / frames appended to toks[b] / frs[b]
static int run_offline_batch(nasr_engine *e, OfflineState *o, const OffBatch &ob, std::vector<std::vector<int32_t>> &toks,
                             std::vector<std::vector<int32_t>> &frs) {
    hipStream_t st = e->st;
    if (ob.M == 0) return 0;
    const std::vector<int> &off = ob.off, &T = ob.T;
    const int first = ob.first, n = ob.n, maxT = ob.maxT;
    // ---- greedy decode in windows of 256 frames per utterance (token ring: 4096 > 256 x 10 symbols) -----------------
    launch_off_dec_reset(n, o->dec.h, o->dec.c, o->dec.ctrl, st);
    if (o->dec.boost_state)                                          // every utterance starts with an empty history (NASR_FLAG_NO_BOOST: in the disabled state)
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)o->dec.boost_state, o->no_boost ? nasr_boost::STATE_OFF : nasr_boost::STATE_ROOT, (size_t)n, st));
    if (o->dec.lm_state) {                                           // ... and at the model's start (NASR_FLAG_NO_LM: switched off); the reset left every slot dirty, so the
        nasr_lm::Greedy g = {};                                  // first iteration refreshes its bias row
        g.lm = e->lm_view; g.attached = e->lm ? 1 : 0;
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)o->dec.lm_state, nasr_lm::greedy_start(g, !o->no_lm), (size_t)n, st));
    }
    std::vector<int> tok_read(n, 0);
    std::vector<DecCtrl> hctrl(n);
    std::vector<int> ring((size_t)n * TOK_CAP), ringf((size_t)n * TOK_CAP);
    std::vector<float> ringl(e->opt_token_logprobs ? (size_t)n * TOK_CAP : 0);
    std::vector<float> ringb(e->opt_frame_blank ? (size_t)n * FRAME_CAP : 0);
    std::vector<float> ringe(e->opt_token_entropy ? (size_t)n * TOK_CAP : 0);
    const int K = e->opt_token_alt;
    std::vector<int32_t> ringai((size_t)n * TOK_CAP * K);
    std::vector<float> ringal((size_t)n * TOK_CAP * K);
    for (int w0 = 0; w0 < maxT; w0 += OFF_DEC_WIN) {
        std::vector<RowDesc> rd(n);
        std::vector<int4> wd(n);
        int max_dec = 0;
        for (int k = 0; k < n; k++) {
            const int nd = std::min(std::max(T[k] - w0, 0), OFF_DEC_WIN);
            memset(&rd[k], 0, sizeof(RowDesc));
            rd[k].slot = k; rd[k].n_dec = nd; rd[k].prompt = -1;
            wd[k] = make_int4(off[k] + w0, nd, 0, 0);
            max_dec = std::max(max_dec, nd);
        }
        HIPCHK(hipMemcpyAsync(o->drows, rd.data(), (size_t)n * sizeof(RowDesc), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(o->dwin, wd.data(), (size_t)n * sizeof(int4), hipMemcpyHostToDevice, st));
        launch_off_window(o->encproj.as<float>(), o->dwin, n, OFF_DEC_WIN, o->win, st);
        DecParams dp;
        bind_decode(e, o->dec, dec_features(e), dp);
        dp.rows = o->drows; dp.B = n; dp.T = OFF_DEC_WIN; dp.encproj = o->win;
        launch_decode_begin(dp, st);
        int h_active = 0;
        if (decode_until_idle(e, dp, n, st, &h_active, 0, decode_blind_iterations(max_dec), max_dec, nullptr, "offline decode")) return -1;
        // tokens of this window: at most 256 x 10 < TOK_CAP per slot, so the ring holds all of them
        HIPCHK(hipMemcpyAsync(hctrl.data(), o->dec.ctrl, (size_t)n * sizeof(DecCtrl), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ring.data(), o->dec.tok_ring, ring.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ringf.data(), o->dec.tok_frame, ringf.size() * 4, hipMemcpyDeviceToHost, st));
        if (!ringl.empty()) HIPCHK(hipMemcpyAsync(ringl.data(), o->dec.tok_logprob, ringl.size() * 4, hipMemcpyDeviceToHost, st));
        if (!ringb.empty()) HIPCHK(hipMemcpyAsync(ringb.data(), o->dec.frame_blank, ringb.size() * 4, hipMemcpyDeviceToHost, st));
        if (!ringe.empty()) HIPCHK(hipMemcpyAsync(ringe.data(), o->dec.tok_entropy, ringe.size() * 4, hipMemcpyDeviceToHost, st));
        if (K) {
            HIPCHK(hipMemcpyAsync(ringai.data(), o->dec.alt_id, ringai.size() * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(ringal.data(), o->dec.alt_lp, ringal.size() * 4, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        for (int k = 0; k < n; k++) {
            const int n_new = hctrl[k].n_tok - tok_read[k];
            if (n_new < 0 || n_new > TOK_CAP) return fail("offline token ring overrun on utterance %d", first + k);
            for (int i = 0; i < n_new; i++) {
                const int pos = (tok_read[k] + i) & (TOK_CAP - 1);
                toks[first + k].push_back(ring[(size_t)k * TOK_CAP + pos]);
                frs[first + k].push_back(ringf[(size_t)k * TOK_CAP + pos]);
                if (!ringl.empty()) o->logprobs[first + k].push_back(ringl[(size_t)k * TOK_CAP + pos]);
                if (!ringe.empty()) o->entropies[first + k].push_back(ringe[(size_t)k * TOK_CAP + pos]);
                if (K) {
                    const size_t at = ((size_t)k * TOK_CAP + pos) * K;
                    o->alt_ids[first + k].insert(o->alt_ids[first + k].end(), ringai.begin() + at, ringai.begin() + at + K);
                    o->alt_lps[first + k].insert(o->alt_lps[first + k].end(), ringal.begin() + at, ringal.begin() + at + K);
                }
            }
            tok_read[k] = hctrl[k].n_tok;
            // the frames of this window: the slot's frame count starts at 0 with the utterance, so frame g sits at ring position g
            if (!ringb.empty()) {
                const int nd = std::min(std::max(T[k] - w0, 0), OFF_DEC_WIN);
                if (hctrl[k].frame0 + hctrl[k].t != w0 + nd && nd > 0) return fail("offline decode left %d frames of utterance %d, expected %d", hctrl[k].frame0 + hctrl[k].t, first + k, w0 + nd);
                for (int g = w0; g < w0 + nd; g++) o->frame_blank_lps[first + k].push_back(ringb[(size_t)k * FRAME_CAP + (g & (FRAME_CAP - 1))]);
            }
        }
    }
    return 0;
}

// debug: room for the taps of B utterances, the log-mel kept at once
static int begin_taps(nasr_engine *e, OfflineState *o, int B, const float *const *mel, const int32_t *n_frames, bool mel_device) {
    if (!e->debug) return 0;
    o->tap_mel.assign(B, {}); o->tap_sub.assign(B, {}); o->tap_enc.assign(B, {}); o->tap_lay.assign(B, {});
    for (int b = 0; b < B; b++) {
        o->tap_mel[b].resize((size_t)n_frames[b] * NMEL);
        if (n_frames[b] > 0) HIPCHK(hipMemcpy(o->tap_mel[b].data(), mel[b], (size_t)n_frames[b] * NMEL * 4, mel_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
    }
    return 0;
}

// checks shared by every entry; prepares the offline state and forgets the taps of the previous call
static int begin_call(nasr_engine *e, int B, const int32_t *prompt_index, const int32_t *n_tokens, uint32_t flags, const char *who) {
    if (!n_tokens) return fail("%s: null n_tokens", who);
    if (flags & NASR_FLAG_NO_SYNC) return fail("%s: NASR_FLAG_NO_SYNC is not supported by the offline path", who);
    if (prompt_index && e->hp.num_prompts > 0)
        for (int b = 0; b < B; b++)
            if (prompt_index[b] < -1 || prompt_index[b] >= e->hp.num_prompts) return fail("prompt_index[%d] = %d out of range", b, prompt_index[b]);
    HIPCHK(hipSetDevice(e->device));
    if (pipe_drain(e)) return -1;                 // complete pipelined steps in flight, as every entry point does
    if (!e->off) e->off = new OfflineState();
    OfflineState *o = e->off;
    o->tap_mel.clear(); o->tap_sub.clear(); o->tap_enc.clear(); o->tap_lay.clear();
    o->logprobs.clear(); o->entropies.clear(); o->alt_ids.clear(); o->alt_lps.clear(); o->frame_blank_lps.clear();
    o->lat_valid = false; o->lat_b.clear(); o->lat_t.clear();
    o->beam_valid = false; o->beam_res.clear();
    o->no_boost = (flags & NASR_FLAG_NO_BOOST) != 0;
    o->no_lm = (flags & NASR_FLAG_NO_LM) != 0;
    return 0;
}

// whole-utterance log-mel on the device: the streaming front end (k_preemph / k_melframes / k_abuf_shift, the reference preprocessor with
// its 256-sample zero start, src/preprocessor.cpp:330-395) run over each utterance from a fresh state, in sub-pushes of MAX_PUSH samples --
// its result does not depend on how the samples are cut (tests/test_oracle_golden.py::test_mel_piece_size_independent), so this is the
// preprocessor run once over the whole utterance.  Frames land in o->pmel, utterance b at mel_off[b].
constexpr int PCM_GROUP = 32;                     // utterances whose preprocessor states exist at once
static int offline_mel(nasr_engine *e, OfflineState *o, int B, const int16_t *const *pcm, const int32_t *n_samples, bool pcm_device,
                       const std::vector<int32_t> &n_mel, std::vector<const float *> &mel_ptr) {
    hipStream_t st = e->st;
    std::vector<size_t> mel_off(B, 0);
    size_t total = 0;
    for (int b = 0; b < B; b++) {
        mel_off[b] = total;
        total += (size_t)n_mel[b];
    }
    if (!o->abuf) {
        if (off_alloc(o, (void **)&o->abuf, (size_t)PCM_GROUP * 2 * ABUF_CAP * 4) || off_alloc(o, (void **)&o->last_sample, PCM_GROUP * 4) ||
            off_alloc(o, (void **)&o->mel_ring, (size_t)PCM_GROUP * MEL_RING * NMEL * 4) || off_alloc(o, (void **)&o->pdesc, PCM_GROUP * sizeof(PcmDesc)))
            return -1;
    }
    if (grow(e, o, o->pmel, std::max<size_t>(total, 1) * NMEL * 4)) return -1;
    for (int g0 = 0; g0 < B; g0 += PCM_GROUP) {
        const int G = std::min(PCM_GROUP, B - g0);
        std::vector<const int16_t *> src(G, nullptr);
        if (pcm_device) {
            for (int k = 0; k < G; k++) src[k] = pcm[g0 + k];
        } else {
            size_t n = 0;
            for (int k = 0; k < G; k++) n += (size_t)n_samples[g0 + k];
            if (grow(e, o, o->pcm, std::max<size_t>(n, 1) * 2)) return -1;
            size_t at = 0;
            for (int k = 0; k < G; k++) {
                src[k] = o->pcm.as<int16_t>() + at;
                if (n_samples[g0 + k] > 0) HIPCHK(hipMemcpyAsync(o->pcm.as<int16_t>() + at, pcm[g0 + k], (size_t)n_samples[g0 + k] * 2, hipMemcpyHostToDevice, st));
                at += (size_t)n_samples[g0 + k];
            }
        }
        // fresh preprocessor state: 256 zero samples at parity 0, last sample 0 (k_stream_reset's values)
        for (int k = 0; k < G; k++) HIPCHK(hipMemsetAsync(o->abuf + (size_t)k * 2 * ABUF_CAP, 0, (NFFT / 2) * 4, st));
        HIPCHK(hipMemsetAsync(o->last_sample, 0, PCM_GROUP * 4, st));
        std::vector<int64_t> done(G, 0);
        std::vector<int> cnt(G, NFFT / 2), par(G, 0), made(G, 0);
        for (;;) {
            std::vector<PcmDesc> pd;
            std::vector<int> who;
            int max_frames = 0, max_n = 0;
            for (int k = 0; k < G; k++) {
                const int64_t rem = n_samples[g0 + k] - done[k];
                if (rem <= 0) continue;
                PcmDesc d;
                memset(&d, 0, sizeof(d));
                d.pcm = src[k] + done[k]; d.slot = k;
                fill_pcm_counts(d, (int)std::min<int64_t>(rem, MAX_PUSH), cnt[k], par[k], 0, 0);      // every sub-push writes from ring row 0; the frames are copied out below
                pd.push_back(d); who.push_back(k);
                max_frames = std::max(max_frames, d.n_frames); max_n = std::max(max_n, d.n);
            }
            if (pd.empty()) break;
            HIPCHK(hipMemcpyAsync(o->pdesc, pd.data(), pd.size() * sizeof(PcmDesc), hipMemcpyHostToDevice, st));
            MelParams mp;
            memset(&mp, 0, sizeof(mp));
            mp.desc = o->pdesc; mp.B = (int)pd.size(); mp.max_frames = max_frames; mp.abuf = o->abuf; mp.last_sample = o->last_sample;
            mp.mel_ring = o->mel_ring; mp.window = e->window; mp.fbT = e->fbT; mp.fb_band = e->fb_band; mp.cos_t = e->cos_t; mp.sin_t = e->sin_t;
            {
                ProfScope ps(e, "k_mel", 0, 0);
                launch_mel(mp, max_n, st);
            }
            for (size_t i = 0; i < pd.size(); i++) {
                const int k = who[i], b = g0 + k;
                if (pd[i].n_frames > 0) {
                    if (made[k] + pd[i].n_frames > n_mel[b]) return fail("internal: mel frame count of utterance %d", b);
                    HIPCHK(hipMemcpyAsync(o->pmel.as<float>() + (mel_off[b] + made[k]) * NMEL, o->mel_ring + (size_t)k * MEL_RING * NMEL,
                                          (size_t)pd[i].n_frames * NMEL * 4, hipMemcpyDeviceToDevice, st));
                    par[k] ^= 1;
                }
                made[k] += pd[i].n_frames;
                done[k] += pd[i].n;
                cnt[k] = pd[i].cnt + pd[i].n - pd[i].consumed;
            }
            // the descriptor block is rewritten by the next sub-push: the launches reading it must have run
            HIPCHK(hipStreamSynchronize(st));
        }
        for (int k = 0; k < G; k++)
            if (made[k] != n_mel[g0 + k]) return fail("internal: utterance %d gave %d mel frames, planned %d", g0 + k, made[k], n_mel[g0 + k]);
    }
    mel_ptr.assign(B, nullptr);
    for (int b = 0; b < B; b++) mel_ptr[b] = o->pmel.as<float>() + mel_off[b] * NMEL;
    return 0;
}
// the one wording of "an utterance is longer than NASR_OFFLINE_MAX_FRAMES"
static int fail_over_limit(const OffInput &in, const int32_t *n_mel, int bad, bool streaming_hint) {
    const char *hint = streaming_hint ? "; transcribe longer audio with the streaming path (nemotron-asr-amd)" : "";
    if (in.is_pcm)
        return fail("utterance %d: %d samples give %d encoder frames, more than NASR_OFFLINE_MAX_FRAMES = %d (the reference's max_pos_len, %.1f s)%s", bad,
                    bad >= 0 ? in.n[bad] : -1, bad >= 0 ? nasr_plan::enc_frames(n_mel[bad]) : -1, NASR_OFFLINE_MAX_FRAMES, nasr_plan::max_samples() / 16000.0, hint);
    if (bad >= 0 && n_mel[bad] >= 0)
        return fail("utterance %d: %d mel frames give %d encoder frames, more than NASR_OFFLINE_MAX_FRAMES = %d (the reference's max_pos_len)%s", bad, n_mel[bad],
                    nasr_plan::enc_frames(n_mel[bad]), NASR_OFFLINE_MAX_FRAMES, hint);
    return fail("offline plan rejected the call");
}

// ---- the third input kind: windows of live streams' frame history (engine option "frame_history", nasr_history.h) -----------------------------
// what can be said of the arguments before anything is completed or forgotten
static int history_check(nasr_engine *e, int B, const OffInput &in, const char *who) {
    if (!e->opt_frame_history) return fail("%s: %s", who, HISTORY_OFF);
    if (!in.streams || !in.first || !in.n) return fail("%s: null streams / first / count", who);
    for (int b = 0; b < B; b++) {
        if (!in.streams[b] || in.streams[b]->e != e) return fail("%s: streams[%d] does not belong to this engine", who, b);
        if (in.first[b] < 0 || in.n[b] < 0) return fail("%s: negative frame window [%lld, %lld + %d) of streams[%d]", who, (long long)in.first[b], (long long)in.first[b], in.n[b], b);
    }
    return 0;
}
// behind begin_call (the steps in flight are complete): every window against what its stream keeps, the one plan over the windows' frame
// counts, and per sub-batch the gather into o->encproj in place of front end, encoder and position tables; then the mode's batch step as ever.
// No stream is written: the gather reads the rings, the modes decode in the offline path's own slots
static int history_call(nasr_engine *e, OfflineState *o, int B, const OffInput &in, const OffMode &m) {
    const int N = e->opt_frame_history;
    std::map<const nasr_stream *, int64_t> done_of;               // the same stream may appear in several rows
    for (int b = 0; b < B; b++) {
        const nasr_stream *s = in.streams[b];
        if (!done_of.count(s) && stream_frames_done(s, &done_of[s])) return -1;
        const nasr_hist::Range kept = nasr_hist::retained(s->hist_valid_from, done_of[s], N);
        if (!nasr_hist::window_kept(kept, in.first[b], in.n[b]))
            return fail("%s: window [%lld, %lld) of streams[%d] is not wholly kept: the stream keeps frames [%lld, %lld) (engine option \"frame_history\" = %d)", m.who,
                        (long long)in.first[b], (long long)in.first[b] + in.n[b], b, (long long)kept.first, (long long)kept.first + kept.count, N);
    }
    std::vector<int> T;
    std::vector<nasr_plan::Batch> batches;
    int bad = -1;
    if (nasr_plan::plan_offline(in.n, B, e->opt_offline_rows, nasr_plan::OFFLINE_MAX_UTTS, T, batches, &bad, true))
        return fail("%s: window %d has %d frames, more than NASR_OFFLINE_MAX_FRAMES = %d", m.who, bad, bad >= 0 ? in.n[bad] : -1, NASR_OFFLINE_MAX_FRAMES);
    int64_t frames = 0;
    auto run = [&]() -> int {
        if (e->debug) { o->tap_mel.assign(B, {}); o->tap_sub.assign(B, {}); o->tap_enc.assign(B, {}); o->tap_lay.assign(B, {}); }      // no encoder ran: its taps are empty
        if (m.setup(o, B)) return -1;
        for (const auto &bt : batches) {
            OffBatch ob;
            ob.first = bt.first; ob.n = bt.count;
            ob.off.assign(bt.count, 0); ob.T.assign(bt.count, 0);
            std::vector<HistWindow> win(bt.count);
            for (int k = 0; k < bt.count; k++) {
                const int b = bt.first + k;
                ob.T[k] = T[b]; ob.off[k] = ob.M; ob.maxT = std::max(ob.maxT, T[b]);
                win[k] = HistWindow{(long long)in.first[b], in.streams[b]->slot, T[b], ob.M, 0};
                ob.M += T[b];
            }
            if (ob.M > 0) {
                if (ensure_dec_slots(e, o) || grow(e, o, o->encproj, (size_t)std::max(ob.M, 64) * JNT * 4)) return -1;
                const HistWindow *dwin;                              // through the pinned descriptor arena, like every step descriptor
                if (stage_desc(e, win, &dwin)) return -1;
                ProfScope ps(e, "k_history_gather", 2.0 * ob.M * nasr_hist::ROW_BYTES);
                launch_history_gather(dwin, bt.count, ob.maxT, e->hist_ring, N, o->encproj.as<float>(), e->st);
                frames += ob.M;
            }
            if (m.batch(o, ob)) return -1;
        }
        return 0;
    };
    if (run()) {
        if (m.failed) m.failed(o);
        return -1;
    }
    e->history_calls++;
    e->history_frames += frames;
    return m.finish(o, B);
}

// An offline call from the ABI's arguments to the caller's results.  The order is the contract of all six entries: a mode's early checks hold
// for B == 0 too; begin_call forgets the call before, so whatever fails behind it leaves no read-out of an earlier call; the limit is checked
// by the one plan before any device work; the mode's batch step also sees the sub-batches without a frame (ob.M == 0)
int offline_call(nasr_engine *e, int B, const OffInput &in, const int32_t *prompt_index, uint32_t flags, const OffMode &m) {
    if (!e) return fail("null engine");
    if (B < 0) return fail("B < 0");
    if (m.early && m.early()) return -1;
    if ((flags & NASR_FLAG_NO_LM) && !m.greedy) return fail("NASR_FLAG_NO_LM belongs to nasr_engine_transcribe / _transcribe_mel; the beam search is fused by nasr_engine_set_lm alone and alignment never is");
    if (B == 0) return 0;
    if (in.is_history) {
        if (history_check(e, B, in, m.who)) return -1;
    } else if (in.is_pcm) {
        if (!in.pcm || !in.n) return fail("null pcm / n_samples");
        for (int b = 0; b < B; b++)
            if (in.n[b] < 0 || (in.n[b] > 0 && !in.pcm[b])) return fail("bad pcm input for utterance %d", b);
    } else {
        if (!in.mel || !in.n) return fail("null mel / n_frames");
        for (int b = 0; b < B; b++)
            if (in.n[b] < 0 || (in.n[b] > 0 && !in.mel[b])) return fail("bad mel input for utterance %d", b);
    }
    if (begin_call(e, B, prompt_index, m.counts, flags, m.who)) return -1;
    OfflineState *o = e->off;
    if (m.check && m.check(B)) return -1;
    if (in.is_history) return history_call(e, o, B, in, m);
    std::vector<int32_t> pcm_mel(in.is_pcm ? B : 0);
    for (int b = 0; b < (int)pcm_mel.size(); b++) pcm_mel[b] = nasr_plan::mel_frames(in.n[b]);
    const int32_t *n_mel = in.is_pcm ? pcm_mel.data() : in.n;
    std::vector<int> T;
    std::vector<nasr_plan::Batch> batches;
    int bad = -1;
    if (nasr_plan::plan_offline(n_mel, B, e->opt_offline_rows, nasr_plan::OFFLINE_MAX_UTTS, T, batches, &bad)) return fail_over_limit(in, n_mel, bad, m.streaming_hint);
    std::vector<const float *> dev_mel;                       // PCM: the log-mel of every utterance in device memory
    if (in.is_pcm && offline_mel(e, o, B, in.pcm, in.n, (flags & NASR_FLAG_PCM_DEVICE) != 0, pcm_mel, dev_mel)) return -1;
    const float *const *mel = in.is_pcm ? dev_mel.data() : in.mel;
    auto run = [&]() -> int {
        if (ensure_offline_pos(e, o) || begin_taps(e, o, B, mel, n_mel, in.is_pcm) || m.setup(o, B)) return -1;
        for (const auto &bt : batches) {
            OffBatch ob;
            if (run_offline_encoder(e, o, mel, n_mel, prompt_index, T, bt.first, bt.count, ob) || m.batch(o, ob)) return -1;
            if (e->debug && ob.M > 0 && fetch_offline_taps(e, o, ob)) return -1;
        }
        return 0;
    };
    if (run()) {
        if (m.failed) m.failed(o);
        return -1;
    }
    return m.finish(o, B);
}

// the greedy mode: tokens and their frames per utterance, with the engine options' per-token values kept for the read-outs below
static OffMode greedy_mode(nasr_engine *e, const char *who, int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens, int32_t *const *frames_out) {
    struct Run { std::vector<std::vector<int32_t>> toks, frs; };
    auto r = std::make_shared<Run>();
    OffMode m;
    m.who = who; m.counts = n_tokens; m.streaming_hint = true; m.greedy = true;
    m.setup = [=](OfflineState *o, int B) {
        o->logprobs.assign(e->opt_token_logprobs ? B : 0, {});
        o->entropies.assign(e->opt_token_entropy ? B : 0, {});
        o->frame_blank_lps.assign(e->opt_frame_blank ? B : 0, {});
        o->alt_ids.assign(e->opt_token_alt ? B : 0, {}); o->alt_lps.assign(e->opt_token_alt ? B : 0, {});
        r->toks.assign(B, {}); r->frs.assign(B, {});
        return 0;
    };
    m.batch = [=](OfflineState *o, const OffBatch &ob) { return run_offline_batch(e, o, ob, r->toks, r->frs); };
    m.finish = [=](OfflineState *, int B) {
        for (int b = 0; b < B; b++) {
            n_tokens[b] = (int32_t)r->toks[b].size();
            const int cap = tokens_cap ? std::max(tokens_cap[b], 0) : 0;
            const int n_copy = std::min((int)r->toks[b].size(), cap);
            if (tokens_out && tokens_out[b]) for (int i = 0; i < n_copy; i++) tokens_out[b][i] = r->toks[b][i];
            if (frames_out && frames_out[b]) for (int i = 0; i < n_copy; i++) frames_out[b][i] = r->frs[b][i];
        }
        return 0;
    };
    return m;
}
}  // namespace nasr_eng

extern "C" int nasr_engine_transcribe_mel(nasr_engine *e, int B, const float *const *mel, const int32_t *n_frames,
                                          const int32_t *prompt_index, int32_t *const *tokens_out, const int32_t *tokens_cap,
                                          int32_t *n_tokens, int32_t *const *frames_out, uint32_t flags) {
    ApiGuard api_guard;
    return offline_call(e, B, mel_input(mel, n_frames), prompt_index, flags,
                        greedy_mode(e, "nasr_engine_transcribe_mel", tokens_out, tokens_cap, n_tokens, frames_out));
}

extern "C" int nasr_engine_transcribe(nasr_engine *e, int B, const int16_t *const *pcm, const int32_t *n_samples,
                                      const int32_t *prompt_index, int32_t *const *tokens_out, const int32_t *tokens_cap,
                                      int32_t *n_tokens, int32_t *const *frames_out, uint32_t flags) {
    ApiGuard api_guard;
    return offline_call(e, B, pcm_input(pcm, n_samples), prompt_index, flags,
                        greedy_mode(e, "nasr_engine_transcribe", tokens_out, tokens_cap, n_tokens, frames_out));
}

extern "C" int nasr_engine_history_transcribe(nasr_engine *e, nasr_stream *const *streams, int B, const int64_t *first, const int32_t *count,
                                              int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens, int32_t *const *frames_out, uint32_t flags) {
    ApiGuard api_guard;
    return offline_call(e, B, history_input(streams, first, count), nullptr, flags,
                        greedy_mode(e, "nasr_engine_history_transcribe", tokens_out, tokens_cap, n_tokens, frames_out));
}

extern "C" int64_t nasr_engine_offline_tap(nasr_engine *e, int which, int u, int index, float *out, int64_t cap) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    OfflineState *o = e->off;
    if (!o || u < 0 || u >= (int)o->tap_mel.size()) return fail("no offline tap of utterance %d (the last offline call must run with nasr_engine_set_debug(e, 1))", u);
    const std::vector<float> *src = nullptr;
    if (which == NASR_TAP_MEL) src = &o->tap_mel[u];
    else if (which == NASR_TAP_SUBSAMPLED) src = &o->tap_sub[u];
    else if (which == NASR_TAP_ENCODER_OUT) src = &o->tap_enc[u];
    else if (which == NASR_TAP_LAYER_OUT) {
        if (index < 0 || index >= (int)o->tap_lay[u].size()) {
            if (o->tap_lay[u].empty() && index >= 0 && index < e->hp.n_layers) src = nullptr;      // an utterance with no encoder frames
            else return fail("layer %d out of range", index);
        } else src = &o->tap_lay[u][index];
    } else return fail("offline tap %d not available", which);
    if (!src) { static const std::vector<float> none; src = &none; }
    if (!out) return (int64_t)src->size();                  // size query
    const int64_t n = std::min<int64_t>((int64_t)src->size(), cap);
    memcpy(out, src->data(), (size_t)n * 4);
    return n;
}

extern "C" int nasr_engine_offline_token_logprobs(nasr_engine *e, int u, float *out, int32_t cap) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    if (!e->opt_token_logprobs) return fail("no token log-probabilities: engine option \"token_logprobs\" is off (set it to 1 before the first step or offline call)");
    OfflineState *o = e->off;
    if (!o || u < 0 || u >= (int)o->logprobs.size()) return fail("no offline token log-probabilities of utterance %d (they are those of the last offline call)", u);
    return (int)read_out(o->logprobs[u], out, cap);
}

extern "C" int nasr_engine_offline_token_entropies(nasr_engine *e, int u, float *out, int32_t cap) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    if (!e->opt_token_entropy) return fail("no token entropies: engine option \"token_entropy\" is off (set it to round(1000 alpha) before the first step or offline call)");
    OfflineState *o = e->off;
    if (!o || u < 0 || u >= (int)o->entropies.size()) return fail("no offline token entropies of utterance %d (they are those of the last offline call)", u);
    return (int)read_out(o->entropies[u], out, cap);
}

extern "C" int nasr_engine_offline_frame_blank_logprobs(nasr_engine *e, int u, float *out, int32_t cap) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    if (!e->opt_frame_blank) return fail("no per-frame blank log-probabilities: engine option \"frame_blank_logprobs\" is off (set it to 1 before the first step or offline call)");
    OfflineState *o = e->off;
    if (!o || u < 0 || u >= (int)o->frame_blank_lps.size()) return fail("no offline blank log-probabilities of utterance %d (they are those of the last offline call)", u);
    return (int)read_out(o->frame_blank_lps[u], out, cap);
}

extern "C" int nasr_engine_offline_token_alternatives(nasr_engine *e, int u, int32_t *ids_out, float *logprobs_out, int32_t cap) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    const int K = e->opt_token_alt;
    if (!K) return fail("no token alternatives: engine option \"token_alternatives\" is off (set it to K = 1 .. 8 before the first step or offline call)");
    OfflineState *o = e->off;
    if (!o || u < 0 || u >= (int)o->alt_ids.size()) return fail("no offline token alternatives of utterance %d (they are those of the last offline call)", u);
    const int have = (int)(o->alt_ids[u].size() / (size_t)K);
    if (!ids_out) return have;                              // size query, in tokens
    if (!logprobs_out) return fail("null argument");
    const int n = std::min<int>(have, std::max(cap, 0));
    memcpy(ids_out, o->alt_ids[u].data(), (size_t)n * K * 4);
    memcpy(logprobs_out, o->alt_lps[u].data(), (size_t)n * K * 4);
    return n;
}
