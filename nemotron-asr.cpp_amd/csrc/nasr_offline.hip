// nasr_offline.hip -- offline full-context transcription of whole utterances, batched (nasr_engine_transcribe_mel).
// Replaces nemo_transcribe_audio / nemo_encode (reference src/nemo-ggml.cpp:1600-1737): the preprocessor output of a whole
// utterance -> ConvSubsampling without drop-2 -> 24 conformer layers whose attention sees every frame of the utterance
// (build_rel_pos_mha :668-755, no mask, no cache; the depthwise conv starts from a zero history) -> prompt fusion -> greedy
// RNN-T decode (:1231-).  The utterances of a call are packed densely (M = sum T_b rows, no padding) and cut into sub-batches
// of at most "offline_rows" rows (nasr_offline_plan.h); every kernel's result for a row depends on its own utterance only, so
// a sub-batch gives the bits the utterance gives alone.  Nothing of the streaming state is touched: the path has its own
// buffers (allocated on the first call), its own decoder slots and token rings, and never captures a graph.
#include "nasr_engine_priv.h"
#include "nasr_offline.h"

struct OfflineState {
    std::vector<void *> bufs;                    // everything below, freed with the engine (or when a buffer grows)
    int rows_cap = 0;
    size_t part_cap = 0, sub_a_cap = 0, sub_b_cap = 0, mel_cap = 0;
    float *x = nullptr, *part = nullptr, *glu = nullptr, *hfuse = nullptr, *encproj = nullptr, *zero_bias = nullptr;
    void *a = nullptr, *hbuf = nullptr, *qkv = nullptr, *ctx = nullptr, *cbuf = nullptr;
    int *tpos = nullptr; int4 *items = nullptr; RowDesc *prow = nullptr;
    void *sub_a = nullptr, *sub_b = nullptr;     // front-end images (f32 sized)
    float *mel = nullptr;
    // PCM entry: the streaming front end's buffers for a group of utterances (one preprocessor state each) and the log-mel it produces
    float *abuf = nullptr, *last_sample = nullptr, *mel_ring = nullptr, *pmel = nullptr; int16_t *pcm = nullptr; PcmDesc *pdesc = nullptr;
    size_t pmel_cap = 0, pcm_cap = 0;
    OffSubDesc *sdesc = nullptr;
    std::vector<void *> pos;                     // per layer [4095][1024] act dtype
    // decode: one slot per utterance of a sub-batch
    DecCtrl *ctrl = nullptr; float *h = nullptr, *c = nullptr, *predg = nullptr, *win = nullptr;
    unsigned long long *key = nullptr; int *n_active = nullptr, *dlist = nullptr, *tok_ring = nullptr, *tok_frame = nullptr;
    unsigned *rowmap = nullptr; RowDesc *drows = nullptr; int4 *dwin = nullptr;
    nasr_lp::Part *lp_part = nullptr; float *tok_logprob = nullptr;      // engine option "token_logprobs" (allocated with the slots when it is on)
    int *boost_state = nullptr; float *boost_raw = nullptr;        // engine option "phrase_boost": the offline slots' automaton states (the tables are the engine's)
    bool no_boost = false;                                         // NASR_FLAG_NO_BOOST of the call in progress
    unsigned long long *alt_key = nullptr; int32_t *alt_id = nullptr; float *alt_lp = nullptr;      // engine option "token_alternatives"
    std::vector<std::vector<int32_t>> alt_ids; std::vector<std::vector<float>> alt_lps;             // ... of the last call, by utterance: [tokens][K] each
    float *fb_row = nullptr, *frame_blank = nullptr;               // engine option "frame_blank_logprobs": scratch [U * W] and a ring [U][FRAME_CAP] (T <= 2048 < FRAME_CAP)
    std::vector<std::vector<float>> frame_blank_lps;               // ... of the last call, by utterance: [T] (nasr_engine_offline_frame_blank_logprobs)
    std::vector<std::vector<float>> logprobs;                      // ... of the last call, by utterance (nasr_engine_offline_token_logprobs)
    // forced alignment (nasr_engine_align*): the prediction-network rows g, the lattice of the sub-batch in flight (two values and one
    // back-pointer byte per cell), its descriptors and its results
    float *al_g = nullptr, *al_lpb = nullptr, *al_lpt = nullptr, *al_tlp = nullptr;
    unsigned char *al_bp = nullptr;
    nasr_align::Utt *al_utt = nullptr; nasr_align::Tile *al_tiles = nullptr;
    int32_t *al_tok = nullptr, *al_frames = nullptr; double *al_scores = nullptr;
    size_t al_g_cap = 0, al_lpb_cap = 0, al_lpt_cap = 0, al_tlp_cap = 0, al_bp_cap = 0, al_tiles_cap = 0, al_tok_cap = 0, al_frames_cap = 0;
    bool lat_valid = false;                                        // the last call was an align call with debug on
    std::vector<std::vector<float>> lat_b, lat_t;                  // ... its lattices by utterance: lp_blank, lp_token [T][U + 1]
    // beam search (nasr_engine_transcribe_beam*): its own decoder slots (3 W per utterance), batch rows (W per utterance), the joint's LP + ALT
    // scratch whatever the engine options are, the search state and trie of the sub-batch in flight, and the results of the last call
    struct BeamBuf { void *p = nullptr; size_t cap = 0; };
    BeamBuf bm_utt, bm_beam, bm_nodes, bm_enc, bm_rows, bm_ctrl, bm_h, bm_c, bm_predg, bm_key, bm_part, bm_alt, bm_cnt, bm_dlist, bm_rowmap, bm_out_lm, bm_bstate, bm_raw, bm_out_boost,
            bm_out_n, bm_out_len, bm_out_score, bm_out_tok, bm_out_frame, bm_out_lp;
    struct BeamHyp { double score; std::vector<int32_t> tokens, frames; std::vector<float> lps; double lm_final = 0.0, total = 0.0;
                     double boost = 0.0; std::vector<float> bonuses; };     // a boosted call: the sum and the per-token bonuses by the set in force during it
    long long beam_lm_generation = 0;                              // the engine's lm_generation at that call
    bool beam_valid = false, beam_lm = false;                      // beam_lm: the last beam call ran with a language model (nasr_engine_set_lm)
    bool beam_boost = false;                                       // the last beam call was boosted (NASR_FLAG_BEAM_BOOST)
    std::vector<std::vector<BeamHyp>> beam_res;                    // by utterance, best first
    float *t_sub = nullptr, *t_lay = nullptr, *t_enc = nullptr;   // debug taps of the sub-batch in flight
    // debug taps of the last call, by utterance
    std::vector<std::vector<float>> tap_mel, tap_sub, tap_enc;
    std::vector<std::vector<std::vector<float>>> tap_lay;
};

namespace nasr_eng {

static int off_alloc(OfflineState *o, void **p, size_t bytes) {
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

// row buffers for `rows` packed rows (grown, never shrunk) and the decode slots
static int ensure_rows(nasr_engine *e, OfflineState *o, int rows) {
    if (rows <= o->rows_cap) return 0;
    HIPCHK(hipStreamSynchronize(e->st));
    void **row_bufs[] = {(void **)&o->x, (void **)&o->glu, (void **)&o->hfuse, (void **)&o->encproj, &o->a, &o->hbuf, &o->qkv, &o->ctx,
                         &o->cbuf, (void **)&o->tpos, (void **)&o->items, (void **)&o->prow};
    for (void **p : row_bufs) { off_free(o, *p); *p = nullptr; }
    const size_t M = (size_t)std::max(rows, 64), es = e->esz;
    int rc = 0;
    rc |= off_alloc(o, (void **)&o->x, M * D * 4);
    rc |= off_alloc(o, (void **)&o->glu, M * D * 4);
    rc |= off_alloc(o, (void **)&o->hfuse, e->hp.num_prompts > 0 ? M * 2048 * 4 : 16);
    rc |= off_alloc(o, (void **)&o->encproj, M * JNT * 4);
    rc |= off_alloc(o, &o->a, M * D * es);
    rc |= off_alloc(o, &o->hbuf, M * FF * es);
    rc |= off_alloc(o, &o->qkv, M * 3 * D * es);
    rc |= off_alloc(o, &o->ctx, M * D * es);
    rc |= off_alloc(o, &o->cbuf, M * D * es);
    rc |= off_alloc(o, (void **)&o->tpos, M * 4);
    rc |= off_alloc(o, (void **)&o->items, M * sizeof(int4));        // at most one attention work item per row
    rc |= off_alloc(o, (void **)&o->prow, M * sizeof(RowDesc));
    if (rc) return -1;
    o->rows_cap = (int)M;
    if (!o->zero_bias) {
        if (off_alloc(o, (void **)&o->zero_bias, 3 * D * 4)) return -1;
        HIPCHK(hipMemset(o->zero_bias, 0, 3 * D * 4));
    }
    if (!o->ctrl) {
        const size_t U = nasr_plan::OFFLINE_MAX_UTTS, W = OFF_DEC_WIN;
        rc |= off_alloc(o, (void **)&o->ctrl, U * sizeof(DecCtrl));
        rc |= off_alloc(o, (void **)&o->h, U * 4 * HID * 4);
        rc |= off_alloc(o, (void **)&o->c, U * 4 * HID * 4);
        rc |= off_alloc(o, (void **)&o->predg, U * JNT * 4);
        rc |= off_alloc(o, (void **)&o->win, U * W * JNT * 4);
        rc |= off_alloc(o, (void **)&o->key, U * W * 8);
        rc |= off_alloc(o, (void **)&o->n_active, 16);
        rc |= off_alloc(o, (void **)&o->dlist, U * 4);
        rc |= off_alloc(o, (void **)&o->rowmap, U * W * 4);
        rc |= off_alloc(o, (void **)&o->tok_ring, U * TOK_CAP * 4);
        rc |= off_alloc(o, (void **)&o->tok_frame, U * TOK_CAP * 4);
        if (e->opt_token_alt) {
            rc |= off_alloc(o, (void **)&o->alt_key, nasr_topk::scratch_keys((int)(U * W), e->opt_token_alt) * sizeof(unsigned long long));
            rc |= off_alloc(o, (void **)&o->alt_id, U * TOK_CAP * e->opt_token_alt * 4);
            rc |= off_alloc(o, (void **)&o->alt_lp, U * TOK_CAP * e->opt_token_alt * 4);
        }
        if (e->opt_frame_blank) {
            rc |= off_alloc(o, (void **)&o->fb_row, U * W * 4);
            rc |= off_alloc(o, (void **)&o->frame_blank, U * FRAME_CAP * 4);
        }
        if (e->opt_token_logprobs || e->opt_token_alt || e->opt_frame_blank) {
            rc |= off_alloc(o, (void **)&o->lp_part, nasr_lp::scratch_parts((int)(U * W)) * sizeof(nasr_lp::Part));
            rc |= off_alloc(o, (void **)&o->tok_logprob, U * TOK_CAP * 4);
        }
        if (e->opt_phrase_boost) {
            rc |= off_alloc(o, (void **)&o->boost_state, U * 4);
            rc |= off_alloc(o, (void **)&o->boost_raw, nasr_lp::scratch_parts((int)(U * W)) * 4);
        }
        rc |= off_alloc(o, (void **)&o->drows, U * sizeof(RowDesc));
        rc |= off_alloc(o, (void **)&o->dwin, U * sizeof(int4));
        rc |= off_alloc(o, (void **)&o->sdesc, U * sizeof(OffSubDesc));
        if (rc) return -1;
        HIPCHK(hipMemset(o->n_active, 0, 16));
    }
    return 0;
}

static int grow(nasr_engine *e, OfflineState *o, void **p, size_t &cap, size_t bytes) {
    if (bytes <= cap) return 0;
    HIPCHK(hipStreamSynchronize(e->st));
    off_free(o, *p);
    *p = nullptr;
    if (off_alloc(o, p, bytes)) return -1;
    cap = bytes;
    return 0;
}

// a sub-batch whose encoder has been enqueued: utterances [first, first + n) of the call, utterance first + k in packed rows
// [off[k], off[k] + T[k]) of o->encproj (and of the debug taps)
struct OffBatch { int first = 0, n = 0, M = 0, maxT = 0; std::vector<int> off, T; };

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
    HIPCHK(hipMemcpy(o->items, items.data(), items.size() * sizeof(int4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o->tpos, tpos.data(), (size_t)M * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o->prow, prow.data(), (size_t)M * sizeof(RowDesc), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o->sdesc, sd.data(), (size_t)n * sizeof(OffSubDesc), hipMemcpyHostToDevice));
    // Every GEMM of the path runs on at least OFF_MIN_ROWS rows (the rows past M are scratch whose results nobody reads) and without
    // split-K: the GEMM form -- and with it the summation order of every output row -- is then the same whatever the rows of the other
    // utterances, which is what makes a batch bit-identical to its utterances alone (the skinny kernel below 33 rows and split-K sum
    // differently; the large-M variants give the same bits, tests/micro/gemm_variant_identity.py).
    auto gm = [](int rows) { return std::max(rows, OFF_MIN_ROWS); };
    const int Mg = gm(M);
    if (grow(e, o, (void **)&o->part, o->part_cap, (size_t)Mg * D * 4)) return -1;
    // front-end images: conv0+dw output [H2][33][256] act, pw3 output f32, dw output [H3][17][256] act, pw6 output act
    const size_t img = std::max({(size_t)gm(h2_rows * 33), (size_t)gm(h3_rows * 17), (size_t)Mg * 17}) * SUBC * 4;
    if (grow(e, o, &o->sub_a, o->sub_a_cap, img) || grow(e, o, &o->sub_b, o->sub_b_cap, img)) return -1;
    if (grow(e, o, (void **)&o->mel, o->mel_cap, (size_t)std::max(mel_rows, 1) * NMEL * 4)) return -1;
    for (int k = 0; k < n; k++)
        if (n_mel[first + k] > 0)
            HIPCHK(hipMemcpyAsync(o->mel + (size_t)sd[k].mel_off * NMEL, mel[first + k], (size_t)n_mel[first + k] * NMEL * 4, hipMemcpyDefault, st));   // host (mel entry) or device (PCM entry)
    // debug taps of this sub-batch
    if (e->debug) {
        off_free(o, o->t_sub); off_free(o, o->t_lay); off_free(o, o->t_enc);
        if (off_alloc(o, (void **)&o->t_sub, (size_t)M * D * 4) || off_alloc(o, (void **)&o->t_lay, (size_t)nL * M * D * 4) ||
            off_alloc(o, (void **)&o->t_enc, (size_t)M * D * 4)) return -1;
    }
    // ---- subsampling over every whole utterance (no drop-2) ------------------------------------------------------
    {
        ProfScope ps(e, "k_off_conv0_dw", (double)mel_rows * NMEL * 4 + (double)h2_rows * 33 * SUBC * e->esz, 2.0 * h2_rows * 33 * SUBC * 90);
        launch_off_conv0_dw(o->sdesc, n, max_h2, o->mel, e->w0t, e->b0, e->w2t, e->b2, o->sub_b, act, st);
    }
    run_sub_pw3(e, o->sub_b, (float *)o->sub_a, gm(h2_rows * 33));
    {
        ProfScope ps(e, "k_sub_dw", (double)h2_rows * 33 * SUBC * 4, 2.0 * h3_rows * 17 * SUBC * 9);
        int r3 = 0;
        for (int k = 0; k < n; k++) {
            const int h2 = nasr_plan::sub_h2(n_mel[first + k]);
            if (h2 == 0) continue;
            launch_sub_dw((const float *)o->sub_a + (size_t)sd[k].out_row * 33 * SUBC, 1, h2, 33, e->w5t, e->b5,
                          (char *)o->sub_b + (size_t)r3 * 17 * SUBC * e->esz, act, st);
            r3 += T[k];
        }
    }
    run_sub_pw6(e, o->sub_b, o->sub_a, gm(h3_rows * 17));
    run_sub_out(e, o->sub_a, o->x, Mg);
    if (e->debug) HIPCHK(hipMemcpyAsync(o->t_sub, o->x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));

    // ---- conformer layers over all M rows ------------------------------------------------------------------------
    LayerRun r;
    r.x = o->x; r.part = o->part; r.glu = o->glu; r.a = o->a; r.hbuf = o->hbuf; r.ctx = o->ctx; r.cbuf = o->cbuf;
    r.M = M; r.Mg = Mg;
    r.split_k = false;
    r.chain = false;
    // q | k | v of every row (no ring: the offline layer has no cache)
    r.qkv_out = [&](int, GemmParams &g) { g.epi = EPI_BIAS_ACT; g.out_act = o->qkv; g.ldo_act = 3 * D; g.bias = o->zero_bias; };
    r.attention = [&](int l) {
        const LayerW &L = e->L[l];
        OffAttnParams ap;
        ap.qkv = o->qkv; ap.pos = o->pos[l]; ap.bias_u = L.bias_u; ap.bias_v = L.bias_v; ap.items = o->items; ap.ctx = o->ctx;
        double sq = 0;
        for (int k = 0; k < n; k++) sq += (double)T[k] * T[k];
        ProfScope ps(e, "k_off_attention", (double)M * 4 * D * e->esz, sq * NH * DH * 6.0);
        launch_off_attention(ap, (int)items.size(), act, st);
    };
    r.dwconv = [&](int l) {
        const LayerW &L = e->L[l];
        ProfScope ps(e, "k_off_dwconv", (double)M * D * (4 + e->esz), 2.0 * M * D * ks);
        launch_off_dwconv(o->glu, o->tpos, M, L.dw, ks, L.cln_w, L.cln_b, o->cbuf, act, st);
    };
    if (e->debug) r.tap = [&](int l) -> int {
        HIPCHK(hipMemcpyAsync(o->t_lay + (size_t)l * M * D, o->x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
        return 0;
    };
    if (enqueue_layers(e, r, 0, nL)) return -1;
    // ---- prompt fusion (one prompt per row), the joint's encoder projection ------------------------------------------
    if (enqueue_encoder_tail(e, o->x, o->hfuse, o->encproj, o->prow, M, Mg, 1, [&]() -> int {
            if (e->debug) HIPCHK(hipMemcpyAsync(o->t_enc, o->x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
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

// one sub-batch: utterances [first, first + n) of the call; tokens / frames appended to toks[b] / frs[b]
static int run_offline_batch(nasr_engine *e, OfflineState *o, const float *const *mel, const int32_t *n_mel, const int32_t *prompt_index,
                             const std::vector<int> &Tall, int first, int n, std::vector<std::vector<int32_t>> &toks,
                             std::vector<std::vector<int32_t>> &frs) {
    hipStream_t st = e->st;
    OffBatch ob;
    if (run_offline_encoder(e, o, mel, n_mel, prompt_index, Tall, first, n, ob)) return -1;
    if (ob.M == 0) return 0;
    const std::vector<int> &off = ob.off, &T = ob.T;
    const int maxT = ob.maxT;
    // ---- greedy decode in windows of 256 frames per utterance (token ring: 4096 > 256 x 10 symbols) -----------------
    launch_off_dec_reset(n, o->h, o->c, o->ctrl, st);
    if (o->boost_state)                                          // every utterance starts with an empty history (NASR_FLAG_NO_BOOST: in the disabled state)
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)o->boost_state, o->no_boost ? nasr_boost::STATE_OFF : nasr_boost::STATE_ROOT, (size_t)n, st));
    std::vector<int> tok_read(n, 0);
    std::vector<DecCtrl> hctrl(n);
    std::vector<int> ring((size_t)n * TOK_CAP), ringf((size_t)n * TOK_CAP);
    std::vector<float> ringl(e->opt_token_logprobs ? (size_t)n * TOK_CAP : 0);
    std::vector<float> ringb(e->opt_frame_blank ? (size_t)n * FRAME_CAP : 0);
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
        launch_off_window(o->encproj, o->dwin, n, OFF_DEC_WIN, o->win, st);
        DecParams dp;
        memset(&dp, 0, sizeof(dp));
        dp.rows = o->drows; dp.B = n; dp.T = OFF_DEC_WIN; dp.ctrl = o->ctrl; dp.h = o->h; dp.c = o->c; dp.encproj = o->win;
        bind_dec_weights(e, dp);
        dp.predg = o->predg; dp.key = o->key; dp.n_active = o->n_active; dp.n_dirty = o->n_active + 1; dp.n_rows = o->n_active + 2;
        dp.dlist = o->dlist; dp.rowmap = o->rowmap; dp.tok_ring = o->tok_ring; dp.tok_frame = o->tok_frame;
        dp.lp_part = o->lp_part; dp.tok_logprob = o->tok_logprob;       // null unless "token_logprobs" or "token_alternatives"
        if (K) { dp.alt_key = o->alt_key; dp.alt_id = o->alt_id; dp.alt_lp = o->alt_lp; dp.alt_k = K; }
        dp.fb_row = o->fb_row; dp.frame_blank = o->frame_blank;         // null unless "frame_blank_logprobs"
        if (o->boost_state) { dp.boost_bonus = e->boost_bonus; dp.boost_next = e->boost_next; dp.boost_state = o->boost_state; dp.boost_raw = o->boost_raw; }
        launch_decode_begin(dp, st);
        int h_active = 0;
        if (decode_until_idle(e, dp, n, st, &h_active, 0, decode_blind_iterations(max_dec), max_dec, nullptr, "offline decode")) return -1;
        // tokens of this window: at most 256 x 10 < TOK_CAP per slot, so the ring holds all of them
        HIPCHK(hipMemcpyAsync(hctrl.data(), o->ctrl, (size_t)n * sizeof(DecCtrl), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ring.data(), o->tok_ring, ring.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ringf.data(), o->tok_frame, ringf.size() * 4, hipMemcpyDeviceToHost, st));
        if (!ringl.empty()) HIPCHK(hipMemcpyAsync(ringl.data(), o->tok_logprob, ringl.size() * 4, hipMemcpyDeviceToHost, st));
        if (!ringb.empty()) HIPCHK(hipMemcpyAsync(ringb.data(), o->frame_blank, ringb.size() * 4, hipMemcpyDeviceToHost, st));
        if (K) {
            HIPCHK(hipMemcpyAsync(ringai.data(), o->alt_id, ringai.size() * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(ringal.data(), o->alt_lp, ringal.size() * 4, hipMemcpyDeviceToHost, st));
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
    if (e->debug && fetch_offline_taps(e, o, ob)) return -1;
    return 0;
}

}  // namespace nasr_eng

namespace nasr_eng {
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

// the call once the log-mel of every utterance exists: mel[b] in host memory (mel entry) or device memory (PCM entry)
static int transcribe_core(nasr_engine *e, int B, const float *const *mel, const int32_t *n_frames, bool mel_device, const int32_t *prompt_index,
                           int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens, int32_t *const *frames_out) {
    OfflineState *o = e->off;
    std::vector<int> T;
    std::vector<nasr_plan::Batch> batches;
    int bad = -1;
    if (nasr_plan::plan_offline(n_frames, B, e->opt_offline_rows, nasr_plan::OFFLINE_MAX_UTTS, T, batches, &bad)) {
        if (bad >= 0 && n_frames[bad] >= 0)
            return fail("utterance %d: %d mel frames give %d encoder frames, more than NASR_OFFLINE_MAX_FRAMES = %d (the reference's max_pos_len); "
                        "transcribe longer audio with the streaming path (nemotron-asr-amd)", bad, n_frames[bad], nasr_plan::enc_frames(n_frames[bad]),
                        NASR_OFFLINE_MAX_FRAMES);
        return fail("offline plan rejected the call");
    }
    if (ensure_offline_pos(e, o)) return -1;
    o->logprobs.assign(e->opt_token_logprobs ? B : 0, {});
    o->frame_blank_lps.assign(e->opt_frame_blank ? B : 0, {});
    o->alt_ids.assign(e->opt_token_alt ? B : 0, {}); o->alt_lps.assign(e->opt_token_alt ? B : 0, {});
    if (begin_taps(e, o, B, mel, n_frames, mel_device)) return -1;
    std::vector<std::vector<int32_t>> toks(B), frs(B);
    for (const auto &bt : batches)
        if (run_offline_batch(e, o, mel, n_frames, prompt_index, T, bt.first, bt.count, toks, frs)) return -1;
    for (int b = 0; b < B; b++) {
        n_tokens[b] = (int32_t)toks[b].size();
        const int cap = tokens_cap ? std::max(tokens_cap[b], 0) : 0;
        const int n_copy = std::min((int)toks[b].size(), cap);
        if (tokens_out && tokens_out[b]) for (int i = 0; i < n_copy; i++) tokens_out[b][i] = toks[b][i];
        if (frames_out && frames_out[b]) for (int i = 0; i < n_copy; i++) frames_out[b][i] = frs[b][i];
    }
    return 0;
}

// checks shared by both entries; prepares the offline state and forgets the taps of the previous call
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
    o->logprobs.clear(); o->alt_ids.clear(); o->alt_lps.clear(); o->frame_blank_lps.clear();
    o->lat_valid = false; o->lat_b.clear(); o->lat_t.clear();
    o->beam_valid = false; o->beam_res.clear();
    o->no_boost = (flags & NASR_FLAG_NO_BOOST) != 0;
    return 0;
}

// whole-utterance log-mel on the device: the streaming front end (k_preemph / k_melframes / k_abuf_shift, the reference preprocessor with
// its 256-sample zero start, src/preprocessor.cpp:330-395) run over each utterance from a fresh state, in sub-pushes of MAX_PUSH samples --
// its result does not depend on how the samples are cut (tests/test_oracle_golden.py::test_mel_piece_size_independent), so this is the
// preprocessor run once over the whole utterance.  Frames land in o->pmel, utterance b at mel_off[b].
constexpr int PCM_GROUP = 32;                     // utterances whose preprocessor states exist at once
static int offline_mel(nasr_engine *e, OfflineState *o, int B, const int16_t *const *pcm, const int32_t *n_samples, bool pcm_device,
                       std::vector<int32_t> &n_mel, std::vector<const float *> &mel_ptr) {
    hipStream_t st = e->st;
    n_mel.assign(B, 0);
    std::vector<size_t> mel_off(B, 0);
    size_t total = 0;
    for (int b = 0; b < B; b++) {
        n_mel[b] = nasr_plan::mel_frames(n_samples[b]);
        mel_off[b] = total;
        total += (size_t)n_mel[b];
    }
    if (!o->abuf) {
        if (off_alloc(o, (void **)&o->abuf, (size_t)PCM_GROUP * 2 * ABUF_CAP * 4) || off_alloc(o, (void **)&o->last_sample, PCM_GROUP * 4) ||
            off_alloc(o, (void **)&o->mel_ring, (size_t)PCM_GROUP * MEL_RING * NMEL * 4) || off_alloc(o, (void **)&o->pdesc, PCM_GROUP * sizeof(PcmDesc)))
            return -1;
    }
    if (grow(e, o, (void **)&o->pmel, o->pmel_cap, std::max<size_t>(total, 1) * NMEL * 4)) return -1;
    for (int g0 = 0; g0 < B; g0 += PCM_GROUP) {
        const int G = std::min(PCM_GROUP, B - g0);
        std::vector<const int16_t *> src(G, nullptr);
        if (pcm_device) {
            for (int k = 0; k < G; k++) src[k] = pcm[g0 + k];
        } else {
            size_t n = 0;
            for (int k = 0; k < G; k++) n += (size_t)n_samples[g0 + k];
            if (grow(e, o, (void **)&o->pcm, o->pcm_cap, std::max<size_t>(n, 1) * 2)) return -1;
            size_t at = 0;
            for (int k = 0; k < G; k++) {
                src[k] = o->pcm + at;
                if (n_samples[g0 + k] > 0) HIPCHK(hipMemcpyAsync(o->pcm + at, pcm[g0 + k], (size_t)n_samples[g0 + k] * 2, hipMemcpyHostToDevice, st));
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
                    HIPCHK(hipMemcpyAsync(o->pmel + (mel_off[b] + made[k]) * NMEL, o->mel_ring + (size_t)k * MEL_RING * NMEL,
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
    for (int b = 0; b < B; b++) mel_ptr[b] = o->pmel + mel_off[b] * NMEL;
    return 0;
}
}  // namespace nasr_eng

extern "C" int nasr_engine_transcribe_mel(nasr_engine *e, int B, const float *const *mel, const int32_t *n_frames,
                                          const int32_t *prompt_index, int32_t *const *tokens_out, const int32_t *tokens_cap,
                                          int32_t *n_tokens, int32_t *const *frames_out, uint32_t flags) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    if (B < 0) return fail("B < 0");
    if (B == 0) return 0;
    if (!mel || !n_frames) return fail("null mel / n_frames");
    for (int b = 0; b < B; b++)
        if (n_frames[b] < 0 || (n_frames[b] > 0 && !mel[b])) return fail("bad mel input for utterance %d", b);
    if (begin_call(e, B, prompt_index, n_tokens, flags, "nasr_engine_transcribe_mel")) return -1;
    return transcribe_core(e, B, mel, n_frames, false, prompt_index, tokens_out, tokens_cap, n_tokens, frames_out);
}

extern "C" int nasr_engine_transcribe(nasr_engine *e, int B, const int16_t *const *pcm, const int32_t *n_samples,
                                      const int32_t *prompt_index, int32_t *const *tokens_out, const int32_t *tokens_cap,
                                      int32_t *n_tokens, int32_t *const *frames_out, uint32_t flags) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    if (B < 0) return fail("B < 0");
    if (B == 0) return 0;
    if (!pcm || !n_samples) return fail("null pcm / n_samples");
    std::vector<int32_t> n_mel(B);
    for (int b = 0; b < B; b++) {
        if (n_samples[b] < 0 || (n_samples[b] > 0 && !pcm[b])) return fail("bad pcm input for utterance %d", b);
        n_mel[b] = nasr_plan::mel_frames(n_samples[b]);
    }
    // the limit is checked before any work (the plan rejects the same call again below, with the same message)
    std::vector<int> T;
    std::vector<nasr_plan::Batch> bt;
    int bad = -1;
    if (nasr_plan::plan_offline(n_mel.data(), B, e->opt_offline_rows, nasr_plan::OFFLINE_MAX_UTTS, T, bt, &bad))
        return fail("utterance %d: %d samples give %d encoder frames, more than NASR_OFFLINE_MAX_FRAMES = %d (the reference's max_pos_len, %.1f s); "
                    "transcribe longer audio with the streaming path (nemotron-asr-amd)", bad, bad >= 0 ? n_samples[bad] : -1,
                    bad >= 0 ? nasr_plan::enc_frames(n_mel[bad]) : -1, NASR_OFFLINE_MAX_FRAMES, nasr_plan::max_samples() / 16000.0);
    if (begin_call(e, B, prompt_index, n_tokens, flags, "nasr_engine_transcribe")) return -1;
    std::vector<const float *> mel;
    if (offline_mel(e, e->off, B, pcm, n_samples, (flags & NASR_FLAG_PCM_DEVICE) != 0, n_mel, mel)) return -1;
    return transcribe_core(e, B, mel.data(), n_mel.data(), true, prompt_index, tokens_out, tokens_cap, n_tokens, frames_out);
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
    const std::vector<float> &src = o->logprobs[u];
    if (!out) return (int)src.size();                       // size query
    const int n = std::min<int>((int)src.size(), std::max(cap, 0));
    memcpy(out, src.data(), (size_t)n * 4);
    return n;
}

extern "C" int nasr_engine_offline_frame_blank_logprobs(nasr_engine *e, int u, float *out, int32_t cap) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    if (!e->opt_frame_blank) return fail("no per-frame blank log-probabilities: engine option \"frame_blank_logprobs\" is off (set it to 1 before the first step or offline call)");
    OfflineState *o = e->off;
    if (!o || u < 0 || u >= (int)o->frame_blank_lps.size()) return fail("no offline blank log-probabilities of utterance %d (they are those of the last offline call)", u);
    const std::vector<float> &src = o->frame_blank_lps[u];
    if (!out) return (int)src.size();                       // size query
    const int n = std::min<int>((int)src.size(), std::max(cap, 0));
    memcpy(out, src.data(), (size_t)n * 4);
    return n;
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

// ---- forced alignment and transcript scoring on the RNN-T lattice ---------------------------------------------------------------------
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
    if (grow(e, o, (void **)&o->al_g, o->al_g_cap, (size_t)g_rows * JNT * 4) || grow(e, o, (void **)&o->al_lpb, o->al_lpb_cap, (size_t)cells * 4) ||
        grow(e, o, (void **)&o->al_lpt, o->al_lpt_cap, (size_t)cells * 4) || grow(e, o, (void **)&o->al_bp, o->al_bp_cap, (size_t)cells) ||
        grow(e, o, (void **)&o->al_tiles, o->al_tiles_cap, tiles.size() * sizeof(nasr_align::Tile)) || grow(e, o, (void **)&o->al_tok, o->al_tok_cap, ntok * 4) ||
        grow(e, o, (void **)&o->al_frames, o->al_frames_cap, ntok * 4) || grow(e, o, (void **)&o->al_tlp, o->al_tlp_cap, ntok * 4)) return -1;
    std::vector<RowDesc> rd(n);
    for (int k = 0; k < n; k++) { memset(&rd[k], 0, sizeof(RowDesc)); rd[k].slot = k; rd[k].prompt = -1; }
    // (the host vectors live until the stream is synchronised below)
    HIPCHK(hipMemcpyAsync(o->al_utt, ud.data(), (size_t)n * sizeof(nasr_align::Utt), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(o->al_tiles, tiles.data(), tiles.size() * sizeof(nasr_align::Tile), hipMemcpyHostToDevice, st));
    if (!tok.empty()) HIPCHK(hipMemcpyAsync(o->al_tok, tok.data(), tok.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(o->drows, rd.data(), (size_t)n * sizeof(RowDesc), hipMemcpyHostToDevice, st));
    // ---- g[u] of every utterance: the decode's own LSTM / joint.pred launches over the utterances that still have a position u --------
    launch_off_dec_reset(n, o->h, o->c, o->ctrl, st);
    DecParams dp;
    memset(&dp, 0, sizeof(dp));
    dp.rows = o->drows; dp.B = n; dp.T = 1; dp.ctrl = o->ctrl; dp.h = o->h; dp.c = o->c;
    bind_dec_weights(e, dp);
    dp.predg = o->predg; dp.n_active = o->n_active; dp.n_dirty = o->n_active + 1; dp.n_rows = o->n_active + 2; dp.dlist = o->dlist;
    AlignPredParams pp;
    memset(&pp, 0, sizeof(pp));
    pp.utt = o->al_utt; pp.n = n; pp.tok = o->al_tok; pp.ctrl = o->ctrl; pp.dlist = o->dlist; pp.n_dirty = dp.n_dirty; pp.predg = o->predg; pp.g = o->al_g;
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
    ap.utt = o->al_utt; ap.encproj = o->encproj; ap.g = o->al_g; ap.tok = o->al_tok; ap.out_w = dp.out_w; ap.out_b = dp.out_b;
    ap.lp_blank = o->al_lpb; ap.lp_token = o->al_lpt;
    for (size_t i = 0; i + 1 < lfirst.size(); i++) {
        const int cnt = lfirst[i + 1] - lfirst[i];
        double c = 0;
        for (int j = lfirst[i]; j < lfirst[i + 1]; j++) c += nasr_align::tile_cells(ud[tiles[j].utt].T, ud[tiles[j].utt].U, tiles[j].t0, tiles[j].u0);
        ProfScope ps(e, "k_align_lattice", (double)cnt * 1040 * JNT * 4, c * 2.0 * JNT * VOCAB);
        ap.tiles = o->al_tiles + lfirst[i];
        launch_align_lattice(ap, cnt, st);
    }
    // ---- forward and Viterbi recursions, backtrace ------------------------------------------------------------------------------------
    AlignRecParams rp;
    memset(&rp, 0, sizeof(rp));
    rp.utt = o->al_utt; rp.lp_blank = o->al_lpb; rp.lp_token = o->al_lpt; rp.bp = o->al_bp; rp.scores = o->al_scores; rp.frames = o->al_frames; rp.tok_lp = o->al_tlp;
    {
        ProfScope ps(e, "k_align_recursion", (double)cells * 9, 0);
        launch_align_recursion(rp, n, st);
    }
    std::vector<double> sc((size_t)n * 2);
    std::vector<int32_t> fr(tok.size());
    std::vector<float> lp(tok.size());
    HIPCHK(hipMemcpyAsync(sc.data(), o->al_scores, sc.size() * 8, hipMemcpyDeviceToHost, st));
    if (!tok.empty()) {
        HIPCHK(hipMemcpyAsync(fr.data(), o->al_frames, fr.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(lp.data(), o->al_tlp, lp.size() * 4, hipMemcpyDeviceToHost, st));
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
            HIPCHK(hipMemcpy(o->lat_b[b].data(), o->al_lpb + ud[k].cell0, nc * 4, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(o->lat_t[b].data(), o->al_lpt + ud[k].cell0, nc * 4, hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

static int align_core(nasr_engine *e, int B, const float *const *mel, const int32_t *n_frames, bool mel_device, const int32_t *prompt_index,
                      const int32_t *const *tokens, const int32_t *n_tokens, double *loglik_out, double *best_out, int32_t *const *frames_out,
                      float *const *token_logprobs_out) {
    OfflineState *o = e->off;
    for (int b = 0; b < B; b++) {
        const int U = n_tokens[b];
        if (U < 0 || U > NASR_ALIGN_MAX_TOKENS)
            return fail("utterance %d: a transcript of %d tokens, outside 0 .. NASR_ALIGN_MAX_TOKENS = %d", b, U, NASR_ALIGN_MAX_TOKENS);
        if (U > 0 && (!tokens || !tokens[b])) return fail("utterance %d: null transcript", b);
        for (int i = 0; i < U; i++)
            if (tokens[b][i] < 0 || tokens[b][i] >= BLANK)
                return fail("utterance %d: token %d of its transcript is %d; only ids 0 .. %d can be aligned (%d is blank)", b, i, tokens[b][i], BLANK - 1, BLANK);
    }
    std::vector<int> T;
    std::vector<nasr_plan::Batch> batches;
    int bad = -1;
    if (nasr_plan::plan_offline(n_frames, B, e->opt_offline_rows, nasr_plan::OFFLINE_MAX_UTTS, T, batches, &bad)) {
        if (bad >= 0 && n_frames[bad] >= 0)
            return fail("utterance %d: %d mel frames give %d encoder frames, more than NASR_OFFLINE_MAX_FRAMES = %d (the reference's max_pos_len)",
                        bad, n_frames[bad], nasr_plan::enc_frames(n_frames[bad]), NASR_OFFLINE_MAX_FRAMES);
        return fail("offline plan rejected the call");
    }
    if (ensure_offline_pos(e, o)) return -1;
    if (begin_taps(e, o, B, mel, n_frames, mel_device)) return -1;
    if (e->debug) { o->lat_b.assign(B, {}); o->lat_t.assign(B, {}); }
    AlignOut out;
    out.loglik.assign(B, 0.0); out.best.assign(B, 0.0); out.frames.assign(B, {}); out.lps.assign(B, {});
    for (const auto &bt : batches) {
        OffBatch ob;
        if (run_offline_encoder(e, o, mel, n_frames, prompt_index, T, bt.first, bt.count, ob)) return -1;
        if (align_batch(e, o, ob, tokens, n_tokens, out)) return -1;
        if (e->debug && ob.M > 0 && fetch_offline_taps(e, o, ob)) return -1;
    }
    o->lat_valid = e->debug;
    for (int b = 0; b < B; b++) {
        if (loglik_out) loglik_out[b] = out.loglik[b];
        if (best_out) best_out[b] = out.best[b];
        if (frames_out && frames_out[b]) memcpy(frames_out[b], out.frames[b].data(), out.frames[b].size() * 4);
        if (token_logprobs_out && token_logprobs_out[b]) memcpy(token_logprobs_out[b], out.lps[b].data(), out.lps[b].size() * 4);
    }
    return 0;
}
}  // namespace nasr_eng

extern "C" int nasr_engine_align_mel(nasr_engine *e, int B, const float *const *mel, const int32_t *n_frames, const int32_t *prompt_index,
                                     const int32_t *const *tokens, const int32_t *n_tokens, double *loglik_out, double *best_out,
                                     int32_t *const *frames_out, float *const *token_logprobs_out, uint32_t flags) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    if (B < 0) return fail("B < 0");
    if (B == 0) return 0;
    if (!mel || !n_frames) return fail("null mel / n_frames");
    for (int b = 0; b < B; b++)
        if (n_frames[b] < 0 || (n_frames[b] > 0 && !mel[b])) return fail("bad mel input for utterance %d", b);
    if (begin_call(e, B, prompt_index, n_tokens, flags, "nasr_engine_align_mel")) return -1;
    return align_core(e, B, mel, n_frames, false, prompt_index, tokens, n_tokens, loglik_out, best_out, frames_out, token_logprobs_out);
}

extern "C" int nasr_engine_align(nasr_engine *e, int B, const int16_t *const *pcm, const int32_t *n_samples, const int32_t *prompt_index,
                                 const int32_t *const *tokens, const int32_t *n_tokens, double *loglik_out, double *best_out,
                                 int32_t *const *frames_out, float *const *token_logprobs_out, uint32_t flags) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    if (B < 0) return fail("B < 0");
    if (B == 0) return 0;
    if (!pcm || !n_samples) return fail("null pcm / n_samples");
    std::vector<int32_t> n_mel(B);
    for (int b = 0; b < B; b++) {
        if (n_samples[b] < 0 || (n_samples[b] > 0 && !pcm[b])) return fail("bad pcm input for utterance %d", b);
        n_mel[b] = nasr_plan::mel_frames(n_samples[b]);
    }
    if (begin_call(e, B, prompt_index, n_tokens, flags, "nasr_engine_align")) return -1;
    // the limit is checked before any work, as in nasr_engine_transcribe
    std::vector<int> T;
    std::vector<nasr_plan::Batch> bt;
    int bad = -1;
    if (nasr_plan::plan_offline(n_mel.data(), B, e->opt_offline_rows, nasr_plan::OFFLINE_MAX_UTTS, T, bt, &bad))
        return fail("utterance %d: %d samples give %d encoder frames, more than NASR_OFFLINE_MAX_FRAMES = %d (the reference's max_pos_len, %.1f s)",
                    bad, bad >= 0 ? n_samples[bad] : -1, bad >= 0 ? nasr_plan::enc_frames(n_mel[bad]) : -1, NASR_OFFLINE_MAX_FRAMES, nasr_plan::max_samples() / 16000.0);
    std::vector<const float *> mel;
    if (offline_mel(e, e->off, B, pcm, n_samples, (flags & NASR_FLAG_PCM_DEVICE) != 0, n_mel, mel)) return -1;
    return align_core(e, B, mel.data(), n_mel.data(), true, prompt_index, tokens, n_tokens, loglik_out, best_out, frames_out, token_logprobs_out);
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

// ---- frame-synchronous beam search: N-best transcripts with scores (rules: nasr_beam.h, kernels: kernels_beam.hip) -----------------------
namespace nasr_eng {
static int beam_buf(nasr_engine *e, OfflineState *o, OfflineState::BeamBuf &b, size_t bytes) { return grow(e, o, &b.p, b.cap, bytes); }

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
    if (beam_buf(e, o, o->bm_utt, n * sizeof(BeamUtt)) || beam_buf(e, o, o->bm_beam, n * sizeof(nasr_beam::Beam)) ||
        beam_buf(e, o, o->bm_nodes, (size_t)nodes * sizeof(nasr_beam::Node)) || beam_buf(e, o, o->bm_enc, rows * JNT * 4) ||
        beam_buf(e, o, o->bm_rows, rows * sizeof(RowDesc)) || beam_buf(e, o, o->bm_ctrl, slots * sizeof(DecCtrl)) ||
        beam_buf(e, o, o->bm_h, slots * 4 * HID * 4) || beam_buf(e, o, o->bm_c, slots * 4 * HID * 4) || beam_buf(e, o, o->bm_predg, slots * JNT * 4) ||
        beam_buf(e, o, o->bm_key, rows * 8) || beam_buf(e, o, o->bm_part, rows * nasr_lp::WG_PARTS * sizeof(nasr_lp::Part)) ||
        beam_buf(e, o, o->bm_alt, rows * nasr_lp::WG_PARTS * nasr_beam::KTOP * 8) || beam_buf(e, o, o->bm_cnt, 8 * 4) ||
        beam_buf(e, o, o->bm_dlist, rows * 4) || beam_buf(e, o, o->bm_rowmap, rows * 4) || beam_buf(e, o, o->bm_out_n, n * 4) ||
        beam_buf(e, o, o->bm_out_len, (size_t)n * nasr_beam::WMAX * 4) || beam_buf(e, o, o->bm_out_score, (size_t)n * nasr_beam::WMAX * 8) ||
        beam_buf(e, o, o->bm_out_tok, (size_t)outs * 4) || beam_buf(e, o, o->bm_out_frame, (size_t)outs * 4) || beam_buf(e, o, o->bm_out_lp, (size_t)outs * 4) ||
        (totals && beam_buf(e, o, o->bm_out_lm, (size_t)n * nasr_beam::WMAX * 8 * 3)) ||
        (boost && (beam_buf(e, o, o->bm_bstate, slots * 4) || beam_buf(e, o, o->bm_raw, rows * nasr_boost::COLS * 4) ||
                   beam_buf(e, o, o->bm_out_boost, (size_t)n * nasr_beam::WMAX * 8))))
        return -1;
    HIPCHK(hipMemcpyAsync(o->bm_utt.p, ud.data(), n * sizeof(BeamUtt), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(o->bm_rows.p, 0, rows * sizeof(RowDesc), st));
    HIPCHK(hipMemsetAsync(o->bm_key.p, 0, rows * 8, st));
    HIPCHK(hipMemsetAsync(o->bm_cnt.p, 0, 8 * 4, st));
    int *cnt = (int *)o->bm_cnt.p;
    BeamParams bp;
    memset(&bp, 0, sizeof(bp));
    bp.utt = (const BeamUtt *)o->bm_utt.p; bp.n = n; bp.W = W; bp.N = N; bp.S = S; bp.prune = 1;
    bp.beam = (nasr_beam::Beam *)o->bm_beam.p; bp.nodes = (nasr_beam::Node *)o->bm_nodes.p; bp.encproj = o->encproj; bp.enc = (float *)o->bm_enc.p;
    bp.rows = (RowDesc *)o->bm_rows.p; bp.ctrl = (DecCtrl *)o->bm_ctrl.p; bp.h = (float *)o->bm_h.p; bp.c = (float *)o->bm_c.p;
    bp.lp_part = (const nasr_lp::Part *)o->bm_part.p; bp.alt_key = (const unsigned long long *)o->bm_alt.p;
    bp.dlist = (int *)o->bm_dlist.p; bp.rowmap = (unsigned *)o->bm_rowmap.p; bp.err = cnt + 4;
    bp.out_n = (int32_t *)o->bm_out_n.p; bp.out_len = (int32_t *)o->bm_out_len.p; bp.out_score = (double *)o->bm_out_score.p;
    bp.out_tok = (int32_t *)o->bm_out_tok.p; bp.out_frame = (int32_t *)o->bm_out_frame.p; bp.out_lp = (float *)o->bm_out_lp.p;
    if (e->lm) {                                               // shallow fusion: the prune only where its proof holds (nasr_beam.h)
        bp.lm_on = 1; bp.lm = e->lm_view; bp.lm_weight = e->lm_weight; bp.lm_bonus = e->lm_bonus;
        bp.prune = nasr_beam::prune_allowed(e->lm_bonus, e->lm->all_nonpositive) ? 1 : 0;
    }
    if (totals) { bp.out_lm = (double *)o->bm_out_lm.p; bp.out_lm_final = bp.out_lm + (size_t)n * nasr_beam::WMAX; bp.out_total = bp.out_lm_final + (size_t)n * nasr_beam::WMAX; }
    if (boost) {                                               // a non-empty set pays positive bonuses: unpruned (nasr_beam.h)
        bp.boost_on = 1; bp.boost_bonus = e->boost_bonus; bp.boost_next = e->boost_next; bp.boost_state = (int *)o->bm_bstate.p;
        bp.raw_logits = (const float *)o->bm_raw.p; bp.out_boost = (double *)o->bm_out_boost.p;
        bp.prune = nasr_beam::prune_allowed(e->lm ? e->lm_bonus : 0.0f, e->lm ? e->lm->all_nonpositive != 0 : true, e->boost_states) ? 1 : 0;
    }
    DecParams dp;
    memset(&dp, 0, sizeof(dp));
    dp.rows = bp.rows; dp.B = (int)rows; dp.T = 1; dp.ctrl = bp.ctrl; dp.h = bp.h; dp.c = bp.c; dp.encproj = bp.enc;
    bind_dec_weights(e, dp);
    dp.predg = (float *)o->bm_predg.p; dp.key = (unsigned long long *)o->bm_key.p; dp.n_active = cnt + 5;
    dp.dlist = bp.dlist; dp.rowmap = bp.rowmap; dp.lp_part = (nasr_lp::Part *)o->bm_part.p; dp.alt_key = (unsigned long long *)o->bm_alt.p; dp.alt_k = nasr_beam::KTOP;
    if (boost) { dp.boost_bonus = bp.boost_bonus; dp.boost_next = bp.boost_next; dp.boost_state = bp.boost_state; dp.raw_logits = (float *)o->bm_raw.p; }
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

static int beam_core(nasr_engine *e, int B, const float *const *mel, const int32_t *n_frames, bool mel_device, const int32_t *prompt_index,
                     int W, int N, int S, int32_t *n_hyps, bool boost) {
    OfflineState *o = e->off;
    std::vector<int> T;
    std::vector<nasr_plan::Batch> batches;
    int bad = -1;
    if (nasr_plan::plan_offline(n_frames, B, e->opt_offline_rows, nasr_plan::OFFLINE_MAX_UTTS, T, batches, &bad)) {
        if (bad >= 0 && n_frames[bad] >= 0)
            return fail("utterance %d: %d mel frames give %d encoder frames, more than NASR_OFFLINE_MAX_FRAMES = %d (the reference's max_pos_len)",
                        bad, n_frames[bad], nasr_plan::enc_frames(n_frames[bad]), NASR_OFFLINE_MAX_FRAMES);
        return fail("offline plan rejected the call");
    }
    if (ensure_offline_pos(e, o)) return -1;
    if (begin_taps(e, o, B, mel, n_frames, mel_device)) return -1;
    o->beam_res.assign(B, {});
    o->beam_lm = e->lm != nullptr; o->beam_lm_generation = e->lm_generation;
    o->beam_boost = boost;
    for (const auto &bt : batches) {
        OffBatch ob;
        if (run_offline_encoder(e, o, mel, n_frames, prompt_index, T, bt.first, bt.count, ob)) { o->beam_res.clear(); return -1; }
        if (beam_batch(e, o, ob, W, N, S)) { o->beam_res.clear(); return -1; }
        if (e->debug && ob.M > 0 && fetch_offline_taps(e, o, ob)) { o->beam_res.clear(); return -1; }
    }
    o->beam_valid = true;
    for (int b = 0; b < B; b++) n_hyps[b] = (int32_t)o->beam_res[b].size();
    return 0;
}
}  // namespace nasr_eng

extern "C" int nasr_engine_transcribe_beam_mel(nasr_engine *e, int B, const float *const *mel, const int32_t *n_frames, const int32_t *prompt_index,
                                               const nasr_beam_params *params, int32_t *n_hyps, uint32_t flags) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    if (B < 0) return fail("B < 0");
    int W, N, S;
    beam_forget(e);
    if (beam_check_params(params, &W, &N, &S) || beam_check_flags(e, flags)) return -1;
    if (B == 0) return 0;
    if (!mel || !n_frames) return fail("null mel / n_frames");
    for (int b = 0; b < B; b++)
        if (n_frames[b] < 0 || (n_frames[b] > 0 && !mel[b])) return fail("bad mel input for utterance %d", b);
    if (begin_call(e, B, prompt_index, n_hyps, flags, "nasr_engine_transcribe_beam_mel")) return -1;
    return beam_core(e, B, mel, n_frames, false, prompt_index, W, N, S, n_hyps, (flags & NASR_FLAG_BEAM_BOOST) != 0);
}

extern "C" int nasr_engine_transcribe_beam(nasr_engine *e, int B, const int16_t *const *pcm, const int32_t *n_samples, const int32_t *prompt_index,
                                           const nasr_beam_params *params, int32_t *n_hyps, uint32_t flags) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    if (B < 0) return fail("B < 0");
    int W, N, S;
    beam_forget(e);
    if (beam_check_params(params, &W, &N, &S) || beam_check_flags(e, flags)) return -1;
    if (B == 0) return 0;
    if (!pcm || !n_samples) return fail("null pcm / n_samples");
    std::vector<int32_t> n_mel(B);
    for (int b = 0; b < B; b++) {
        if (n_samples[b] < 0 || (n_samples[b] > 0 && !pcm[b])) return fail("bad pcm input for utterance %d", b);
        n_mel[b] = nasr_plan::mel_frames(n_samples[b]);
    }
    if (begin_call(e, B, prompt_index, n_hyps, flags, "nasr_engine_transcribe_beam")) return -1;
    // the limit is checked before any work, as in nasr_engine_transcribe
    std::vector<int> T;
    std::vector<nasr_plan::Batch> bt;
    int bad = -1;
    if (nasr_plan::plan_offline(n_mel.data(), B, e->opt_offline_rows, nasr_plan::OFFLINE_MAX_UTTS, T, bt, &bad))
        return fail("utterance %d: %d samples give %d encoder frames, more than NASR_OFFLINE_MAX_FRAMES = %d (the reference's max_pos_len, %.1f s)",
                    bad, bad >= 0 ? n_samples[bad] : -1, bad >= 0 ? nasr_plan::enc_frames(n_mel[bad]) : -1, NASR_OFFLINE_MAX_FRAMES, nasr_plan::max_samples() / 16000.0);
    std::vector<const float *> mel;
    if (offline_mel(e, e->off, B, pcm, n_samples, (flags & NASR_FLAG_PCM_DEVICE) != 0, n_mel, mel)) return -1;
    return beam_core(e, B, mel.data(), n_mel.data(), true, prompt_index, W, N, S, n_hyps, (flags & NASR_FLAG_BEAM_BOOST) != 0);
}

extern "C" int nasr_engine_beam_hypothesis(nasr_engine *e, int u, int rank, int32_t *tokens_out, int32_t *frames_out, float *token_logprobs_out,
                                           int32_t cap, double *score_out) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    OfflineState *o = e->off;
    if (!o || !o->beam_valid || u < 0 || u >= (int)o->beam_res.size())
        return fail("no beam hypotheses of utterance %d (they are those of the last offline call, which must be a beam call)", u);
    if (rank < 0 || rank >= (int)o->beam_res[u].size()) return fail("utterance %d has %d hypotheses, no rank %d", u, (int)o->beam_res[u].size(), rank);
    const OfflineState::BeamHyp &h = o->beam_res[u][rank];
    const int n = std::min<int>((int)h.tokens.size(), std::max(cap, 0));
    if (tokens_out) memcpy(tokens_out, h.tokens.data(), (size_t)n * 4);
    if (frames_out) memcpy(frames_out, h.frames.data(), (size_t)n * 4);
    if (token_logprobs_out) memcpy(token_logprobs_out, h.lps.data(), (size_t)n * 4);
    if (score_out) *score_out = h.score;
    return (int)h.tokens.size();
}

// the language-model side of a hypothesis of the last beam call, which must have run with an LM attached: lm_final (the EOS term included
// when the model has one) and the final key, both as the device computed them; the per-token values are recomputed here by the same
// nasr_lm::lookup over the returned tokens (the trie node does not carry them)
extern "C" int nasr_engine_beam_hypothesis_lm(nasr_engine *e, int u, int rank, double *lm_logprob_out, double *total_out, float *token_lm_logprobs_out,
                                              int32_t cap) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    OfflineState *o = e->off;
    if (!o || !o->beam_valid || u < 0 || u >= (int)o->beam_res.size())
        return fail("no beam hypotheses of utterance %d (they are those of the last offline call, which must be a beam call)", u);
    if (!o->beam_lm || !e->lm) return fail("the last beam call ran without a language model (nasr_engine_set_lm)");
    if (o->beam_lm_generation != e->lm_generation)
        return fail("the language model was replaced after the last beam call (nasr_engine_set_lm): its hypotheses have no LM read-out any more");
    if (rank < 0 || rank >= (int)o->beam_res[u].size()) return fail("utterance %d has %d hypotheses, no rank %d", u, (int)o->beam_res[u].size(), rank);
    const OfflineState::BeamHyp &h = o->beam_res[u][rank];
    if (lm_logprob_out) *lm_logprob_out = h.lm_final;
    if (total_out) *total_out = h.total;
    const int n = std::min<int>((int)h.tokens.size(), std::max(cap, 0));
    if (token_lm_logprobs_out) {
        const nasr_lm::View v = e->lm->view();
        int32_t state = v.start;
        for (int i = 0; i < n; i++) token_lm_logprobs_out[i] = (float)nasr_lm::lookup(v, state, h.tokens[(size_t)i], &state);
    }
    return (int)h.tokens.size();
}

// the boost side of a hypothesis of the last beam call, which must have been boosted (NASR_FLAG_BEAM_BOOST): the sum of its tokens' bonuses and the
// ranking key, both as the device computed them; the per-token bonuses were fixed when the call fetched its results, from the set it ran with
extern "C" int nasr_engine_beam_hypothesis_boost(nasr_engine *e, int u, int rank, double *boost_out, double *total_out, float *token_bonus_out, int32_t cap) {
    ApiGuard api_guard;
    if (!e) return fail("null engine");
    OfflineState *o = e->off;
    if (!o || !o->beam_valid || u < 0 || u >= (int)o->beam_res.size())
        return fail("no beam hypotheses of utterance %d (they are those of the last offline call, which must be a beam call)", u);
    if (!o->beam_boost) return fail("the last beam call ran without phrase boosting (NASR_FLAG_BEAM_BOOST)");
    if (rank < 0 || rank >= (int)o->beam_res[u].size()) return fail("utterance %d has %d hypotheses, no rank %d", u, (int)o->beam_res[u].size(), rank);
    const OfflineState::BeamHyp &h = o->beam_res[u][rank];
    if (boost_out) *boost_out = h.boost;
    if (total_out) *total_out = h.total;
    const int n = std::min<int>((int)h.tokens.size(), std::max(cap, 0));
    if (token_bonus_out) memcpy(token_bonus_out, h.bonuses.data(), (size_t)n * 4);
    return (int)h.tokens.size();
}
