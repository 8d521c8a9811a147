// nemo_amd.cpp -- see nemo_amd.h
#include "nemo_amd.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "boost_phrases.h"
#include "gguf_reader.h"
#include "lm_arpa.h"
#include "nemotron_asr_amd.h"
#include "stream_envelope.h"

using nasr_host::GgufFile;
using nasr_host::GgufValue;

std::string tokens_to_text(const std::vector<int> &tokens, const std::vector<std::string> &vocab) {
    std::string out;
    for (int id : tokens) {
        if (id < 0 || id >= (int)vocab.size()) continue;
        const std::string &piece = vocab[(size_t)id];
        if (piece.compare(0, 3, "\xe2\x96\x81") == 0) {   // U+2581
            out += ' ';
            out.append(piece, 3, std::string::npos);
        } else {
            out += piece;
        }
    }
    return out;
}

std::string tokens_to_text(const std::vector<timed_token> &tokens, const std::vector<std::string> &vocab, bool timestamp_words) {
    std::string out;
    for (const timed_token &t : tokens) {
        if (t.token_id < 0 || t.token_id >= (int)vocab.size()) continue;
        const std::string &piece = vocab[(size_t)t.token_id];
        if (piece.compare(0, 3, "\xe2\x96\x81") == 0) {
            out += ' ';
            if (timestamp_words) {
                char stamp[32];
                snprintf(stamp, sizeof(stamp), "{%.2f}", t.to_seconds());
                out += stamp;
            }
            out.append(piece, 3, std::string::npos);
        } else {
            out += piece;
        }
    }
    return out;
}

std::vector<timed_token> nemo_stream_get_timed_tokens(nemo_stream_context *sctx) {
    std::vector<timed_token> out;
    if (!sctx) return out;
    const size_t n = sctx->tokens.size();
    std::vector<int32_t> frames(n ? n : 1);
    const size_t first = n > 4096 ? n - 4096 : 0;       // older frames have left the device ring
    const int got = nasr_stream_get_token_frames(sctx->stream, (int64_t)first, (int32_t)(n - first), frames.data());
    if (got < 0) { fprintf(stderr, "%s: %s\n", __func__, nasr_last_error()); return out; }
    for (size_t i = 0; i < first; i++) out.emplace_back(sctx->tokens[i], -1);
    for (int i = 0; i < got; i++) out.emplace_back(sctx->tokens[first + (size_t)i], frames[(size_t)i]);
    return out;
}

std::vector<float> nemo_stream_get_token_logprobs(nemo_stream_context *sctx) {
    std::vector<float> out;
    if (!sctx) return out;
    const size_t n = sctx->tokens.size();
    std::vector<float> lp(n ? n : 1);
    const size_t first = n > 4096 ? n - 4096 : 0;       // older values have left the device ring
    const int got = nasr_stream_get_token_logprobs(sctx->stream, (int64_t)first, (int32_t)(n - first), lp.data());
    if (got < 0) { fprintf(stderr, "%s: %s\n", __func__, nasr_last_error()); return out; }
    out.assign(first, NAN);
    out.insert(out.end(), lp.begin(), lp.begin() + got);
    return out;
}

std::vector<float> nemo_stream_get_token_entropies(nemo_stream_context *sctx) {
    std::vector<float> out;
    if (!sctx) return out;
    const size_t n = sctx->tokens.size();
    std::vector<float> h(n ? n : 1);
    const size_t first = n > 4096 ? n - 4096 : 0;       // older values have left the device ring
    const int got = nasr_stream_get_token_entropies(sctx->stream, (int64_t)first, (int32_t)(n - first), h.data());
    if (got < 0) { fprintf(stderr, "%s: %s\n", __func__, nasr_last_error()); return out; }
    out.assign(first, NAN);
    out.insert(out.end(), h.begin(), h.begin() + got);
    return out;
}

std::vector<float> nemo_stream_get_frame_blank_logprobs(nemo_stream_context *sctx) {
    std::vector<float> out;
    if (!sctx) return out;
    const int n = nasr_stream_get_frame_blank_logprobs(sctx->stream, 0, 0, nullptr);      // frames decoded so far
    if (n < 0) { fprintf(stderr, "%s: %s\n", __func__, nasr_last_error()); return out; }
    const int first = n > 4096 ? n - 4096 : 0;          // older values have left the device ring
    std::vector<float> lp((size_t)(n - first) + 1);
    const int got = nasr_stream_get_frame_blank_logprobs(sctx->stream, first, n - first, lp.data());
    if (got < 0) { fprintf(stderr, "%s: %s\n", __func__, nasr_last_error()); return out; }
    out.assign((size_t)first, NAN);
    out.insert(out.end(), lp.begin(), lp.begin() + got);
    return out;
}

bool nemo_stream_set_endpointing(nemo_stream_context *sctx, const nasr_endpoint::Config *cfg) {
    if (!sctx) return false;
    const int n = nasr_stream_get_frame_blank_logprobs(sctx->stream, 0, 0, nullptr);      // fails when the option is off
    nasr_stream_stats stats;
    if (n < 0 || nasr_stream_get_stats(sctx->stream, &stats) < 0) { fprintf(stderr, "%s: %s\n", __func__, nasr_last_error()); return false; }
    sctx->ep_on = true;
    sctx->ep_cfg = cfg ? *cfg : nasr_endpoint::Config();
    sctx->ep_state = nasr_endpoint::State();
    sctx->ep_state.utt_start = n;
    sctx->ep_frames = n;
    sctx->ep_tokens = stats.tokens;
    sctx->ep_events.clear();
    return true;
}

const std::vector<nasr_endpoint::Event> &nemo_stream_get_endpoints(nemo_stream_context *sctx) {
    static const std::vector<nasr_endpoint::Event> empty;
    if (!sctx || !sctx->ep_on) return empty;
    const int n = nasr_stream_get_frame_blank_logprobs(sctx->stream, 0, 0, nullptr);
    nasr_stream_stats stats;
    if (n < 0 || nasr_stream_get_stats(sctx->stream, &stats) < 0) { fprintf(stderr, "%s: %s\n", __func__, nasr_last_error()); return sctx->ep_events; }
    if (n <= sctx->ep_frames) return sctx->ep_events;
    // the new frames' values (those that have left the ring: NaN, not silent) and the frames of the device's new tokens, in token order
    const int64_t first = std::max<int64_t>(sctx->ep_frames, (int64_t)n - 4096);
    std::vector<float> lp((size_t)(n - first));
    if (nasr_stream_get_frame_blank_logprobs(sctx->stream, first, (int32_t)(n - first), lp.data()) != n - first) { fprintf(stderr, "%s: %s\n", __func__, nasr_last_error()); return sctx->ep_events; }
    const int64_t tok_first = std::max<int64_t>(sctx->ep_tokens, (int64_t)stats.tokens - 4096);
    std::vector<int32_t> tf((size_t)(stats.tokens - tok_first) + 1);
    const int got = nasr_stream_get_token_frames(sctx->stream, tok_first, (int32_t)(stats.tokens - tok_first), tf.data());
    if (got < 0) { fprintf(stderr, "%s: %s\n", __func__, nasr_last_error()); return sctx->ep_events; }
    size_t ti = 0;
    int carried = (int)(tok_first - sctx->ep_tokens);      // tokens whose frames have left the ring: counted on the first new frame
    for (int64_t f = sctx->ep_frames; f < n; f++) {
        int on_frame = carried;
        carried = 0;
        while (ti < (size_t)got && tf[ti] <= f) { on_frame++; ti++; }
        nasr_endpoint::Event ev;
        if (nasr_endpoint::advance(sctx->ep_state, sctx->ep_cfg, f, f >= first ? lp[(size_t)(f - first)] : NAN, on_frame, &ev)) sctx->ep_events.push_back(ev);
    }
    sctx->ep_frames = n;
    sctx->ep_tokens = stats.tokens;
    return sctx->ep_events;
}

nemo_token_alternatives nemo_stream_get_token_alternatives(nemo_stream_context *sctx) {
    nemo_token_alternatives out;
    if (!sctx || !sctx->nctx || sctx->nctx->token_alternatives <= 0) return out;
    const int k = sctx->nctx->token_alternatives;
    const size_t n = sctx->tokens.size();
    const size_t first = n > 4096 ? n - 4096 : 0;       // older values have left the device ring
    std::vector<int32_t> ids((n - first) * k + 1);
    std::vector<float> lp((n - first) * k + 1);
    const int got = nasr_stream_get_token_alternatives(sctx->stream, (int64_t)first, (int32_t)(n - first), ids.data(), lp.data());
    if (got < 0) { fprintf(stderr, "%s: %s\n", __func__, nasr_last_error()); return out; }
    out.k = k;
    out.n_tokens = first + (size_t)got;
    out.ids.assign(first * k, -1);
    out.logprobs.assign(first * k, NAN);
    out.ids.insert(out.ids.end(), ids.begin(), ids.begin() + (size_t)got * k);
    out.logprobs.insert(out.logprobs.end(), lp.begin(), lp.begin() + (size_t)got * k);
    return out;
}

nemo_context *nemo_init_with_device(const char *model_path, int device, int dtype, int max_streams) {
    return nemo_init_with_rows(model_path, device, dtype, max_streams, 0);
}
nemo_context *nemo_init_with_rows(const char *model_path, int device, int dtype, int max_streams, int workspace_rows) {
    if (!model_path) return nullptr;
    GgufFile g;
    std::string err;
    if (!g.open(model_path, err)) {
        fprintf(stderr, "%s: failed to open GGUF file: %s\n", __func__, err.c_str());
        return nullptr;
    }
    nemo_context *ctx = new nemo_context();
    nemo_hparams &hp = ctx->hparams;
    uint32_t v;
    // nemo.* keys (reference src/nemo-ggml.cpp:108-142); absent keys keep their defaults
    if (g.get_u32("nemo.n_mels", v)) hp.n_mels = (int32_t)v;
    if (g.get_u32("nemo.d_model", v)) hp.d_model = (int32_t)v;
    if (g.get_u32("nemo.n_heads", v)) hp.n_heads = (int32_t)v;
    if (g.get_u32("nemo.d_head", v)) hp.d_head = (int32_t)v;
    if (g.get_u32("nemo.d_ff", v)) hp.d_ff = (int32_t)v;
    if (g.get_u32("nemo.n_layers", v)) hp.n_layers = (int32_t)v;
    if (g.get_u32("nemo.vocab_size", v)) hp.vocab_size = (int32_t)v;
    if (g.get_u32("nemo.decoder_dim", v)) hp.decoder_dim = (int32_t)v;
    if (g.get_u32("nemo.joint_dim", v)) hp.joint_dim = (int32_t)v;
    if (g.get_u32("nemo.subsampling_factor", v)) hp.subsampling_factor = (int32_t)v;
    if (g.get_u32("nemo.att_left_context", v)) hp.att_left_context = (int32_t)v;
    if (g.get_u32("nemo.num_prompts", v)) hp.num_prompts = (int32_t)v;
    // vocabulary: string array preferred, legacy 8-byte-record blob otherwise (:149-169)
    if (const GgufValue *vl = g.find("tokenizer.vocab_list"); vl && vl->type == 9) {
        ctx->vocab = vl->arr_s;
    } else if (const GgufValue *vb = g.find("tokenizer.vocab"); vb && vb->type == 8) {
        const size_t n = (size_t)hp.vocab_size - 1;
        for (size_t i = 0; i < n && (i + 1) * 8 <= vb->s.size(); i++) {
            const char *rec = vb->s.data() + i * 8;
            ctx->vocab.emplace_back(rec, strnlen(rec, 8));
        }
    } else {
        fprintf(stderr, "%s: no vocabulary in GGUF (need tokenizer.vocab_list or tokenizer.vocab)\n", __func__);
        delete ctx;
        return nullptr;
    }
    // language prompt dictionary (:171-182)
    const GgufValue *pl = g.find("nemo.prompt_langs"), *pi = g.find("nemo.prompt_ids");
    if (pl && pi && pl->arr_s.size() == pi->arr_i.size())
        for (size_t i = 0; i < pl->arr_s.size(); i++) ctx->prompt_dict[pl->arr_s[i]] = (int)pi->arr_i[i];
    if (hp.num_prompts > 0) ctx->prompt_index = 101;   // "auto" (:459-462)
    // kernel size from the depthwise conv weight, stored (k, C) -> ne[1] = k (:357-360)
    if (const nasr_host::GgufTensor *dw = g.tensor("encoder.layers.0.conv.depthwise_conv.weight")) hp.kernel_size = (int32_t)dw->ne[1];

    std::vector<nasr_weight_desc> descs;
    descs.reserve(g.tensors().size());
    for (const auto &t : g.tensors()) {
        nasr_weight_desc d;
        d.name = t.name.c_str();
        d.type = t.type;
        d.n_dims = t.n_dims;
        for (int i = 0; i < 4; i++) d.ne[i] = t.ne[i];
        d.data = t.data;
        descs.push_back(d);
    }
    nasr_hparams nh;
    nh.n_mels = hp.n_mels; nh.d_model = hp.d_model; nh.n_heads = hp.n_heads; nh.d_head = hp.d_head; nh.d_ff = hp.d_ff;
    nh.n_layers = hp.n_layers; nh.vocab_size = hp.vocab_size; nh.decoder_dim = hp.decoder_dim; nh.joint_dim = hp.joint_dim;
    nh.subsampling_factor = hp.subsampling_factor; nh.att_left_context = hp.att_left_context; nh.kernel_size = hp.kernel_size;
    nh.num_prompts = hp.num_prompts;
    if (nasr_engine_create_ex(&ctx->engine, device, dtype, &nh, descs.data(), (int)descs.size(), max_streams, workspace_rows) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        delete ctx;
        return nullptr;
    }
    ctx->max_streams = max_streams;
    ctx->workspace_rows = std::max(std::max(max_streams * 14, 256), workspace_rows);
    return ctx;
}

nemo_context *nemo_init(const char *model_path) { return nemo_init_with_device(model_path, 0, NASR_DTYPE_BF16, 64); }

bool nemo_set_token_logprobs(nemo_context *ctx, bool on) {
    if (!ctx || !ctx->engine) return false;
    if (nasr_engine_set_option(ctx->engine, "token_logprobs", on ? 1 : 0) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    ctx->token_logprobs = on;
    return true;
}

bool nemo_set_token_entropy(nemo_context *ctx, float alpha) {
    if (!ctx || !ctx->engine) return false;
    const int milli = alpha >= 0.0f && alpha < 1e4f ? (int)std::lround((double)alpha * 1000.0) : -1;      // anything else: a value the engine refuses, with its message
    if (nasr_engine_set_option(ctx->engine, "token_entropy", milli) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    ctx->token_entropy_milli = milli;
    return true;
}

bool nemo_set_frame_blank_logprobs(nemo_context *ctx, bool on) {
    if (!ctx || !ctx->engine) return false;
    if (nasr_engine_set_option(ctx->engine, "frame_blank_logprobs", on ? 1 : 0) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    return true;
}

bool nemo_set_phrase_boost(nemo_context *ctx, int max_states) {
    if (!ctx || !ctx->engine) return false;
    if (nasr_engine_set_option(ctx->engine, "phrase_boost", max_states) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    return true;
}

static bool apply_boost_phrases(nemo_context *ctx, const boost_phrases::Result &r, const char *who) {
    for (const std::string &p : r.problems) fprintf(stderr, "%s: skipped, %s\n", who, p.c_str());
    std::vector<const int32_t *> tok;
    std::vector<int32_t> len;
    std::vector<float> bonus;
    for (const boost_phrases::Phrase &p : r.phrases) { tok.push_back(p.tokens.data()); len.push_back((int32_t)p.tokens.size()); bonus.push_back(p.bonus); }
    if (nasr_engine_set_boost_phrases(ctx->engine, (int)tok.size(), tok.data(), len.data(), bonus.data()) < 0) {
        fprintf(stderr, "%s: %s\n", who, nasr_last_error());
        return false;
    }
    return true;
}

bool nemo_set_boost_phrases(nemo_context *ctx, const std::vector<std::string> &phrases, const std::vector<float> &bonus, float default_bonus) {
    if (!ctx || !ctx->engine) return false;
    return apply_boost_phrases(ctx, boost_phrases::from_list(phrases, bonus, ctx->vocab, default_bonus), __func__);
}

bool nemo_load_boost_file(nemo_context *ctx, const char *path, float default_bonus) {
    if (!ctx || !ctx->engine || !path) return false;
    boost_phrases::Result r;
    if (!boost_phrases::parse_file(path, ctx->vocab, default_bonus, r)) {
        fprintf(stderr, "%s: cannot read '%s'\n", __func__, path);
        return false;
    }
    return apply_boost_phrases(ctx, r, __func__);
}

bool nemo_load_lm_arpa(nemo_context *ctx, const char *path, float weight, float token_bonus, float unk_logprob) {
    if (!ctx || !ctx->engine || !path) return false;
    lm_arpa::Model m;
    const std::string err = lm_arpa::parse_file(path, ctx->vocab, m);
    if (!err.empty()) { fprintf(stderr, "%s: %s: %s\n", __func__, path, err.c_str()); return false; }
    if (!m.has_unk && std::isnan(unk_logprob)) {
        fprintf(stderr, "%s: %s has no <unk> unigram: give unk_logprob\n", __func__, path);
        return false;
    }
    if (m.skipped_unk) fprintf(stderr, "%s: %lld n-grams with <unk> inside were skipped\n", __func__, m.skipped_unk);
    nasr_lm_desc d;
    memset(&d, 0, sizeof(d));
    d.order = m.order; d.n_ngrams = (int64_t)m.lengths.size();
    d.lengths = m.lengths.data(); d.tokens = m.tokens.data(); d.logprob = m.logprob.data(); d.backoff = m.backoff.data();
    d.unk_logprob = std::isnan(unk_logprob) ? m.unk_logprob : unk_logprob; d.weight = weight; d.token_bonus = token_bonus;
    if (nasr_engine_set_lm(ctx->engine, &d) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    ctx->lm_attached = true;
    return true;
}

bool nemo_clear_lm(nemo_context *ctx) {
    if (!ctx || !ctx->engine) return false;
    if (nasr_engine_set_lm(ctx->engine, nullptr) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    ctx->lm_attached = false;
    return true;
}

bool nemo_set_lm_fusion(nemo_context *ctx, bool enable) {
    if (!ctx || !ctx->engine) return false;
    if (nasr_engine_set_option(ctx->engine, "lm_fusion", enable ? 1 : 0) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    return true;
}

bool nemo_set_greedy_lm_weights(nemo_context *ctx, float weight, float token_bonus) {
    if (!ctx || !ctx->engine) return false;
    if (nasr_engine_set_greedy_lm_weights(ctx->engine, weight, token_bonus) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    return true;
}

bool nemo_set_beam_boost(nemo_context *ctx, bool enable) {
    if (!ctx || !ctx->engine) return false;
    int64_t cap = 0;
    if (enable && (nasr_engine_get_counter(ctx->engine, "boost_states", &cap) < 0 || cap == 0)) {
        fprintf(stderr, "%s: phrase boosting is off (nemo_set_phrase_boost)\n", __func__);
        return false;
    }
    ctx->beam_boost = enable;
    return true;
}

bool nemo_stream_set_boost(nemo_stream_context *sctx, bool enable) {
    if (!sctx || !sctx->stream) return false;
    if (nasr_stream_set_boost(sctx->stream, enable ? 1 : 0) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    return true;
}

bool nemo_set_token_alternatives(nemo_context *ctx, int k) {
    if (!ctx || !ctx->engine) return false;
    if (nasr_engine_set_option(ctx->engine, "token_alternatives", k) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    ctx->token_alternatives = k;
    return true;
}

bool nemo_set_pipeline(nemo_context *ctx, int depth) {
    if (!ctx || !ctx->engine) return false;
    if (nasr_engine_set_option(ctx->engine, "pipeline", depth) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    return true;
}

void nemo_free(nemo_context *ctx) {
    if (!ctx) return;
    nasr_engine_destroy(ctx->engine);
    delete ctx;
}

static bool lookup_lang(nemo_context *ctx, const char *lang, const char *who, int &idx) {
    if (ctx->hparams.num_prompts <= 0) {
        fprintf(stderr, "%s: model is not multilingual (num_prompts=0)\n", who);
        return false;
    }
    auto it = ctx->prompt_dict.find(lang);
    if (it == ctx->prompt_dict.end()) {
        fprintf(stderr, "%s: unknown language code '%s'\n", who, lang);
        return false;
    }
    idx = it->second;
    return true;
}

nemo_alignment nemo_align_audio(nemo_context *ctx, const int16_t *audio, int n_samples, const std::vector<int32_t> &tokens) {
    nemo_alignment out;
    if (!ctx || !ctx->engine || n_samples < 0 || (n_samples > 0 && !audio)) return out;
    out.frames.assign(tokens.size(), -1);
    out.logprobs.assign(tokens.size(), NAN);
    const int32_t n_tok = (int32_t)tokens.size(), prompt = ctx->prompt_index;
    const int32_t *tp = tokens.data();
    int32_t *fp = out.frames.data();
    float *lp = out.logprobs.data();
    if (nasr_engine_align(ctx->engine, 1, &audio, &n_samples, ctx->hparams.num_prompts > 0 ? &prompt : nullptr, &tp, &n_tok, &out.loglik, &out.best,
                          &fp, &lp, 0) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return out;
    }
    out.ok = true;
    return out;
}

// the hypotheses of utterance 0 of the beam call that has just returned n_hyps (an offline call or a second pass), with the LM and boost sides
// where the context has them; empty on failure
static std::vector<nemo_hypothesis> read_beam_hypotheses(nemo_context *ctx, int n_hyps, const char *who) {
    std::vector<nemo_hypothesis> out;
    for (int r = 0; r < n_hyps; r++) {
        nemo_hypothesis h;
        const int n = nasr_engine_beam_hypothesis(ctx->engine, 0, r, nullptr, nullptr, nullptr, 0, nullptr);
        if (n < 0) { fprintf(stderr, "%s: %s\n", who, nasr_last_error()); out.clear(); return out; }
        h.tokens.assign((size_t)n, 0); h.frames.assign((size_t)n, 0); h.logprobs.assign((size_t)n, 0.0f);
        nasr_engine_beam_hypothesis(ctx->engine, 0, r, h.tokens.data(), h.frames.data(), h.logprobs.data(), n, &h.score);
        if (ctx->lm_attached) {
            if (nasr_engine_beam_hypothesis_lm(ctx->engine, 0, r, &h.lm_logprob, &h.total, nullptr, 0) < 0) {
                fprintf(stderr, "%s: %s\n", who, nasr_last_error());
                out.clear();
                return out;
            }
            h.has_lm = true;
        }
        if (ctx->beam_boost) {
            h.token_bonuses.assign((size_t)n, 0.0f);
            if (nasr_engine_beam_hypothesis_boost(ctx->engine, 0, r, &h.boost, &h.total, h.token_bonuses.data(), n) < 0) {
                fprintf(stderr, "%s: %s\n", who, nasr_last_error());
                out.clear();
                return out;
            }
            h.has_boost = true;
        }
        out.push_back(h);
    }
    return out;
}

std::vector<nemo_hypothesis> nemo_transcribe_beam(nemo_context *ctx, const int16_t *audio, int n_samples, int beam, int nbest, int max_symbols) {
    std::vector<nemo_hypothesis> out;
    if (!ctx || !ctx->engine || n_samples < 0 || (n_samples > 0 && !audio)) return out;
    const int32_t prompt = ctx->prompt_index;
    const int32_t *pp = ctx->hparams.num_prompts > 0 ? &prompt : nullptr;
    if (beam == 0) {                                           // greedy: at most 10 tokens per 80 ms frame
        nemo_hypothesis h;
        const int32_t cap = n_samples / 128 + 16;
        h.tokens.assign((size_t)cap, 0); h.frames.assign((size_t)cap, 0);
        int32_t *tp = h.tokens.data(), *fp = h.frames.data(), n = 0;
        if (nasr_engine_transcribe(ctx->engine, 1, &audio, &n_samples, pp, &tp, &cap, &n, &fp, 0) < 0) {
            fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
            return out;
        }
        h.tokens.resize((size_t)std::min(n, cap)); h.frames.resize(h.tokens.size());
        h.score = NAN;
        const auto read = [&](int (*get)(nasr_engine *, int, float *, int32_t), std::vector<float> &v) {      // the call's per-token values, by token
            v.assign(h.tokens.size(), NAN);
            return h.tokens.empty() || get(ctx->engine, 0, v.data(), (int32_t)v.size()) >= 0;
        };
        if ((ctx->token_logprobs && !read(nasr_engine_offline_token_logprobs, h.logprobs)) || (ctx->token_entropy_milli && !read(nasr_engine_offline_token_entropies, h.entropies))) {
            fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
            return out;
        }
        out.push_back(h);
        return out;
    }
    nasr_beam_params bp;
    bp.beam = beam; bp.nbest = nbest; bp.max_symbols = max_symbols; bp.reserved = 0;
    int32_t n_hyps = 0;
    if (nasr_engine_transcribe_beam(ctx->engine, 1, &audio, &n_samples, pp, &bp, &n_hyps, ctx->beam_boost ? NASR_FLAG_BEAM_BOOST : 0) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return out;
    }
    return read_beam_hypotheses(ctx, n_hyps, __func__);
}

bool nemo_set_language(nemo_context *ctx, const char *lang) {
    if (!ctx || !lang) return false;
    return lookup_lang(ctx, lang, __func__, ctx->prompt_index);
}

nemo_stream_context *nemo_stream_init(nemo_context *ctx, const nemo_cache_config *config) {
    if (!ctx) return nullptr;
    nemo_stream_context *s = new nemo_stream_context();
    s->nctx = ctx;
    if (config) s->config = *config;
    // architecture fields always come from the loaded header (reference src/nemo-stream.cpp:704-728)
    s->config.att_left_context = ctx->hparams.att_left_context;
    s->config.subsampling_factor = ctx->hparams.subsampling_factor;
    s->config.n_mels = ctx->hparams.n_mels;
    s->prompt_index = ctx->hparams.num_prompts > 0 ? ctx->prompt_index : -1;
    if (nasr_stream_create(ctx->engine, s->config.att_right_context, s->prompt_index, &s->stream) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        delete s;
        return nullptr;
    }
    return s;
}

bool nemo_stream_set_language(nemo_stream_context *sctx, const char *lang) {
    if (!sctx || !lang) return false;
    int idx;
    if (!lookup_lang(sctx->nctx, lang, __func__, idx)) return false;
    if (nasr_stream_set_prompt(sctx->stream, idx) < 0) return false;
    sctx->prompt_index = idx;
    return true;
}

static std::string absorb(nemo_stream_context *s, const int32_t *tok, int n) {
    if (n <= 0) return "";
    std::vector<int> ids(tok, tok + n);
    s->tokens.insert(s->tokens.end(), ids.begin(), ids.end());
    std::string text = tokens_to_text(ids, s->nctx->vocab);
    s->transcript += text;
    return text;
}

// one engine call for B streams: nasr_engine_step on s16 16 kHz mono, or (own_format) nasr_engine_step_audio on each stream's own format
static bool process_batch(nemo_stream_context *const *sctx, int B, const void *const *audio, const int *n_samples, std::string *out, bool own_format,
                          const char *who) {
    if (!sctx || B <= 0 || !audio || !n_samples) return false;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<nasr_stream *> st((size_t)B);
    std::vector<std::vector<int32_t>> buf((size_t)B);
    std::vector<int32_t *> ptr((size_t)B);
    std::vector<int32_t> cap((size_t)B), cnt((size_t)B), ns((size_t)B);
    for (int b = 0; b < B; b++) {
        if (!sctx[b]) return false;
        st[b] = sctx[b]->stream;
        ns[b] = n_samples[b] > 0 ? n_samples[b] : 0;
        cap[b] = (ns[b] / (own_format ? 640 : 1280) + 16) * 10;      // <= 10 symbols per 80 ms frame (640 input frames at 8 kHz)
        buf[b].resize((size_t)cap[b]);
        ptr[b] = buf[b].data();
    }
    const int rc = own_format ? nasr_engine_step_audio(sctx[0]->nctx->engine, st.data(), B, audio, ns.data(), ptr.data(), cap.data(), cnt.data(), 0)
                              : nasr_engine_step(sctx[0]->nctx->engine, st.data(), B, (const int16_t *const *)audio, ns.data(), ptr.data(), cap.data(), cnt.data(), 0);
    if (rc < 0) {
        fprintf(stderr, "%s: %s\n", who, nasr_last_error());
        return false;
    }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int b = 0; b < B; b++) {
        nemo_stream_context *s = sctx[b];
        s->total_audio_seconds += (double)ns[b] / (own_format ? s->audio_rate : s->config.sample_rate);
        s->total_compute_seconds += dt / B;
        std::string text = absorb(s, buf[b].data(), cnt[b]);
        // a full buffer: more tokens may be queued on the stream (nothing is dropped below the ABI) -- fetch them now
        while (cnt[b] >= cap[b]) {
            if (nasr_engine_collect(s->nctx->engine, &st[b], 1, &ptr[b], &cap[b], &cnt[b]) < 0) {
                fprintf(stderr, "%s: %s\n", who, nasr_last_error());
                return false;
            }
            text += absorb(s, buf[b].data(), cnt[b]);
        }
        if (out) out[b] = text;
        // host-mirror counter: no device synchronisation on the per-call path (a pipelined step stays in flight)
        nasr_stream_stats stt;
        if (nasr_stream_get_progress(s->stream, &stt) == 0) s->total_chunks_processed = stt.chunks;
    }
    return true;
}

bool nemo_stream_process_batch(nemo_stream_context *const *sctx, int B, const int16_t *const *audio,
                               const int *n_samples, std::string *out) {
    return process_batch(sctx, B, (const void *const *)audio, n_samples, out, false, __func__);
}

bool nemo_stream_set_audio_format(nemo_stream_context *sctx, int sample_rate, int encoding, int channels, int channel) {
    if (!sctx) return false;
    const nasr_audio_format f = {sample_rate, encoding, channels, channel};
    if (nasr_stream_set_audio_format(sctx->stream, &f) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    sctx->audio_rate = sample_rate; sctx->audio_encoding = encoding; sctx->audio_channels = channels; sctx->audio_channel = channel;
    return true;
}

std::string nemo_stream_process_audio(nemo_stream_context *sctx, const void *audio, int n_frames) {
    if (!sctx || !audio || n_frames <= 0) return "";
    std::string out;
    if (!process_batch(&sctx, 1, &audio, &n_frames, &out, true, __func__)) return "";
    return out;
}

std::string nemo_stream_process_incremental(nemo_stream_context *sctx, const int16_t *audio, int n_samples) {
    if (!sctx || !audio || n_samples <= 0) return "";         // reference src/nemo-stream.cpp:1150
    std::string out;
    if (!nemo_stream_process_batch(&sctx, 1, &audio, &n_samples, &out)) return "";
    return out;
}

bool nemo_stream_collect_batch(nemo_stream_context *const *sctx, int B, std::string *out) {
    if (!sctx || B <= 0) return false;
    std::vector<nasr_stream *> st((size_t)B);
    std::vector<std::vector<int32_t>> buf((size_t)B, std::vector<int32_t>(256));
    std::vector<int32_t *> ptr((size_t)B);
    std::vector<int32_t> cap((size_t)B, 256), cnt((size_t)B);
    for (int b = 0; b < B; b++) {
        if (!sctx[b]) return false;
        st[b] = sctx[b]->stream;
        ptr[b] = buf[b].data();
    }
    for (bool more = true; more;) {
        if (nasr_engine_collect(sctx[0]->nctx->engine, st.data(), B, ptr.data(), cap.data(), cnt.data()) < 0) {
            fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
            return false;
        }
        more = false;
        for (int b = 0; b < B; b++) {
            const std::string text = absorb(sctx[b], buf[b].data(), cnt[b]);
            if (out) out[b] += text;
            more = more || cnt[b] >= cap[b];
        }
    }
    return true;
}

bool nemo_stream_finalize_batch(nemo_stream_context *const *sctx, int B, std::string *out) {
    if (!sctx || B <= 0) return false;
    std::vector<nasr_stream *> st((size_t)B);
    std::vector<std::vector<int32_t>> buf((size_t)B, std::vector<int32_t>(256));
    std::vector<int32_t *> ptr((size_t)B);
    std::vector<int32_t> cap((size_t)B, 256), cnt((size_t)B);
    for (int b = 0; b < B; b++) {
        if (!sctx[b] || sctx[b]->nctx != sctx[0]->nctx) return false;
        st[(size_t)b] = sctx[b]->stream;
        ptr[(size_t)b] = buf[(size_t)b].data();
    }
    if (nasr_engine_finalize(sctx[0]->nctx->engine, st.data(), B, ptr.data(), cap.data(), cnt.data()) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    for (bool more = true; more;) {
        more = false;
        for (int b = 0; b < B; b++) {
            const std::string text = absorb(sctx[b], buf[(size_t)b].data(), cnt[(size_t)b]);
            if (out) out[b] += text;
            more = more || cnt[(size_t)b] >= cap[(size_t)b];
        }
        if (more && nasr_engine_collect(sctx[0]->nctx->engine, st.data(), B, ptr.data(), cap.data(), cnt.data()) < 0) {
            fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
            return false;
        }
    }
    return true;
}

std::string nemo_stream_finalize(nemo_stream_context *sctx) {
    if (!sctx) return "";
    int32_t tok[256], cap = 256, cnt = 0;
    int32_t *tp = tok;
    if (nasr_engine_finalize(sctx->nctx->engine, &sctx->stream, 1, &tp, &cap, &cnt) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return "";
    }
    // the text produced by the tail flush (:1292) -- with pipelined steps also the step that was still in flight
    std::string text = absorb(sctx, tok, cnt);
    while (cnt >= cap) {
        if (nasr_engine_collect(sctx->nctx->engine, &sctx->stream, 1, &tp, &cap, &cnt) < 0) {
            fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
            break;
        }
        text += absorb(sctx, tok, cnt);
    }
    return text;
}

nemo_stream_context *nemo_stream_fork(nemo_stream_context *sctx) {
    if (!sctx) return nullptr;
    nemo_stream_context *f = new nemo_stream_context(*sctx);      // config, prompt, audio format, transcript, tokens, endpoint detector state and events, timing
    f->stream = nullptr;
    if (nasr_stream_fork(sctx->stream, &f->stream) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        delete f;
        return nullptr;
    }
    return f;
}

bool nemo_stream_save(nemo_stream_context *sctx, std::vector<uint8_t> &out) {
    out.clear();
    if (!sctx) return false;
    nemo_env::Envelope env;
    int64_t need = 0;
    nasr_stream_save(sctx->stream, nullptr, 0, &need);          // the size of THIS stream's blob (an error by contract, with the size set)
    if (need <= 0) { fprintf(stderr, "%s: %s\n", __func__, nasr_last_error()); return false; }
    env.engine_blob.resize((size_t)need);
    if (nasr_stream_save(sctx->stream, env.engine_blob.data(), need, &need) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    env.engine_blob.resize((size_t)need);
    env.transcript = sctx->transcript;
    env.tokens.assign(sctx->tokens.begin(), sctx->tokens.end());
    env.right_context = sctx->config.att_right_context; env.prompt_index = sctx->prompt_index;
    env.audio_rate = sctx->audio_rate; env.audio_encoding = sctx->audio_encoding; env.audio_channels = sctx->audio_channels; env.audio_channel = sctx->audio_channel;
    env.ep_on = sctx->ep_on ? 1 : 0;
    memcpy(&env.ep_min_blank_bits, &sctx->ep_cfg.min_blank_logprob, 4);
    env.ep_idle = sctx->ep_cfg.silence_frames_idle; env.ep_after_speech = sctx->ep_cfg.silence_frames_after_speech; env.ep_max_utterance = sctx->ep_cfg.max_utterance_frames;
    env.ep_utt_start = sctx->ep_state.utt_start; env.ep_state_tokens = sctx->ep_state.tokens; env.ep_trailing = sctx->ep_state.trailing;
    env.ep_frames = sctx->ep_frames; env.ep_tokens = sctx->ep_tokens;
    for (const nasr_endpoint::Event &ev : sctx->ep_events) env.ep_events.push_back(nemo_env::Event{ev.frame, ev.utt_start, ev.rule, ev.tokens});
    memcpy(&env.audio_seconds_bits, &sctx->total_audio_seconds, 8);
    env.chunks_processed = sctx->total_chunks_processed;
    nemo_env::write(env, out);
    return true;
}

nemo_stream_context *nemo_stream_restore(nemo_context *ctx, const uint8_t *data, size_t size) {
    if (!ctx || !data) return nullptr;
    nemo_env::Envelope env;
    std::string err;
    if (!nemo_env::parse(data, (int64_t)size, env, err)) {
        fprintf(stderr, "%s: %s\n", __func__, err.c_str());
        return nullptr;
    }
    nemo_stream_context *s = new nemo_stream_context();
    s->nctx = ctx;
    if (nasr_stream_restore(ctx->engine, env.engine_blob.data(), (int64_t)env.engine_blob.size(), &s->stream) < 0) {      // the engine checks everything the blob says, right_context and prompt included
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        delete s;
        return nullptr;
    }
    s->config.att_right_context = env.right_context;
    s->config.att_left_context = ctx->hparams.att_left_context;
    s->config.subsampling_factor = ctx->hparams.subsampling_factor;
    s->config.n_mels = ctx->hparams.n_mels;
    s->prompt_index = env.prompt_index;
    s->audio_rate = env.audio_rate; s->audio_encoding = env.audio_encoding; s->audio_channels = env.audio_channels; s->audio_channel = env.audio_channel;
    s->transcript = env.transcript;
    s->tokens.assign(env.tokens.begin(), env.tokens.end());
    s->ep_on = env.ep_on != 0;
    memcpy(&s->ep_cfg.min_blank_logprob, &env.ep_min_blank_bits, 4);
    s->ep_cfg.silence_frames_idle = env.ep_idle; s->ep_cfg.silence_frames_after_speech = env.ep_after_speech; s->ep_cfg.max_utterance_frames = env.ep_max_utterance;
    s->ep_state.utt_start = env.ep_utt_start; s->ep_state.tokens = env.ep_state_tokens; s->ep_state.trailing = env.ep_trailing;
    s->ep_frames = env.ep_frames; s->ep_tokens = env.ep_tokens;
    for (const nemo_env::Event &ev : env.ep_events) { nasr_endpoint::Event o; o.frame = ev.frame; o.utt_start = ev.utt_start; o.rule = ev.rule; o.tokens = ev.tokens; s->ep_events.push_back(o); }
    memcpy(&s->total_audio_seconds, &env.audio_seconds_bits, 8);
    s->total_chunks_processed = env.chunks_processed;
    return s;
}

std::string nemo_stream_preview(nemo_stream_context *sctx) {
    if (!sctx) return "";
    int32_t tok[256], cap = 256, cnt = 0;
    int32_t *tp = tok;
    if (nasr_engine_preview(sctx->nctx->engine, &sctx->stream, 1, &tp, &cap, &cnt, nullptr) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return "";
    }
    return tokens_to_text(std::vector<int>(tok, tok + std::min(cnt, cap)), sctx->nctx->vocab);      // tentative: neither the transcript nor the tokens change
}

std::string beam_hypothesis_line(size_t rank, const nemo_hypothesis &h, const std::vector<std::string> &vocab) {
    const std::string text = tokens_to_text(std::vector<int>(h.tokens.begin(), h.tokens.end()), vocab);
    char head[160];
    if (h.has_boost && h.has_lm) snprintf(head, sizeof(head), "%zu %.6f %.6f %.6f %.6f ", rank, h.score, h.lm_logprob, h.boost, h.total);
    else if (h.has_boost) snprintf(head, sizeof(head), "%zu %.6f %.6f %.6f ", rank, h.score, h.boost, h.total);
    else if (h.has_lm) snprintf(head, sizeof(head), "%zu %.6f %.6f %.6f ", rank, h.score, h.lm_logprob, h.total);
    else snprintf(head, sizeof(head), "%zu %.6f ", rank, h.score);
    return head + text;
}

bool nemo_set_frame_history(nemo_context *ctx, int frames) {
    if (!ctx || !ctx->engine) return false;
    if (nasr_engine_set_option(ctx->engine, "frame_history", frames) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    return true;
}

bool nemo_stream_history_range(nemo_stream_context *sctx, int64_t *first, int *count) {
    int32_t n = 0;
    if (!sctx || !first || !count) return false;
    if (nasr_stream_history_range(sctx->stream, first, &n) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return false;
    }
    *count = n;
    return true;
}

std::vector<nemo_hypothesis> nemo_stream_second_pass_beam(nemo_stream_context *sctx, int64_t first, int count, int beam, int nbest, int max_symbols) {
    std::vector<nemo_hypothesis> out;
    if (!sctx || !sctx->nctx || !sctx->nctx->engine) return out;
    nemo_context *ctx = sctx->nctx;
    nasr_beam_params bp;
    bp.beam = beam; bp.nbest = nbest; bp.max_symbols = max_symbols; bp.reserved = 0;
    const int32_t cnt = count;
    int32_t n_hyps = 0;
    if (nasr_engine_history_beam(ctx->engine, &sctx->stream, 1, &first, &cnt, &bp, &n_hyps, ctx->beam_boost ? NASR_FLAG_BEAM_BOOST : 0) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return out;
    }
    return read_beam_hypotheses(ctx, n_hyps, __func__);
}

nemo_alignment nemo_stream_second_pass_align(nemo_stream_context *sctx, int64_t first, int count, const std::vector<int32_t> &tokens) {
    nemo_alignment out;
    if (!sctx || !sctx->nctx || !sctx->nctx->engine) return out;
    out.frames.assign(tokens.size(), -1);
    out.logprobs.assign(tokens.size(), NAN);
    const int32_t n_tok = (int32_t)tokens.size(), cnt = count;
    const int32_t *tp = tokens.data();
    int32_t *fp = out.frames.data();
    float *lp = out.logprobs.data();
    if (nasr_engine_history_align(sctx->nctx->engine, &sctx->stream, 1, &first, &cnt, &tp, &n_tok, &out.loglik, &out.best, &fp, &lp, 0) < 0) {
        fprintf(stderr, "%s: %s\n", __func__, nasr_last_error());
        return out;
    }
    out.ok = true;
    return out;
}

std::string nemo_stream_get_transcript(nemo_stream_context *sctx) { return sctx ? sctx->transcript : ""; }

const std::vector<int> &nemo_stream_get_tokens(nemo_stream_context *sctx) {
    static const std::vector<int> empty;
    return sctx ? sctx->tokens : empty;
}

void nemo_stream_reset(nemo_stream_context *sctx) {
    if (!sctx) return;
    // the reference's reset as coded (src/nemo-stream.cpp:95-115): the conv cache and the preprocessor carry survive
    nasr_stream_reset_ex(sctx->stream, NASR_RESET_REFERENCE);
    sctx->tokens.clear();
    sctx->transcript.clear();
    sctx->total_audio_seconds = sctx->total_compute_seconds = 0;
    sctx->total_chunks_processed = 0;
    sctx->ep_state = nasr_endpoint::State();          // the engine's frame and token counts restart at 0 with the reset
    sctx->ep_frames = sctx->ep_tokens = 0;
    sctx->ep_events.clear();
}

void nemo_stream_free(nemo_stream_context *sctx) {
    if (!sctx) return;
    nasr_stream_destroy(sctx->stream);
    delete sctx;
}
