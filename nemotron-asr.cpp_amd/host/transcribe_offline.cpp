// nemotron-transcribe-amd -- offline (full-context) transcription of one whole utterance on the MI355X engine: the greedy decode
// (nasr_engine_transcribe), or with --beam the N best distinct transcripts of the frame-synchronous beam search
// (nasr_engine_transcribe_beam, through nemo_transcribe_beam).  The reference's counterpart is nemo_transcribe_audio (greedy only).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nemo_amd.h"
#include "token_confidence.h"

static void usage(const char *prog) {
    fprintf(stderr,
            "Usage: %s <model.gguf> <audio.pcm> [--beam W] [--nbest N] [--max-symbols S] [--lm FILE.arpa] [--lm-weight X] [--token-bonus Y] [--boost-file FILE] [--boost-bonus X] [--f32] [--device N] [--lang CODE] [--print-tokens] [--confidence] [--confidence-method M] [--confidence-alpha A] [--confidence-norm N] [--confidence-agg G]\n"
            "  audio: raw s16le, 16 kHz, mono, one whole utterance (up to 2048 encoder frames = 163.8 s)\n"
            "  without --beam: the greedy transcript, one line\n"
            "  --beam W (1 .. 8): one line per hypothesis, best first: rank score text   (score = ln P of the hypothesis's best path;\n"
            "  --nbest N <= W hypotheses, default W; --max-symbols S tokens per 80 ms frame, 1 .. 10, default 4).  Beam 1 is not the greedy decode\n"
            "  --lm FILE.arpa (with --beam): shallow fusion of a back-off n-gram model over the vocabulary's pieces (one piece or ids:N per ARPA\n"
            "  word, <s>, </s>, <unk>; up to 5-grams); hypotheses rank by total = score + X * lm + Y * tokens (--lm-weight X, default 0.5;\n"
            "  --token-bonus Y, default 0; both 0 .. 100) and the lines read: rank score lm total text.  The model re-scores the transducer's\n"
            "  candidates, it proposes none\n"
            "  --lm without --beam: the greedy decode is fused instead: arg-max over logit + X * ln P_lm(token | tokens so far) + Y for every\n"
            "  non-blank token, blank unbiased (Y offsets the deletions that follow from that); here the model can propose a token.  --lm-weight\n"
            "  must then be given: 0.5 is the beam search's default, the greedy decode's own is 0 (nothing fused), and the useful values differ\n"
            "  --boost-file F: phrase boosting: one phrase per line, `phrase<TAB>bonus` (bonus optional; natural-log units added to the logits of the\n"
            "  tokens that start or continue a phrase; `ids:1,2,3` gives literal token ids); --boost-bonus X: the bonus of lines that give none\n"
            "  (default 4.0).  Without --beam the greedy decode is boosted.  With --beam the search is boosted: a boosted token is proposed even outside a\n"
            "  hypothesis' largest outputs, hypotheses rank by total = score (+ the LM terms) + boost, and the lines read: rank score [lm] boost total text\n"
            "  --confidence (greedy only): the transcript again with [0.93] behind every word, exp of the smallest ln P among the word's tokens.\n"
            "  --confidence-method max_prob|entropy|tsallis [--confidence-alpha A] [--confidence-norm lin|exp] [--confidence-agg min|mean|prod]: the\n"
            "  bracketed number becomes the chosen measure, as in nemotron-asr-amd (A default 0.333, norm default exp, agg default min)\n"
            "  --print-tokens: after each line `tokens ...` and `frames ...`, the ids and the encoder frame each is emitted at\n",
            prog);
}

int main(int argc, char **argv) {
    if (argc < 3) { usage(argv[0]); return 1; }
    const char *model_path = argv[1], *audio_path = argv[2], *lang = nullptr;
    int device = 0, dtype = 1, beam = 0, nbest = 0, max_symbols = 0;
    bool print_tokens = false;
    bool confidence = false, conf_opts = false, conf_entropy_opts = false, conf_max_prob = true;
    token_conf::Method conf_method = token_conf::METHOD_ENTROPY;
    token_conf::Norm conf_norm = token_conf::NORM_EXP;
    token_conf::Agg conf_agg = token_conf::AGG_MIN;
    float conf_alpha = 0.333f;
    const char *lm_path = nullptr;
    float lm_weight = 0.5f, token_bonus = 0.0f;
    bool lm_opts = false, lm_weight_given = false, boost_opts = false;
    const char *boost_file = nullptr;
    float boost_bonus = 4.0f;
    for (int i = 3; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--lang" && i + 1 < argc) lang = argv[++i];
        else if (a == "--device" && i + 1 < argc) device = atoi(argv[++i]);
        else if (a == "--beam" && i + 1 < argc) beam = atoi(argv[++i]);
        else if (a == "--nbest" && i + 1 < argc) nbest = atoi(argv[++i]);
        else if (a == "--max-symbols" && i + 1 < argc) max_symbols = atoi(argv[++i]);
        else if (a == "--lm" && i + 1 < argc) lm_path = argv[++i];
        else if (a == "--lm-weight" && i + 1 < argc) { lm_weight = strtof(argv[++i], nullptr); lm_opts = lm_weight_given = true; }
        else if (a == "--token-bonus" && i + 1 < argc) { token_bonus = strtof(argv[++i], nullptr); lm_opts = true; }
        else if (a == "--boost-file" && i + 1 < argc) boost_file = argv[++i];
        else if (a == "--boost-bonus" && i + 1 < argc) { boost_bonus = strtof(argv[++i], nullptr); boost_opts = true; }
        else if (a == "--f32") dtype = 0;
        else if (a == "--print-tokens") print_tokens = true;
        else if (a == "--confidence") confidence = true;
        else if (a == "--confidence-method" && i + 1 < argc) {
            if (!token_conf::parse_method(argv[++i], &conf_max_prob, &conf_method)) { fprintf(stderr, "--confidence-method must be max_prob, entropy or tsallis (got %s)\n", argv[i]); return 1; }
            confidence = conf_opts = true;
        }
        else if (a == "--confidence-alpha" && i + 1 < argc) { conf_alpha = strtof(argv[++i], nullptr); confidence = conf_opts = conf_entropy_opts = true; }
        else if (a == "--confidence-norm" && i + 1 < argc) {
            if (!token_conf::parse_norm(argv[++i], &conf_norm)) { fprintf(stderr, "--confidence-norm must be lin or exp (got %s)\n", argv[i]); return 1; }
            confidence = conf_opts = conf_entropy_opts = true;
        }
        else if (a == "--confidence-agg" && i + 1 < argc) {
            if (!token_conf::parse_agg(argv[++i], &conf_agg)) { fprintf(stderr, "--confidence-agg must be min, mean or prod (got %s)\n", argv[i]); return 1; }
            confidence = conf_opts = true;
        }
        else { usage(argv[0]); return 1; }
    }
    if (beam == 0 && (nbest != 0 || max_symbols != 0)) { fprintf(stderr, "--nbest and --max-symbols go with --beam\n"); return 1; }
    if (beam < 0) { fprintf(stderr, "--beam must be 1 .. 8\n"); return 1; }
    if (lm_path && beam == 0 && !lm_weight_given) {
        fprintf(stderr, "--lm without --beam fuses the greedy decode and needs --lm-weight X (0.5 is the beam search's default; the greedy decode's own is 0: nothing fused)\n");
        return 1;
    }
    if (lm_opts && !lm_path) { fprintf(stderr, "--lm-weight and --token-bonus go with --lm\n"); return 1; }
    if (confidence && beam != 0) { fprintf(stderr, "--confidence and its options go with the greedy mode (no --beam)\n"); return 1; }
    if (conf_entropy_opts && conf_max_prob) { fprintf(stderr, "--confidence-alpha and --confidence-norm go with --confidence-method entropy or tsallis\n"); return 1; }
    if (boost_opts && !boost_file) { fprintf(stderr, "--boost-bonus goes with --boost-file\n"); return 1; }
    FILE *in = fopen(audio_path, "rb");
    if (!in) { fprintf(stderr, "Failed to open audio file: %s\n", audio_path); return 1; }
    std::vector<int16_t> pcm;
    std::vector<int16_t> buf(1 << 16);
    for (size_t got; (got = fread(buf.data(), sizeof(int16_t), buf.size(), in)) > 0;) pcm.insert(pcm.end(), buf.begin(), buf.begin() + (long)got);
    fclose(in);

    nemo_context *ctx = nemo_init_with_device(model_path, device, dtype, 1);
    if (!ctx) { fprintf(stderr, "Failed to load model: %s\n", model_path); return 1; }
    if (lang && !nemo_set_language(ctx, lang)) { fprintf(stderr, "Failed to set language '%s'\n", lang); nemo_free(ctx); return 1; }
    if (confidence && conf_max_prob && !nemo_set_token_logprobs(ctx, true)) { nemo_free(ctx); return 1; }
    if (confidence && !conf_max_prob && !nemo_set_token_entropy(ctx, conf_alpha)) { fprintf(stderr, "--confidence-alpha must be 0.05 .. 0.9, 1 or 1.1 .. 4\n"); nemo_free(ctx); return 1; }
    if (lm_path && beam == 0 && !nemo_set_lm_fusion(ctx, true)) { nemo_free(ctx); return 1; }      // greedy: the model biases the device decode, by weights of its own
    if (lm_path && !nemo_load_lm_arpa(ctx, lm_path, beam == 0 ? 0.0f : lm_weight, beam == 0 ? 0.0f : token_bonus)) { nemo_free(ctx); return 1; }
    if (lm_path && beam == 0 && !nemo_set_greedy_lm_weights(ctx, lm_weight, token_bonus)) { nemo_free(ctx); return 1; }
    if (boost_file && !(nemo_set_phrase_boost(ctx, 4096) && nemo_load_boost_file(ctx, boost_file, boost_bonus) && (beam == 0 || nemo_set_beam_boost(ctx, true)))) {
        fprintf(stderr, "Failed to load boost phrases from '%s'\n", boost_file);
        nemo_free(ctx);
        return 1;
    }
    const std::vector<nemo_hypothesis> hyps = nemo_transcribe_beam(ctx, pcm.data(), (int)pcm.size(), beam, nbest, max_symbols);
    if (hyps.empty()) { nemo_free(ctx); return 1; }
    for (size_t r = 0; r < hyps.size(); r++) {
        const std::vector<int> toks(hyps[r].tokens.begin(), hyps[r].tokens.end());
        const std::string text = tokens_to_text(toks, ctx->vocab);
        if (beam == 0) printf("%s\n", text.c_str());
        else printf("%s\n", beam_hypothesis_line(r, hyps[r], ctx->vocab).c_str());
        if (confidence) {                                          // greedy only: the words again, each with its number
            const std::vector<word_conf::Word> ws =
                !conf_opts ? word_conf::words(toks, hyps[r].logprobs, ctx->vocab)
                           : token_conf::words(toks, conf_max_prob ? token_conf::max_prob_confidences(hyps[r].logprobs)
                                                                   : token_conf::confidences(hyps[r].entropies, (double)ctx->token_entropy_milli / 1000.0, conf_method, conf_norm),
                                               ctx->vocab, conf_agg);
            printf("%s\n", word_conf::annotate(ws).c_str());
        }
        if (print_tokens) {
            printf("tokens");
            for (int t : toks) printf(" %d", t);
            printf("\nframes");
            for (int f : hyps[r].frames) printf(" %d", f);
            printf("\n");
        }
    }
    nemo_free(ctx);
    return 0;
}
