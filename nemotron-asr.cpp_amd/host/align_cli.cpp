// nemotron-align-amd -- forced alignment and transcript scoring of one utterance on the MI355X engine (nasr_engine_align, through
// nemo_align_audio): given audio and the transcript that was spoken, when was each word spoken, how sure is the model of it, and what is
// ln P(transcript | audio).  The reference has no counterpart.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "align_words.h"
#include "boost_phrases.h"
#include "nemo_amd.h"

static void usage(const char *prog) {
    fprintf(stderr,
            "Usage: %s <model.gguf> <audio.pcm> <transcript.txt | -> [--f32] [--device N] [--lang CODE] [--print-tokens]\n"
            "  audio: raw s16le, 16 kHz, mono, one whole utterance (up to 2048 encoder frames = 163.8 s)\n"
            "  transcript: text; every word is cut into vocabulary pieces by greedy longest match, `ids:12,55,9` gives token ids literally\n"
            "  prints one line per word: start_s end_s confidence word   (80 ms frames; confidence = exp(min ln P of the word's tokens)),\n"
            "  then `loglik X` = ln P(transcript | audio) and `best X` = the score of the best alignment\n"
            "  --print-tokens: also `tokens ...` and `frames ...`, the ids and the encoder frame each is emitted at\n",
            prog);
}

int main(int argc, char **argv) {
    if (argc < 4) { usage(argv[0]); return 1; }
    const char *model_path = argv[1], *audio_path = argv[2], *text_path = argv[3], *lang = nullptr;
    int device = 0, dtype = 1;
    bool print_tokens = false;
    for (int i = 4; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--lang" && i + 1 < argc) lang = argv[++i];
        else if (a == "--device" && i + 1 < argc) device = atoi(argv[++i]);
        else if (a == "--f32") dtype = 0;
        else if (a == "--print-tokens") print_tokens = true;
        else { usage(argv[0]); return 1; }
    }
    // inputs first: nothing of this needs the GPU
    FILE *in = fopen(audio_path, "rb");
    if (!in) { fprintf(stderr, "Failed to open audio file: %s\n", audio_path); return 1; }
    std::vector<int16_t> pcm;
    std::vector<int16_t> buf(1 << 16);
    for (size_t got; (got = fread(buf.data(), sizeof(int16_t), buf.size(), in)) > 0;) pcm.insert(pcm.end(), buf.begin(), buf.begin() + (long)got);
    fclose(in);
    FILE *tf = strcmp(text_path, "-") == 0 ? stdin : fopen(text_path, "rb");
    if (!tf) { fprintf(stderr, "Failed to open transcript: %s\n", text_path); return 1; }
    std::string text;
    for (int c; (c = fgetc(tf)) != EOF;) text.push_back((char)c);
    if (tf != stdin) fclose(tf);

    nemo_context *ctx = nemo_init_with_device(model_path, device, dtype, 1);
    if (!ctx) { fprintf(stderr, "Failed to load model: %s\n", model_path); return 1; }
    if (lang && !nemo_set_language(ctx, lang)) { fprintf(stderr, "Failed to set language '%s'\n", lang); nemo_free(ctx); return 1; }
    // the transcript, word by word
    const boost_phrases::Vocab vocab(ctx->vocab);
    std::vector<int32_t> tokens;
    for (size_t pos = 0; pos < text.size();) {
        while (pos < text.size() && strchr(" \t\r\n", text[pos])) pos++;
        size_t end = pos;
        while (end < text.size() && !strchr(" \t\r\n", text[end])) end++;
        if (end == pos) break;
        const std::string word = text.substr(pos, end - pos);
        pos = end;
        if (word.compare(0, 4, "ids:") == 0) {
            std::vector<int32_t> ids;
            const std::string why = boost_phrases::phrase_tokens(word, vocab, ids);
            if (!why.empty()) { fprintf(stderr, "transcript: \"%s\": %s\n", word.c_str(), why.c_str()); nemo_free(ctx); return 1; }
            tokens.insert(tokens.end(), ids.begin(), ids.end());
        } else if (!boost_phrases::segment_word(word, vocab, tokens)) {
            fprintf(stderr, "transcript: the vocabulary's pieces cannot spell \"%s\" (write it as ids:..)\n", word.c_str());
            nemo_free(ctx);
            return 1;
        }
    }
    const nemo_alignment al = nemo_align_audio(ctx, pcm.data(), (int)pcm.size(), tokens);
    if (!al.ok) { nemo_free(ctx); return 1; }
    if (!tokens.empty() && al.frames[0] < 0) {                 // audio too short for one encoder frame: no path through the lattice
        fprintf(stderr, "no alignment: the audio gives no encoder frame, the transcript has %zu tokens\n", tokens.size());
        nemo_free(ctx);
        return 1;
    }
    const std::vector<int> toks(tokens.begin(), tokens.end()), frames(al.frames.begin(), al.frames.end());
    for (const align_words::Row &r : align_words::rows(toks, frames, al.logprobs, ctx->vocab))
        printf("%.2f %.2f %.4f %s\n", r.start_s, r.end_s, (double)r.confidence, r.word.c_str());
    printf("loglik %.6f\nbest %.6f\n", al.loglik, al.best);
    if (print_tokens) {
        printf("tokens");
        for (int t : toks) printf(" %d", t);
        printf("\nframes");
        for (int f : frames) printf(" %d", f);
        printf("\n");
    }
    nemo_free(ctx);
    return 0;
}
