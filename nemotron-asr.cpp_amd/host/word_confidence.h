// word_confidence.h -- per-word confidence from per-token log-probabilities (engine option "token_logprobs"), pure host code so
// that the CPU suite compiles it under sanitizers (tests/test_word_confidence.py), like server_protocol.h.
// Words are cut exactly where tokens_to_text (nemo_amd.cpp; reference src/nemo-ggml.cpp:1556-1583) cuts them: a piece that starts
// with U+2581 opens a word, every other piece continues the current one (pieces in front of the first U+2581 form a word of their
// own, glued to the start of the text as tokens_to_text glues them), ids outside the vocabulary are skipped.  A word's
// confidence is exp(min ln P of its tokens): NeMo's `max_prob` confidence measure with `min` aggregation over the word's
// tokens.  A token whose log-probability is NaN (it has left the engine's 4096-token ring) makes its word NaN.
#pragma once
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

namespace word_conf {

struct Word {
    std::string text;        // without the U+2581 marker
    bool opens;              // started by a U+2581 piece (tokens_to_text puts a space in front of it)
    int first_token;         // index into the token list of the word's first piece
    int n_tokens;            // pieces of the word (skipped ids not counted)
    float confidence;        // exp(min ln P), NaN if any of them is NaN
};

inline bool piece_opens_word(const std::string &piece) { return piece.compare(0, 3, "\xe2\x96\x81") == 0; }

// logprobs[i] belongs to tokens[i]; a shorter logprobs list leaves the tokens beyond it at NaN
inline std::vector<Word> words(const std::vector<int> &tokens, const std::vector<float> &logprobs, const std::vector<std::string> &vocab) {
    std::vector<Word> out;
    std::vector<float> min_lp;
    for (size_t i = 0; i < tokens.size(); i++) {
        const int id = tokens[i];
        if (id < 0 || id >= (int)vocab.size()) continue;
        const std::string &piece = vocab[(size_t)id];
        const bool opens = piece_opens_word(piece);
        if (opens || out.empty()) {
            out.push_back(Word{std::string(), opens, (int)i, 0, 0.0f});
            min_lp.push_back(0.0f);
        }
        Word &w = out.back();
        float &m = min_lp.back();
        w.text.append(piece, opens ? 3 : 0, std::string::npos);
        const float lp = i < logprobs.size() ? logprobs[i] : NAN;
        if (w.n_tokens == 0) m = lp;
        else if (std::isnan(lp) || std::isnan(m)) m = NAN;
        else if (lp < m) m = lp;
        w.n_tokens++;
    }
    for (size_t k = 0; k < out.size(); k++) out[k].confidence = std::isnan(min_lp[k]) ? NAN : std::exp(min_lp[k]);
    return out;
}

// tokens_to_text's text with "[0.93]" behind every word; stamps[k] (optional, "{12.34}"-style, one per word) goes in front of
// word k as tokens_to_text(timed, vocab, true) puts it
inline std::string annotate(const std::vector<Word> &ws, const std::vector<std::string> *stamps = nullptr) {
    std::string out;
    for (size_t k = 0; k < ws.size(); k++) {
        const Word &w = ws[k];
        if (w.opens) {
            out += ' ';
            if (stamps && k < stamps->size()) out += (*stamps)[k];
        }
        out += w.text;
        char buf[32];
        if (std::isnan(w.confidence)) snprintf(buf, sizeof(buf), "[nan]");
        else snprintf(buf, sizeof(buf), "[%.2f]", (double)w.confidence);
        out += buf;
    }
    return out;
}

}  // namespace word_conf
