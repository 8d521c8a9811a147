// align_words.h -- aligned tokens (nasr_engine_align*: a transcript's tokens, the encoder frame each is emitted at on the best path, and
// ln P of each there) -> word rows, pure host code so that the CPU suite compiles it under sanitizers (tests/test_align_math.py), like
// word_confidence.h, whose word cut and confidence rule it applies: a piece that starts with U+2581 opens a word, a word's confidence is
// exp(min ln P of its tokens).  A word starts where the frame of its first token starts and ends where the frame of its last token
// ends; a frame is 1280 samples at 16 kHz (80 ms).  A word whose tokens carry no frame (frames of -1: the utterance has no encoder frame,
// so the transcript has no alignment) gets start_s = end_s = -1.
#pragma once
#include "word_confidence.h"

namespace align_words {

constexpr double FRAME_S = 1280.0 / 16000.0;

struct Row { double start_s, end_s; float confidence; std::string word; };

inline std::vector<Row> rows(const std::vector<int> &tokens, const std::vector<int> &frames, const std::vector<float> &logprobs,
                             const std::vector<std::string> &vocab) {
    std::vector<Row> out;
    for (const word_conf::Word &w : word_conf::words(tokens, logprobs, vocab)) {
        int f0 = -1, f1 = -1, left = w.n_tokens;                   // frames of the word's first and last piece (skipped ids carry none)
        for (size_t i = (size_t)w.first_token; i < tokens.size() && left > 0; i++) {
            if (tokens[i] < 0 || tokens[i] >= (int)vocab.size()) continue;
            const int f = i < frames.size() ? frames[i] : -1;
            if (f0 < 0) f0 = f;
            f1 = f;
            left--;
        }
        const bool placed = f0 >= 0 && f1 >= 0;
        out.push_back(Row{placed ? f0 * FRAME_S : -1.0, placed ? (f1 + 1) * FRAME_S : -1.0, w.confidence, w.text});
    }
    return out;
}

}  // namespace align_words
