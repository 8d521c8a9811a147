// token_confidence.h -- per-token and per-word confidence from per-token entropies (engine option "token_entropy" = round(1000 alpha)),
// pure host code so that the CPU suite compiles it under sanitizers (tests/test_token_confidence.py), like word_confidence.h, whose word
// cut it reuses.  The engine reports H, the entropy of order alpha (Renyi; Shannon at alpha = 1) in nats of the joint's softmax over
// V = 1025 outputs where a token was emitted.  The maps to [0, 1] are those of entropy-based confidence estimation (Laptev and Ginsburg,
// "Fast entropy-based methods of word-level confidence estimation for end-to-end automatic speech recognition"; NeMo's `entropy` method):
//   Renyi / Shannon (METHOD_ENTROPY)   lin: 1 - H / ln V                   exp: (V e^-H - 1) / (V - 1)
//   Tsallis (METHOD_TSALLIS, alpha != 1): T = (1 - e^((1 - alpha) H)) / (alpha - 1), T_max = (1 - V^(1 - alpha)) / (alpha - 1)
//                                      lin: 1 - T / T_max                  exp: (e^-T - e^-T_max) / (1 - e^-T_max)
// (sum p^alpha = e^((1 - alpha) H): the Tsallis entropy needs nothing but H.)  Every map gives 1 at H = 0 and 0 at H = ln V and falls
// monotonically between them; NaN (a token that has left the engine's ring) stays NaN.  At alpha = 1 Tsallis is Shannon.
// A word's confidence is the min, the mean or the product of its tokens' confidences; words are cut by word_conf::words.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "word_confidence.h"

namespace token_conf {

constexpr int VOCAB = 1025;
enum Method { METHOD_ENTROPY = 0, METHOD_TSALLIS = 1 };
enum Norm { NORM_LIN = 0, NORM_EXP = 1 };
enum Agg { AGG_MIN = 0, AGG_MEAN = 1, AGG_PROD = 2 };

inline double clamp01(double c) { return c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c); }      // NaN passes: both comparisons are false

// one token: H in nats, alpha the order the engine was set to (1 = Shannon)
inline float confidence(float H, double alpha, Method method, Norm norm) {
    if (std::isnan(H)) return NAN;
    const double V = (double)VOCAB, lnV = std::log(V), h = (double)H;
    if (method == METHOD_ENTROPY || alpha == 1.0) {
        if (norm == NORM_LIN) return (float)clamp01(1.0 - h / lnV);
        return (float)clamp01((V * std::exp(-h) - 1.0) / (V - 1.0));
    }
    // 1 - e^x through expm1: near alpha = 1 the difference would otherwise cancel
    const double T = -std::expm1((1.0 - alpha) * h) / (alpha - 1.0), Tmax = -std::expm1((1.0 - alpha) * lnV) / (alpha - 1.0);
    if (norm == NORM_LIN) return (float)clamp01(1.0 - T / Tmax);
    return (float)clamp01((std::exp(-T) - std::exp(-Tmax)) / -std::expm1(-Tmax));
}
inline std::vector<float> confidences(const std::vector<float> &entropies, double alpha, Method method, Norm norm) {
    std::vector<float> c(entropies.size());
    for (size_t i = 0; i < c.size(); i++) c[i] = confidence(entropies[i], alpha, method, norm);
    return c;
}

// min, mean or product of n confidences; any NaN makes the result NaN, no token at all too
inline float aggregate(const float *c, size_t n, Agg agg) {
    if (n == 0) return NAN;
    double acc = agg == AGG_PROD ? 1.0 : (agg == AGG_MEAN ? 0.0 : (double)c[0]);
    for (size_t i = 0; i < n; i++) {
        if (std::isnan(c[i])) return NAN;
        if (agg == AGG_MIN) acc = (double)c[i] < acc ? (double)c[i] : acc;
        else if (agg == AGG_MEAN) acc += (double)c[i];
        else acc *= (double)c[i];
    }
    return (float)(agg == AGG_MEAN ? acc / (double)n : acc);
}

// word_conf::words' words with Word::confidence = the aggregate of the per-token confidences (conf[i] belongs to tokens[i]; a shorter
// list leaves the tokens beyond it at NaN).  Ids outside the vocabulary are skipped, as the word cut skips them
inline std::vector<word_conf::Word> words(const std::vector<int> &tokens, const std::vector<float> &conf, const std::vector<std::string> &vocab, Agg agg) {
    std::vector<word_conf::Word> ws = word_conf::words(tokens, std::vector<float>(), vocab);
    for (size_t k = 0; k < ws.size(); k++) {
        const size_t end = k + 1 < ws.size() ? (size_t)ws[k + 1].first_token : tokens.size();
        std::vector<float> c;
        for (size_t i = (size_t)ws[k].first_token; i < end; i++) {
            if (tokens[i] < 0 || tokens[i] >= (int)vocab.size()) continue;
            c.push_back(i < conf.size() ? conf[i] : NAN);
        }
        ws[k].confidence = aggregate(c.data(), c.size(), agg);
    }
    return ws;
}

inline bool parse_method(const std::string &s, bool *max_prob, Method *m) {
    *max_prob = s == "max_prob";
    if (s == "entropy") *m = METHOD_ENTROPY; else if (s == "tsallis") *m = METHOD_TSALLIS; else return *max_prob;
    return true;
}
inline bool parse_norm(const std::string &s, Norm *n) { if (s == "lin") *n = NORM_LIN; else if (s == "exp") *n = NORM_EXP; else return false; return true; }
inline bool parse_agg(const std::string &s, Agg *a) { if (s == "min") *a = AGG_MIN; else if (s == "mean") *a = AGG_MEAN; else if (s == "prod") *a = AGG_PROD; else return false; return true; }

// max_prob under the same aggregations: the per-token confidence is P(token) = exp(ln P)
inline std::vector<float> max_prob_confidences(const std::vector<float> &logprobs) {
    std::vector<float> c(logprobs.size());
    for (size_t i = 0; i < c.size(); i++) c[i] = std::isnan(logprobs[i]) ? NAN : std::exp(logprobs[i]);
    return c;
}

}  // namespace token_conf
