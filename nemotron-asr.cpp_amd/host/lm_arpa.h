// lm_arpa.h -- a small ARPA reader for the beam search's language model (nasr_engine_set_lm, csrc/nasr_lm.h), pure host code so that the CPU
// suite compiles it under sanitizers (tests/test_lm_abi.py), like boost_phrases.h.
// The model is over the transducer's own token ids, so an ARPA "word" is ONE vocabulary piece: it maps to the id of the piece with exactly
// that string (boost_phrases::Vocab); `ids:N` is the literal id N; <s> is BOS, </s> is EOS.  The unigram of <unk> becomes unk_logprob and is
// not an n-gram of the set; n-grams of higher order that contain <unk> are skipped and counted.  The file gives log10 values, the model takes
// natural logs.  Read: the \data\ counts (`ngram N=count`), the \N-grams: sections (`logprob<ws>w1 .. wN[<ws>backoff]`) and \end\.  A section's
// count must match its header.  Every error carries its line number.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "boost_phrases.h"

namespace lm_arpa {

constexpr int MAX_ORDER = 5, BOS = 1025, EOS = 1026;
constexpr double LN10 = 2.302585092994046;

struct Model {
    int order = 0;
    std::vector<int32_t> lengths, tokens;       // the layout of nasr_lm_desc
    std::vector<float> logprob, backoff;
    bool has_unk = false;
    float unk_logprob = 0.0f;
    long long skipped_unk = 0;
};

inline bool word_id(const std::string &w, const boost_phrases::Vocab &v, int32_t &id, std::string &why) {
    if (w == "<s>") { id = BOS; return true; }
    if (w == "</s>") { id = EOS; return true; }
    if (w.compare(0, 4, "ids:") == 0) {
        char *end = nullptr;
        const long x = strtol(w.c_str() + 4, &end, 10);
        if (end == w.c_str() + 4 || *end) { why = "malformed literal id \"" + w + "\" (want ids:12)"; return false; }
        if (x < 0 || x >= boost_phrases::N_TOKEN_IDS) { why = "token id " + std::to_string(x) + " is not a non-blank vocabulary id (0 .. 1023)"; return false; }
        id = (int32_t)x;
        return true;
    }
    const auto it = v.id.find(w);
    if (it == v.id.end()) { why = "\"" + w + "\" is not a piece of the vocabulary (write it as ids:N)"; return false; }
    id = it->second;
    return true;
}

inline bool number(const std::string &s, float &out) {
    char *end = nullptr;
    out = strtof(s.c_str(), &end);
    return end != s.c_str() && !*end && std::isfinite(out);
}

// "" or "line N: what is wrong"
inline std::string parse(const std::string &content, const boost_phrases::Vocab &v, Model &out) {
    out = Model();
    long long want[MAX_ORDER + 1] = {0}, seen[MAX_ORDER + 1] = {0};
    int line = 0, section = -1;                 // -1: before \data\, 0: in \data\, n: in \n-grams:
    bool ended = false;
    auto at = [&](const std::string &m) { return "line " + std::to_string(line) + ": " + m; };
    auto close = [&]() -> std::string {
        if (section >= 1 && seen[section] != want[section])
            return at("the " + std::to_string(section) + "-gram section has " + std::to_string(seen[section]) + " entries, \\data\\ announced " + std::to_string(want[section]));
        return "";
    };
    for (size_t pos = 0; pos < content.size() && !ended;) {
        size_t end = content.find('\n', pos);
        if (end == std::string::npos) end = content.size();
        std::string l = content.substr(pos, end - pos);
        pos = end + 1;
        line++;
        while (!l.empty() && (l.back() == '\r' || l.back() == ' ' || l.back() == '\t')) l.pop_back();
        if (l.empty()) continue;
        if (l[0] == '\\') {
            const std::string err = close();
            if (!err.empty()) return err;
            if (l == "\\data\\") { if (section != -1) return at("a second \\data\\"); section = 0; continue; }
            if (l == "\\end\\") { if (section < 0) return at("\\end\\ before \\data\\"); ended = true; continue; }
            char *e = nullptr;
            const long n = strtol(l.c_str() + 1, &e, 10);
            if (e == l.c_str() + 1 || std::string(e) != "-grams:") return at("unknown section \"" + l + "\"");
            if (section < 0) return at("a section before \\data\\");
            if (n < 1 || n > MAX_ORDER || want[n] == 0) return at("section " + l + " was not announced in \\data\\");
            if (n != (section == 0 ? 1 : section + 1)) return at("section " + l + " is out of order");
            section = (int)n;
            continue;
        }
        if (section < 0) continue;              // a preamble before \data\ is allowed
        if (section == 0) {
            if (l.compare(0, 6, "ngram ") != 0) return at("expected `ngram N=count`");
            char *e = nullptr;
            const long n = strtol(l.c_str() + 6, &e, 10);
            if (e == l.c_str() + 6 || *e != '=') return at("expected `ngram N=count`");
            char *e2 = nullptr;
            const long long c = strtoll(e + 1, &e2, 10);
            if (e2 == e + 1 || *e2 || c < 0) return at("expected `ngram N=count`");
            if (n < 1 || n > MAX_ORDER) return at("order " + std::to_string(n) + " outside 1 .. " + std::to_string(MAX_ORDER));
            if (c > (1ll << 24)) return at("more than 2^24 n-grams");
            want[n] = c;
            if (c > 0 && (int)n > out.order) out.order = (int)n;
            continue;
        }
        std::vector<std::string> f;
        for (size_t p = 0; p < l.size();) {
            while (p < l.size() && (l[p] == ' ' || l[p] == '\t')) p++;
            size_t q = p;
            while (q < l.size() && l[q] != ' ' && l[q] != '\t') q++;
            if (q > p) f.push_back(l.substr(p, q - p));
            p = q;
        }
        const int n = section;
        if ((int)f.size() != n + 1 && (int)f.size() != n + 2) return at("a " + std::to_string(n) + "-gram line has a value, " + std::to_string(n) + " words and at most a back-off");
        float lp10 = 0.0f, bo10 = 0.0f;
        if (!number(f[0], lp10)) return at("malformed log-probability \"" + f[0] + "\"");
        if ((int)f.size() == n + 2 && !number(f[(size_t)n + 1], bo10)) return at("malformed back-off \"" + f[(size_t)n + 1] + "\"");
        if (lp10 > 0.0f) return at("a log-probability above 0");
        seen[n]++;
        bool unk = false;
        for (int j = 1; j <= n; j++) unk = unk || f[(size_t)j] == "<unk>";
        if (unk) {
            if (n == 1) { out.has_unk = true; out.unk_logprob = (float)((double)lp10 * LN10); }
            else out.skipped_unk++;
            continue;
        }
        for (int j = 1; j <= n; j++) {
            int32_t id = 0;
            std::string why;
            if (!word_id(f[(size_t)j], v, id, why)) return at(why);
            if (id == BOS && j != 1) return at("<s> inside an n-gram");
            if (id == EOS && j != n) return at("</s> before the end of an n-gram");
            out.tokens.push_back(id);
        }
        out.lengths.push_back(n);
        out.logprob.push_back((float)((double)lp10 * LN10));
        out.backoff.push_back((float)((double)bo10 * LN10));
    }
    if (section < 0) return "line " + std::to_string(line) + ": no \\data\\ section";
    if (!ended) { line++; return at("no \\end\\"); }
    if (out.order == 0) return at("no n-grams announced");
    for (int n = 1; n <= out.order; n++)
        if (seen[n] != want[n]) return at("the " + std::to_string(n) + "-gram section has " + std::to_string(seen[n]) + " entries, \\data\\ announced " + std::to_string(want[n]));
    return "";
}

// "" or the error ("cannot read ..." or "line N: ...")
inline std::string parse_file(const char *path, const std::vector<std::string> &pieces, Model &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return std::string("cannot read '") + path + "'";
    std::string content;
    char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) content.append(buf, n);
    fclose(f);
    return parse(content, boost_phrases::Vocab(pieces), out);
}

}  // namespace lm_arpa
