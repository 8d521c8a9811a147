// boost_phrases.h -- text phrases -> token ids for phrase boosting (engine option "phrase_boost", nasr_engine_set_boost_phrases), pure host
// code so that the CPU suite compiles it under sanitizers (tests/test_boost_phrases_host.py), like word_confidence.h.
// The GGUF carries the vocabulary's pieces but no SentencePiece scores, so a phrase cannot be encoded the way the tokenizer would.  Instead
// each whitespace-separated word is segmented by GREEDY LONGEST MATCH against the pieces, starting from its U+2581-prefixed form (the form a
// word has at its start, where tokens_to_text puts a space): at every position the longest piece that matches is taken.  For a word the
// model spells another way the phrase simply never matches; write such a phrase as literal ids, `ids:12,55,9`.  A phrase that cannot be
// covered (a character no piece has), that is empty or that needs more than 32 tokens is reported by line number and skipped.
// A boost file holds one phrase per line, `phrase<TAB>bonus`; the bonus (natural-log units, 0 < bonus <= 1e4) is optional, lines that are
// empty or start with '#' are skipped.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <vector>

namespace boost_phrases {

constexpr float DEFAULT_BONUS = 4.0f;     // used when neither the line nor the caller gives one: e^4 ~ 55 x the token's odds
constexpr int MAX_TOKENS = 32, N_TOKEN_IDS = 1024;      // limits of nasr_engine_set_boost_phrases: phrase length, non-blank ids
constexpr float MAX_BONUS = 1.0e4f;

struct Phrase {
    std::vector<int32_t> tokens;
    float bonus;
    int line;                // 1-based line (or list position) it came from
};
struct Result {
    std::vector<Phrase> phrases;
    std::vector<std::string> problems;       // "line 3: ..." for every phrase that was skipped
};

struct Vocab {
    std::unordered_map<std::string, int32_t> id;      // piece -> lowest id that spells it
    size_t longest = 0;                               // bytes of the longest piece
    explicit Vocab(const std::vector<std::string> &pieces) {
        for (size_t i = 0; i < pieces.size() && i < (size_t)N_TOKEN_IDS; i++) {
            if (pieces[i].empty()) continue;
            if (id.emplace(pieces[i], (int32_t)i).second && pieces[i].size() > longest) longest = pieces[i].size();
        }
    }
};

// appends the pieces of `word` (no whitespace inside) to out; false if some position has no matching piece (out is then left as it was)
inline bool segment_word(const std::string &word, const Vocab &v, std::vector<int32_t> &out) {
    const std::string s = "\xe2\x96\x81" + word;
    const size_t n0 = out.size();
    for (size_t pos = 0; pos < s.size();) {
        size_t len = std::min(v.longest, s.size() - pos);
        for (; len > 0; len--) {
            const auto it = v.id.find(s.substr(pos, len));
            if (it != v.id.end()) { out.push_back(it->second); break; }
        }
        if (len == 0) { out.resize(n0); return false; }
        pos += len;
    }
    return true;
}

// one phrase: `ids:a,b,c` literally, otherwise word by word.  Returns "" or what is wrong with it.
inline std::string phrase_tokens(const std::string &text, const Vocab &v, std::vector<int32_t> &out) {
    out.clear();
    if (text.compare(0, 4, "ids:") == 0) {
        const char *p = text.c_str() + 4;
        while (*p) {
            char *end = nullptr;
            const long id = strtol(p, &end, 10);
            if (end == p) return "malformed id list (want ids:12,55,9)";
            if (id < 0 || id >= N_TOKEN_IDS) return "token id " + std::to_string(id) + " is not a non-blank vocabulary id (0 .. 1023)";
            out.push_back((int32_t)id);
            p = end;
            while (*p == ' ') p++;
            if (*p == ',') { p++; if (!*p) return "malformed id list (want ids:12,55,9)"; }
            else if (*p) return "malformed id list (want ids:12,55,9)";
        }
    } else {
        size_t pos = 0;
        while (pos < text.size()) {
            while (pos < text.size() && (text[pos] == ' ' || text[pos] == '\t')) pos++;
            size_t end = pos;
            while (end < text.size() && text[end] != ' ' && text[end] != '\t') end++;
            if (end > pos && !segment_word(text.substr(pos, end - pos), v, out))
                return "the vocabulary's pieces cannot spell \"" + text.substr(pos, end - pos) + "\"";
            pos = end;
        }
    }
    if (out.empty()) return "empty phrase";
    if ((int)out.size() > MAX_TOKENS) return "the phrase needs " + std::to_string(out.size()) + " tokens, more than 32";
    return "";
}

inline bool valid_bonus(float b) { return b > 0.0f && b <= MAX_BONUS; }      // false for NaN

// phrases given one by one (bonus[i], or default_bonus where the list is shorter); `line` = position in the list
inline Result from_list(const std::vector<std::string> &texts, const std::vector<float> &bonus, const std::vector<std::string> &pieces, float default_bonus = DEFAULT_BONUS) {
    Result r;
    const Vocab v(pieces);
    for (size_t i = 0; i < texts.size(); i++) {
        Phrase p;
        p.line = (int)i + 1;
        p.bonus = i < bonus.size() ? bonus[i] : default_bonus;
        const std::string why = valid_bonus(p.bonus) ? phrase_tokens(texts[i], v, p.tokens) : "the bonus must be finite, > 0 and <= 1e4";
        if (why.empty()) r.phrases.push_back(p);
        else r.problems.push_back("line " + std::to_string(p.line) + ": " + why);
    }
    return r;
}

// the content of a boost file
inline Result parse(const std::string &content, const std::vector<std::string> &pieces, float default_bonus = DEFAULT_BONUS) {
    Result r;
    const Vocab v(pieces);
    int line = 0;
    for (size_t pos = 0; pos < content.size();) {
        size_t end = content.find('\n', pos);
        if (end == std::string::npos) end = content.size();
        std::string l = content.substr(pos, end - pos);
        pos = end + 1;
        line++;
        while (!l.empty() && (l.back() == '\r' || l.back() == ' ' || l.back() == '\t')) l.pop_back();
        if (l.empty() || l[0] == '#') continue;
        Phrase p;
        p.line = line;
        p.bonus = default_bonus;
        std::string why;
        const size_t tab = l.find('\t');
        if (tab != std::string::npos) {
            const std::string b = l.substr(tab + 1);
            char *e = nullptr;
            p.bonus = strtof(b.c_str(), &e);
            while (e && (*e == ' ' || *e == '\t')) e++;
            if (e == b.c_str() || (e && *e)) why = "malformed bonus \"" + b + "\"";
            l.resize(tab);
        }
        if (why.empty() && !valid_bonus(p.bonus)) why = "the bonus must be finite, > 0 and <= 1e4";
        if (why.empty()) why = phrase_tokens(l, v, p.tokens);
        if (why.empty()) r.phrases.push_back(p);
        else r.problems.push_back("line " + std::to_string(line) + ": " + why);
    }
    return r;
}

// false if the file cannot be read
inline bool parse_file(const char *path, const std::vector<std::string> &pieces, float default_bonus, Result &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    std::string content;
    char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) content.append(buf, n);
    fclose(f);
    out = parse(content, pieces, default_bonus);
    return true;
}

}  // namespace boost_phrases
