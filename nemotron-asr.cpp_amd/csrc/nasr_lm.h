// nasr_lm.h -- the back-off n-gram language model of the beam search's shallow fusion (nasr_engine_set_lm; the fused rules are in
// nasr_beam.h): the builder, the compiled tables and the lookup.  Pure code without HIP, like nasr_beam.h / nasr_boost.h: the CPU suite
// compiles it with g++ under sanitizers (tests/test_lm_math.py), kernels_beam.hip runs the same lookup on the device and the engine runs it
// on the host when it reads a hypothesis' per-token values out.
//
// The model is over the transducer's own token ids: tokens 0 .. 1023, BOS = 1025 only as the first token of an n-gram, EOS = 1026 only as
// the last, 1024 (blank) never.  Order 1 .. 5.  An n-gram has tokens (oldest first), logprob (natural log, finite, <= 0) and backoff
// (natural log, finite, any sign).  unk_logprob (finite, <= 0) is the unigram value of every token and of EOS without a unigram of its own.
//
// Semantics (ARPA back-off): P(w | ctx) = p(ctx w) if that n-gram is in the set, else backoff(ctx) * P(w | ctx without its oldest token);
// backoff = 1 for a context that is not in the set; at the empty context the dense unigram.
//
// Compiled form:
//   states[]   one per n-gram of length < order plus state 0 = the empty context: {f32 backoff, i32 state of the longest proper suffix that
//              is in the set}
//   uni[1027]  {f32 lp, i32 next}: the unigram of every id (own value or unk_logprob) and the state it leads to
//   arcs[]     open addressing, capacity a power of two >= 2 * arcs, linear probing from mix(state * 2048 + token): {u64 key, f32 lp,
//              i32 next} for every n-gram of length >= 2, as an arc from its context's state; next = the state of the longest suffix of
//              context + token, of length <= order - 1, that is in the set.  An empty entry has key EMPTY
//   max_probe  the longest probe sequence the builder produced: no lookup probes more slots than that per level
// lookup walks from the state down its back-off chain: a missing arc adds the state's backoff and moves to its back-off state; at state 0
// the unigram ends the walk.  A state of depth d has a chain of at most d states, d <= order - 1, so `order` levels suffice.  The result is
// the DOUBLE sum of the f32 values in the order met: the backoffs passed, then the arc's (or unigram's) lp.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <map>
#include <string>
#include <vector>
#include "nasr_logprob.h"

namespace nasr_lm {

constexpr int MAX_ORDER = 5, N_TOKENS = 1024, BLANK_ID = 1024, BOS = 1025, EOS = 1026, UNI = 1027;
constexpr long long MAX_NGRAMS = 1ll << 24;
constexpr unsigned long long EMPTY = ~0ull;

struct State { float backoff; int32_t back; };
struct Uni { float lp; int32_t next; };
struct Arc { unsigned long long key; float lp; int32_t next; };
static_assert(sizeof(Arc) == 16 && sizeof(State) == 8 && sizeof(Uni) == 8, "table entries are read as 16 / 8 byte loads");

// what a lookup needs: pointers into host or device memory and the stored loop bounds
struct View {
    const State *states; const Uni *uni; const Arc *arcs;
    unsigned long long mask;            // capacity - 1
    int32_t order, max_probe, n_states, start;
    int32_t has_eos, all_nonpositive;
};

NASR_LP_HD unsigned long long arc_key(int state, int token) { return (unsigned long long)state * 2048ull + (unsigned long long)token; }
NASR_LP_HD unsigned long long mix(unsigned long long x) {      // splitmix64's finalizer
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// ln P(token | state) and the state after it.  token in 0 .. 1023 or EOS; anything else is read as an id without n-grams of its own
NASR_LP_HD double lookup(const View &lm, int state, int token, int32_t *next) {
    if ((unsigned)token >= (unsigned)UNI) token = BLANK_ID;
    if ((unsigned)state >= (unsigned)lm.n_states) state = 0;
    double acc = 0.0;
    for (int level = 0; level < lm.order && state != 0; level++) {
        const unsigned long long key = arc_key(state, token);
        unsigned long long at = mix(key) & lm.mask;
        for (int p = 0; p < lm.max_probe; p++) {
            const Arc a = lm.arcs[at];
            if (a.key == key) { *next = a.next; return acc + (double)a.lp; }
            if (a.key == EMPTY) break;
            at = (at + 1) & lm.mask;
        }
        const State s = lm.states[state];
        acc += (double)s.backoff;
        state = s.back;
    }
    const Uni u = lm.uni[token];
    *next = u.next;
    return acc + (double)u.lp;
}

// ---- shallow fusion in the greedy decode (engine option "lm_fusion") --------------------------------------------------------
// A stream carries one lookup state; the arg-max key of vocabulary entry v gets lmbias(v) = (float)(weight * lookup(state, v) + token_bonus),
// blank and the padding columns get 0, and so does every entry when no model is attached or the stream is switched off.  The state moves to
// the lookup's `next` when a symbol is committed.  The decode kernels read the view and the weights through one fixed block of device memory,
// so a change of model or weights rewrites the block and leaves captured graphs as they are.
constexpr int32_t STATE_DISABLED = -1;              // nasr_stream_set_lm(s, 0) / NASR_FLAG_NO_LM: no bias, and the state never moves
constexpr int ROW_COLS = 1040;                      // the joint kernels' padded vocabulary: a lane's four entries are one aligned 16-byte load
struct Greedy {
    View lm;
    float weight, token_bonus;
    int32_t attached, pad;                          // 0: no model (lm is all zero)
};
// the state of an empty history
NASR_LP_HD int32_t greedy_start(const Greedy &g, bool enabled) { return !enabled ? STATE_DISABLED : g.attached ? g.lm.start : 0; }
// weight * lp + token_bonus in double, product and sum rounded on their own (no fused multiply-add, like nasr_beam::fused_total), then to f32
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
NASR_LP_HD float greedy_bias_value(float weight, double lp, float token_bonus) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = (double)weight * lp;
    return (float)(a + (double)token_bonus);
}
// lmbias(v) of a stream in `state`, v in 0 .. ROW_COLS - 1, and the state after emitting v (the state itself where v gets no bias)
NASR_LP_HD float lmbias(const Greedy &g, int32_t state, int v, int32_t *next) {
    *next = state;
    if (!g.attached || state < 0 || (unsigned)v >= (unsigned)N_TOKENS) return 0.0f;
    const double lp = lookup(g.lm, state, v, next);
    return greedy_bias_value(g.weight, lp, g.token_bonus);
}

// ---- host: the builder ---------------------------------------------------------------------------------------------------------------
struct Model {
    std::vector<State> states;
    std::vector<Uni> uni;
    std::vector<Arc> arcs;
    int order = 0, max_probe = 0, start = 0;
    bool has_eos = false, all_nonpositive = true;
    long long n_ngrams = 0, n_arcs = 0;
    View view() const {
        View v;
        v.states = states.data(); v.uni = uni.data(); v.arcs = arcs.data(); v.mask = arcs.size() - 1;
        v.order = order; v.max_probe = max_probe; v.n_states = (int32_t)states.size(); v.start = start;
        v.has_eos = has_eos ? 1 : 0; v.all_nonpositive = all_nonpositive ? 1 : 0;
        return v;
    }
};

inline std::string ngram_text(const int32_t *tok, int len) {
    std::string s = "(";
    for (int i = 0; i < len; i++) { s += (i ? " " : ""); s += std::to_string(tok[i]); }
    return s + ")";
}

// Builds `out` from n n-grams (lengths[i] tokens each, concatenated in `tokens`; backoff may be null = all 0).  The table's capacity is
// the smallest power of two >= max(2 * arcs, 1), or >= arcs + 1 when `tight` (the tests' way to long probe sequences that wrap around the
// table's end).  Returns 0, or -1 with a message that names the offending n-gram; `out` is then unspecified
inline int build(int order, long long n, const int32_t *lengths, const int32_t *tokens, const float *logprob, const float *backoff, float unk_logprob,
                 Model &out, std::string &err, bool tight = false) {
    char buf[160];
    if (order < 1 || order > MAX_ORDER) { snprintf(buf, sizeof buf, "order %d outside 1 .. %d", order, MAX_ORDER); err = buf; return -1; }
    if (n < 0 || n > MAX_NGRAMS) { snprintf(buf, sizeof buf, "%lld n-grams, more than %lld", n, MAX_NGRAMS); err = buf; return -1; }
    if (!(isfinite(unk_logprob) && unk_logprob <= 0.0f)) { err = "unk_logprob must be finite and <= 0"; return -1; }
    if (n > 0 && (!lengths || !tokens || !logprob)) { err = "null n-gram arrays"; return -1; }
    typedef std::vector<int32_t> Seq;
    std::map<Seq, long long> index;                 // n-gram -> its number
    std::vector<long long> first((size_t)n + 1, 0);
    for (long long i = 0; i < n; i++) {
        const int len = lengths[i];
        if (len < 1 || len > order) { snprintf(buf, sizeof buf, "n-gram %lld has length %d outside 1 .. order = %d", i, len, order); err = buf; return -1; }
        first[(size_t)i + 1] = first[(size_t)i] + len;
    }
    out = Model();
    out.order = order; out.n_ngrams = n;
    for (long long i = 0; i < n; i++) {
        const int len = lengths[i];
        const int32_t *tk = tokens + first[(size_t)i];
        const std::string name = "n-gram " + std::to_string(i) + " " + ngram_text(tk, len);
        for (int j = 0; j < len; j++) {
            const bool ok = (tk[j] >= 0 && tk[j] < N_TOKENS) || (tk[j] == BOS && j == 0) || (tk[j] == EOS && j == len - 1);
            if (!ok) { err = name + ": id " + std::to_string(tk[j]) + " out of place at position " + std::to_string(j); return -1; }
        }
        const float bo = backoff ? backoff[i] : 0.0f;
        if (!(isfinite(logprob[i]) && logprob[i] <= 0.0f)) { err = name + ": logprob must be finite and <= 0"; return -1; }
        if (!isfinite(bo)) { err = name + ": backoff must be finite"; return -1; }
        if (!index.emplace(Seq(tk, tk + len), i).second) { err = name + ": duplicate n-gram"; return -1; }
        if (bo > 0.0f) out.all_nonpositive = false;
        if (tk[len - 1] == EOS) out.has_eos = true;
    }
    // states: the empty context, then every n-gram shorter than the order, in input order
    std::vector<int32_t> state_of((size_t)n, 0);    // 0: not a state
    out.states.push_back(State{0.0f, 0});
    for (long long i = 0; i < n; i++) {
        const int len = lengths[i];
        const int32_t *tk = tokens + first[(size_t)i];
        if (len > 1 && !index.count(Seq(tk, tk + len - 1))) {
            err = "n-gram " + std::to_string(i) + " " + ngram_text(tk, len) + ": its context " + ngram_text(tk, len - 1) + " is not an n-gram of the set";
            return -1;
        }
        if (len < order) {
            state_of[(size_t)i] = (int32_t)out.states.size();
            out.states.push_back(State{backoff ? backoff[i] : 0.0f, 0});
        }
    }
    // the state of the longest suffix of seq[from ..] of length <= order - 1 that is a state (0 if none)
    auto suffix_state = [&](const int32_t *seq, int len, int from) {
        for (int s = std::max(from, len - (order - 1)); s < len; s++) {
            auto it = index.find(Seq(seq + s, seq + len));
            if (it != index.end() && state_of[(size_t)it->second]) return state_of[(size_t)it->second];
        }
        return (int32_t)0;
    };
    out.uni.assign((size_t)UNI, Uni{unk_logprob, 0});
    long long n_arcs = 0;
    for (long long i = 0; i < n; i++) {
        const int len = lengths[i];
        const int32_t *tk = tokens + first[(size_t)i];
        if (state_of[(size_t)i]) out.states[(size_t)state_of[(size_t)i]].back = suffix_state(tk, len, 1);
        if (len == 1) out.uni[(size_t)tk[0]] = Uni{logprob[i], state_of[(size_t)i]};
        else n_arcs++;
    }
    out.n_arcs = n_arcs;
    size_t cap = 1;
    while ((long long)cap < (tight ? n_arcs + 1 : 2 * n_arcs)) cap <<= 1;
    out.arcs.assign(cap, Arc{EMPTY, 0.0f, 0});
    for (long long i = 0; i < n; i++) {
        const int len = lengths[i];
        if (len == 1) continue;
        const int32_t *tk = tokens + first[(size_t)i];
        const int32_t ctx = state_of[(size_t)index[Seq(tk, tk + len - 1)]];
        Arc a;
        a.key = arc_key(ctx, tk[len - 1]); a.lp = logprob[i];
        a.next = suffix_state(tk, len, 0);
        size_t at = (size_t)(mix(a.key) & (cap - 1));
        int probes = 1;
        while (out.arcs[at].key != EMPTY) { at = (at + 1) & (cap - 1); probes++; }
        out.arcs[at] = a;
        out.max_probe = std::max(out.max_probe, probes);
    }
    auto bos = index.find(Seq(1, BOS));
    out.start = bos != index.end() ? state_of[(size_t)bos->second] : 0;
    return 0;
}

}  // namespace nasr_lm
