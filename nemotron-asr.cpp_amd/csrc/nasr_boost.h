// nasr_boost.h -- phrase boosting ("hotwords", engine option "phrase_boost") of the device RNN-T greedy decode: the automaton builder, the
// table layout and the lookups the decode kernels run.  Pure code without HIP, compiled by the CPU suite with g++ under sanitizers
// (tests/test_boost_automaton.py), like nasr_logprob.h / nasr_gemm_plan.h; kernels_decode.hip includes it and calls the same functions.
//
// Semantics.  A boost set is a list of phrases; phrase i is 1 .. 32 non-blank token ids p_i with a bonus w_i (finite, 0 < w_i <= 1e4, natural-log
// units).  For a stream whose emitted non-blank history since its last history reset is h,
//   bonus(v) = max { w_i : 0 <= k < len(p_i), p_i[0:k] is a suffix of h, p_i[k] == v }      (0 if there is no such pair; blank never gets one)
// and the decode takes arg-max_v (logit[v] + bonus(v)), first maximum wins.  This is what an Aho-Corasick automaton over the phrases computes:
// the state is the longest suffix of h that is a prefix of some phrase, bonus(v) the maximum over the state's failure chain of the bonuses of
// the trie edges labelled v.  Both are tabulated densely per state, so the kernels do one load and no chain walk:
//   bonus [state][COLS] f32    the bonus of every vocabulary entry in that state (columns 1024 .. 1039: 0)
//   next  [state][COLS] i32    the state after emitting that entry              (columns 1024 .. 1039: the state itself)
// COLS = 1040 = the joint kernels' padded vocabulary (65 tiles of 16), so the four consecutive entries of an MFMA lane are one aligned 16-byte
// load.  State 0 is "boost disabled": all-zero bonus, every transition back to 0, so a disabled stream takes the same code path with no
// branch.  State 1 is the root (empty history).  A state moves only when a symbol is committed (k_dec_commit), exactly like the decoder state.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define NASR_BOOST_HD __host__ __device__ __forceinline__
#else
#define NASR_BOOST_HD inline
#endif

namespace nasr_boost {

constexpr int VOCAB = 1025, BLANK = 1024;
constexpr int COLS = 1040;                          // table row width: the vocabulary padded to 65 tiles of 16
constexpr int MAX_PHRASE_LEN = 32;
constexpr int STATE_OFF = 0, STATE_ROOT = 1;
constexpr int MIN_STATES = 2, MAX_STATES = 4096;    // capacity range of engine option "phrase_boost" (4096 states = 2 x 17 MB of tables)
constexpr float MAX_BONUS = 1.0e4f;

struct alignas(16) Bonus4 { float x, y, z, w; };    // a lane's four consecutive entries

// ---- layout and lookups (host and device) ----------------------------------------------------------------------------------------
NASR_BOOST_HD size_t table_index(int state, int v) { return (size_t)state * COLS + (size_t)v; }
NASR_BOOST_HD size_t table_elems(int states) { return (size_t)(states > 0 ? states : 0) * COLS; }
NASR_BOOST_HD float bonus_of(const float *bonus, int state, int v) { return bonus[table_index(state, v)]; }
NASR_BOOST_HD int next_of(const int32_t *next, int state, int token) { return next[table_index(state, token)]; }
// entries v0 .. v0 + 3 of a state's row, v0 a multiple of 4 below COLS (lane (q) of vocab tile nt: v0 = 16 nt + 4 q, nt < 65)
NASR_BOOST_HD Bonus4 bonus4_of(const float *bonus, int state, int v0) { return *(const Bonus4 *)(bonus + table_index(state, v0)); }
// with "token_logprobs": the joint kernels leave, per softmax part of a row (nasr_logprob.h: 65 parts of 16 entries or 17 of 64), the RAW logit of
// the part's winner by boosted key; the row's winner is the winner of its part, so the commit kernel finds its raw logit in this part
NASR_BOOST_HD int raw_part_of(int token, int n_parts) { return n_parts == 65 ? token >> 4 : token >> 6; }

// ---- the builder (host) -----------------------------------------------------------------------------------------------------------
enum Status { OK = 0, ERR_ARGUMENT = 1, ERR_LENGTH = 2, ERR_TOKEN = 3, ERR_BONUS = 4, ERR_CAPACITY = 5 };
inline const char *status_text(int s) {
    switch (s) {
    case OK: return "ok";
    case ERR_ARGUMENT: return "null or negative argument";
    case ERR_LENGTH: return "a phrase must have 1 .. 32 tokens";
    case ERR_TOKEN: return "a phrase token must be a non-blank vocabulary id (0 .. 1023)";
    case ERR_BONUS: return "a bonus must be finite, > 0 and <= 1e4";
    case ERR_CAPACITY: return "the phrases need more automaton states than the capacity";
    }
    return "?";
}

struct Automaton {
    int n_states = 0;                    // rows of the tables: the disabled state, the root and one per distinct non-empty phrase prefix
    std::vector<float> bonus;            // [n_states][COLS]
    std::vector<int32_t> next;           // [n_states][COLS]
    std::vector<int32_t> depth;          // [n_states] length of the state's prefix (0 for the disabled state and the root)
};

inline int validate(int n_phrases, const int32_t *const *tokens, const int32_t *lens, const float *bonus, int *bad_phrase) {
    if (bad_phrase) *bad_phrase = -1;
    if (n_phrases < 0) return ERR_ARGUMENT;
    if (n_phrases > 0 && (!tokens || !lens || !bonus)) return ERR_ARGUMENT;
    for (int i = 0; i < n_phrases; i++) {
        if (bad_phrase) *bad_phrase = i;
        if (lens[i] < 1 || lens[i] > MAX_PHRASE_LEN) return ERR_LENGTH;
        if (!tokens[i]) return ERR_ARGUMENT;
        for (int k = 0; k < lens[i]; k++)
            if (tokens[i][k] < 0 || tokens[i][k] >= BLANK) return ERR_TOKEN;
        if (!(bonus[i] > 0.0f) || !(bonus[i] <= MAX_BONUS)) return ERR_BONUS;      // NaN fails both comparisons, +inf the second
    }
    if (bad_phrase) *bad_phrase = -1;
    return OK;
}

// phrases in; states, per-state bonus and next state out.  `capacity` = the most states the tables may have (the two fixed ones included).
// On any error `out` is left untouched.
inline int build(int n_phrases, const int32_t *const *tokens, const int32_t *lens, const float *bonus, int capacity, Automaton &out, int *bad_phrase = nullptr) {
    const int rc = validate(n_phrases, tokens, lens, bonus, bad_phrase);
    if (rc) return rc;
    if (capacity < MIN_STATES) return ERR_CAPACITY;
    Automaton a;
    auto add_state = [&](int depth) {
        a.bonus.resize(a.bonus.size() + COLS, 0.0f);
        a.next.resize(a.next.size() + COLS, -1);
        a.depth.push_back(depth);
        return a.n_states++;
    };
    add_state(0);                                                  // STATE_OFF
    add_state(0);                                                  // STATE_ROOT
    // the trie: next = child or -1, bonus = the largest bonus among the phrases that run through the edge
    for (int i = 0; i < n_phrases; i++) {
        int s = STATE_ROOT;
        for (int k = 0; k < lens[i]; k++) {
            const size_t at = table_index(s, tokens[i][k]);
            int c = a.next[at];
            if (c < 0) {
                if (a.n_states >= capacity) { if (bad_phrase) *bad_phrase = i; return ERR_CAPACITY; }
                c = add_state(k + 1);
                a.next[at] = c;
            }
            a.bonus[at] = fmaxf(a.bonus[at], bonus[i]);
            s = c;
        }
    }
    // breadth first: a state's failure state is shallower, so its row is complete when the state is reached
    std::vector<int32_t> fail((size_t)a.n_states, STATE_ROOT), queue;
    queue.reserve((size_t)a.n_states);
    for (int v = 0; v < BLANK; v++) {
        int32_t &c = a.next[table_index(STATE_ROOT, v)];
        if (c < 0) c = STATE_ROOT; else queue.push_back(c);
    }
    for (size_t head = 0; head < queue.size(); head++) {
        const int s = queue[head], f = fail[(size_t)s];
        for (int v = 0; v < BLANK; v++) {
            const size_t at = table_index(s, v), fat = table_index(f, v);
            if (a.next[at] < 0) a.next[at] = a.next[fat];
            else { fail[(size_t)a.next[at]] = a.next[fat]; queue.push_back(a.next[at]); }
            a.bonus[at] = fmaxf(a.bonus[at], a.bonus[fat]);
        }
    }
    for (int s = 0; s < a.n_states; s++) {
        for (int v = BLANK; v < COLS; v++) a.next[table_index(s, v)] = s;           // blank and the padding: never emitted, never boosted
        if (s == STATE_OFF) for (int v = 0; v < BLANK; v++) a.next[table_index(s, v)] = STATE_OFF;
    }
    out = std::move(a);
    return OK;
}

}  // namespace nasr_boost
