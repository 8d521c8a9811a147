// nasr_beam.h -- the rules of the frame-synchronous beam search of the offline path (nasr_engine_transcribe_beam*): ordering and ties,
// insertion into C with merge and keep-W, selection of A from D with the optional prune, the trie of emitted tokens, slot binding, the
// final N-best and its backtrace.  Pure code without HIP so that the CPU suite compiles it with g++ under sanitizers
// (tests/test_beam_math.py), like nasr_align.h / nasr_topk.h; kernels_beam.hip includes it and runs the same functions on the device.
//
// Parameters: beam W in 1 .. 8, nbest N in 1 .. W, max_symbols S in 1 .. 10 (0 in the parameter struct = S_DEFAULT).
// A hypothesis is a token sequence y, the frame at which each token was emitted, a score, and the prediction-network state after
// blank, y_0 .. y_{|y|-1} from the zero state (alignment's teacher-forced state).  The score is a DOUBLE sum of f32 ln-softmax values over
// the joint's 1025 outputs (blank included): lb(t, h) = ln P(blank), ly(t, h, k) = ln P(k) at frame t with h's state.
//
//   Beam_0 = { (y = (), score 0, fresh state) }
//   for t = 0 .. T-1:
//       A = Beam_t (ordered best first);  C = {}
//       for v = 0 .. S:
//           every h in A, in order, arrives in C with (h.y, h.score + lb(t, h));  C keeps its W best
//           if v == S: stop
//           D = { (h.y + k, h.score + ly(t, h, k)) : h in A, k in expand(h) }
//           A = the W best of D, in order, each with the state after its token
//       Beam_{t+1} = C
//   result = the N best of Beam_T
//
// Expansion: the row's 8 largest joint outputs in the alternatives' order (nasr_topk.h: descending logit, lower id first among equal bits);
// blank is dropped and the first W of the rest are kept -- exactly W tokens for W <= 7, 7 or 8 for W = 8.
// Merging: two arrivals in C with the same token sequence are one hypothesis; the higher score stays, with that path's frames, and a later
// arrival replaces an earlier one only when strictly greater.  A score is therefore always the score of ONE lattice path (the final blank of
// every frame included): no sums over paths.  Sequence identity is exact: the parent chains are compared token by token; the hash only
// pre-filters.
// Ordering: better = the higher score; among equal scores the earlier arrival wins (lower round, then lower position of the hypothesis /
// parent in A, then earlier in the parent's expansion list) -- every list below is filled in arrival order and an entry is placed behind
// the entries whose score is not lower.
// Prune (optional): once C is full a child of D whose score does not exceed C's W-th best is dropped at once.  ln P <= 0, so nothing that
// descends from it could enter C or replace an entry of it, and the dropped children are a suffix of D's order: results do not change.
//
// Beam 1 is NOT the greedy decode: greedy emits the arg-max whenever it is not blank, while this search keeps, per frame, the single best of
// "blank now" over all symbol counts -- it may drop a token whose continuation scores below the blank (4 of 16 cases differed on the
// alignment tests' checkpoint).  Phrase boosting is applied only in calls that ask for it (the BOOST forms below); either way the scores are
// the model's probabilities, as in alignment.
// T == 0 gives one hypothesis: empty, score 0.
//
// Trie: every child selected into A is a node (parent, token, frame, ln P).  At most W nodes per round with v < S, so an utterance of T
// frames needs at most T * S * W nodes (node_bound); a sub-batch's pool is the sum.
// Slots: a hypothesis owns one decoder slot (committed LSTM state, candidate, g).  A hypothesis parked in C keeps its slot while A's slots are
// reused, so an utterance has 3 W slots: <= W in C, <= W in A, <= W for A's children.
//
// Shallow fusion with a back-off n-gram language model over the token ids (nasr_lm.h; nasr_engine_set_lm), the LM forms below.
// A hypothesis also carries lm = the DOUBLE sum of its tokens' nasr_lm::lookup results in token order, and lm_state.  A child of h with
// token k has score = h.score + ly as above, lm = h.lm + lookup(h.lm_state, k), lm_state = that lookup's next state.  Everywhere a score is
// compared above -- insert_sorted_t, c_arrive_t's strictly-greater test, the selection of A from D, the prune's floor -- the key is
//     total = score + (double)weight * lm + (double)token_bonus * len
// evaluated as exactly that expression in double from the running sums (no fused multiply-add).  score keeps its meaning: the model's
// probability of one lattice path.  Two arrivals of the same sequence have the same lm and len, so the merge rule is unchanged in effect.
// The expansion list is unchanged: the LM re-scores the candidates, it does not propose them.  weight and token_bonus are finite in
// [0, 100].  With weight 0 and bonus 0, total == score bit for bit.
// The prune's proof needs every increment of the key to be <= 0: ln P <= 0 always, weight * (an LM term) <= 0 only when every logprob and
// every backoff of the model is <= 0 (nasr_lm's all_nonpositive), and token_bonus * 1 <= 0 only when token_bonus == 0.  So the prune is
// applied only when token_bonus == 0 and all_nonpositive; otherwise the search runs unpruned (prune_allowed).
// At the end, if some n-gram ends in EOS, every hypothesis of Beam_T gets lm_final = lm + lookup(lm_state, EOS) (else lm_final = lm) and the N
// best are taken by score + weight * lm_final + token_bonus * len, stable on ties (Beam_T's order): final_rank_t.
//
// Phrase boosting (engine option "phrase_boost", call flag NASR_FLAG_BEAM_BOOST; nasr_boost.h defines the set, the automaton and bonus_of), the
// BOOST forms below, with or without the LM.  A hypothesis also carries boost_state = the automaton state after its tokens from STATE_ROOT
// (blank never moves it) and boost = the DOUBLE sum of bonus_of(state before y_i, y_i) over its tokens.
// Proposal: a hypothesis in state s expands from its row's 8 largest keys pack_key(logit[v] + bonus(s, v), v) -- the f32 sum the greedy BOOST
// kernels form -- descending, the lower id first among equal bits; blank is dropped and the first W of the rest are kept.  So a boosted token
// outside the raw 8 largest outputs can be proposed.  The ln P of an entry stays the MODEL's: lp_of(raw logit, m, log s), never
// (logit + bonus) - bonus.
// Ranking: everywhere a key is compared (insert_sorted_t, c_arrive_t, the selection of A from D, the prune's floor, final_rank_t) the key is
//     fused_total(score, weight, lm, token_bonus, len) + boost            (score + boost without an LM)
// with boost added last as its own rounded double add.  score, the per-token ln P and the frames keep their meaning: one lattice path of the
// model.  Two arrivals of the same sequence have equal boost, so the merge rule is unchanged.
// Prune: a positive bonus is a positive increment of the key, so a boosted call with a non-empty set (more than the 2 fixed automaton
// states) runs unpruned (prune_allowed).  With the empty set every bonus is 0 and boost stays 0.0: every key, list and result is that of the
// call without boosting.
// No retraction: a partial match that later fails keeps the bonus it was paid -- the greedy definition; the tables hold a max over the failure
// chain, so "paid so far" is not a function of the state.
#pragma once
#include "nasr_topk.h"
#include "nasr_lm.h"
#include "nasr_boost.h"

namespace nasr_beam {

constexpr int WMAX = 8, SMAX = 10, S_DEFAULT = 4, KTOP = nasr_topk::KMAX, BLANK_ID = nasr_lp::LP_VOCAB - 1;
constexpr int SLOTS_PER_W = 3;
static_assert(KTOP == 8, "the expansion reads the alternatives' 8 keys");

struct Node { int32_t parent, token, frame; float lp; };                  // parent = -1: the root (empty sequence)
struct Hyp {
    double score;
    unsigned long long hash;            // of the token sequence: a pre-filter for same_seq
    int32_t node, len;                  // last trie node (-1: empty), tokens
    int32_t slot, lm_state;             // decoder slot within the utterance, 0 .. 3 W - 1; LM state after the sequence (0 without an LM)
    double lm;                          // sum of the tokens' LM terms (0 without an LM)
    double boost;                       // sum of the tokens' phrase bonuses (0 without boosting)
    int32_t boost_state;                // automaton state after the sequence (STATE_ROOT without boosting)
};
struct Beam {                           // the search state of one utterance
    Hyp a[WMAX], c[WMAX];
    int32_t na, nc;
    int32_t t, v;                       // frame, round within the frame
    int32_t n_nodes, T;
};
struct Child { int32_t parent_slot, slot, token, pad; };                  // a new entry of A: gather the parent's candidate state into `slot`

NASR_LP_HD bool valid_params(int W, int N, int S) { return W >= 1 && W <= WMAX && N >= 1 && N <= W && S >= 1 && S <= SMAX; }
NASR_LP_HD long long node_bound(int T, int W, int S) { return (long long)T * S * W; }
NASR_LP_HD int n_slots(int W) { return SLOTS_PER_W * W; }
NASR_LP_HD long long rounds(int T, int S) { return (long long)T * (S + 1); }

NASR_LP_HD unsigned long long hash0() { return 0xcbf29ce484222325ull; }
NASR_LP_HD unsigned long long hash_next(unsigned long long h, int token) { return (h ^ (unsigned long long)(token + 1)) * 0x100000001b3ull; }

// exact equality of two token sequences given by their last nodes: equal lengths, then the chains token by token until they meet
NASR_LP_HD bool same_seq(const Node *nodes, int a, int a_len, int b, int b_len) {
    if (a_len != b_len) return false;
    for (int i = 0; i < a_len && a != b; i++) {
        if (nodes[a].token != nodes[b].token) return false;
        a = nodes[a].parent; b = nodes[b].parent;
    }
    return true;
}

// score + weight * lm + token_bonus * len, each product and sum rounded on its own: no fused multiply-add, so host and device agree bit for bit
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))                // g++ contracts by default where the target has fused multiply-add
#endif
NASR_LP_HD double fused_total(double score, float weight, double lm, float token_bonus, int len) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = (double)weight * lm;
    const double b = (double)token_bonus * (double)len;
    return score + a + b;
}
// key + boost as one rounded double add of its own
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
NASR_LP_HD double boosted_total(double key, double boost) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return key + boost;
}
// the ordering key.  LM = false: the score itself.  BOOST: + boost, added last
template <bool LM, bool BOOST = false>
NASR_LP_HD double total_of(const Hyp &h, float weight, float token_bonus) {
    const double key = LM ? fused_total(h.score, weight, h.lm, token_bonus, h.len) : h.score;
    return BOOST ? boosted_total(key, h.boost) : key;
}
NASR_LP_HD bool valid_weights(float weight, float token_bonus) {
    return weight >= 0.0f && weight <= 100.0f && token_bonus >= 0.0f && token_bonus <= 100.0f;       // false for NaN
}
NASR_LP_HD bool prune_allowed(float token_bonus, bool all_nonpositive) { return token_bonus == 0.0f && all_nonpositive; }
// a boosted call: also only with the empty set (boost_states = the automaton's states, 2 = the disabled state and the root alone).  Without an LM
// pass token_bonus 0 and all_nonpositive true
NASR_LP_HD bool prune_allowed(float token_bonus, bool all_nonpositive, int boost_states) {
    return prune_allowed(token_bonus, all_nonpositive) && boost_states <= nasr_boost::MIN_STATES;
}

// dst = src field by field: on the device a whole-struct copy of these bytes may go through scratch memory, which the select kernel keeps clear of.
// Without BOOST the two boost fields are neither read nor written
template <bool BOOST = false>
NASR_LP_HD void copy_hyp(Hyp &dst, const Hyp &src) {
    dst.score = src.score; dst.hash = src.hash; dst.node = src.node; dst.len = src.len; dst.slot = src.slot; dst.lm_state = src.lm_state; dst.lm = src.lm;
    if (BOOST) { dst.boost = src.boost; dst.boost_state = src.boost_state; }
}

// place h behind the entries of list[0 .. n) whose key is not lower; the list keeps at most W entries.  Returns false when h fell off
template <bool LM, bool BOOST = false>
NASR_LP_HD bool insert_sorted_t(Hyp *list, int32_t &n, int W, const Hyp &h, float weight, float token_bonus) {
    int pos = n;
    const double key = total_of<LM, BOOST>(h, weight, token_bonus);
    while (pos > 0 && total_of<LM, BOOST>(list[pos - 1], weight, token_bonus) < key) pos--;
    if (pos >= W) return false;
    const int last = n < W ? n : W - 1;
    for (int i = last; i > pos; i--) copy_hyp<BOOST>(list[i], list[i - 1]);
    copy_hyp<BOOST>(list[pos], h);
    if (n < W) n++;
    return true;
}

// an arrival in C: merge with the entry of the same sequence (strictly greater replaces), else insert and keep the W best
template <bool LM, bool BOOST = false>
NASR_LP_HD void c_arrive_t(Beam &b, int W, const Node *nodes, const Hyp &h, float weight, float token_bonus) {
    for (int i = 0; i < b.nc; i++) {
        if (b.c[i].hash != h.hash || !same_seq(nodes, b.c[i].node, b.c[i].len, h.node, h.len)) continue;
        if (!(total_of<LM, BOOST>(h, weight, token_bonus) > total_of<LM, BOOST>(b.c[i], weight, token_bonus))) return;
        for (int j = i; j + 1 < b.nc; j++) copy_hyp<BOOST>(b.c[j], b.c[j + 1]);
        b.nc--;
        break;
    }
    insert_sorted_t<LM, BOOST>(b.c, b.nc, W, h, weight, token_bonus);
}

// the expansion list of a row from its 8 largest keys (sorted descending) and its softmax (m, log s): tokens and their f32 ln P
NASR_LP_HD int expand(const nasr_topk::tkey *top, int W, float m, float log_s, int32_t *tok, float *lp) {
    int n = 0;
    for (int j = 0; j < KTOP && n < W; j++) {
        const int id = nasr_topk::alt_id(top[j]);
        if (top[j] == 0ull || id == BLANK_ID) continue;
        tok[n] = id; lp[n] = nasr_topk::alt_lp(top[j], m, log_s); n++;
    }
    return n;
}

// The boosted expansion.  boosted_top: the row's 8 largest keys pack_key(logit[v] + bonus_row[v], v) over the 1025 outputs, descending (what the
// boosted joint form leaves per row, restated for the host).  expand_ids: the list's tokens from those keys, by expand's rule.  boost_entry:
// what one entry carries -- the MODEL's ln P from the RAW logit, the bonus and the next automaton state from the tables' rows of the state
NASR_LP_HD void boosted_top(const float *raw, const float *bonus_row, nasr_topk::tkey *top) {
    nasr_topk::RowTop rt;
    nasr_topk::row_begin(rt);
    for (int v = 0; v < nasr_lp::LP_VOCAB; v++) {
        const nasr_topk::tkey k = nasr_lp::pack_key(raw[v] + bonus_row[v], v);
        if (k > rt.last) nasr_topk::row_insert(rt, KTOP, k);
    }
    for (int j = 0; j < KTOP; j++) top[j] = rt.top[j];
}
NASR_LP_HD int expand_ids(const nasr_topk::tkey *top, int W, int32_t *tok) {
    int n = 0;
    for (int j = 0; j < KTOP && n < W; j++) {
        const int id = nasr_topk::alt_id(top[j]);
        if (top[j] == 0ull || id == BLANK_ID) continue;
        tok[n++] = id;
    }
    return n;
}
NASR_LP_HD void boost_entry(float raw_logit, float m, float log_s, const float *bonus, const int32_t *next, int state, int token, float *lp, float *bon,
                            int32_t *next_state) {
    *lp = nasr_topk::lp_of(raw_logit, m, log_s);
    *bon = nasr_boost::bonus_of(bonus, state, token);
    *next_state = nasr_boost::next_of(next, state, token);
}
// a row's boosted expansion list from its RAW logits [1025] and the tables: tokens, raw ln P, bonus and next state
NASR_LP_HD int expand_boost(const float *raw, const float *bonus, const int32_t *next, int state, int W, float m, float log_s, int32_t *tok, float *lp,
                            float *bon, int32_t *next_state) {
    nasr_topk::tkey top[KTOP];
    boosted_top(raw, bonus + nasr_boost::table_index(state, 0), top);
    const int n = expand_ids(top, W, tok);
    for (int k = 0; k < n; k++) boost_entry(raw[tok[k]], m, log_s, bonus, next, state, tok[k], lp + k, bon + k, next_state + k);
    return n;
}

// the lowest slot of the utterance's 3 W that is not in `used`
NASR_LP_HD int take_slot(unsigned &used, int W) {
    for (int s = 0; s < n_slots(W); s++)
        if (!(used & (1u << s))) { used |= 1u << s; return s; }
    return -1;
}

// One round of one utterance.  In: lb[i] and the expansion list (ex_n[i] entries of ex_tok / ex_lp [i][KTOP]) of every a[i], evaluated at frame
// b.t.  Out: the beam after the round; children[0 .. return value) = the new entries of A whose state must be gathered (none on the round that
// ends a frame: A is then C, whose states exist).  *advanced = the round ended the frame.  nodes: the utterance's pool of node_cap nodes;
// returns -1 if it would overflow (it cannot within node_bound).  sel: room for WMAX candidates (the kernel passes LDS: one thread runs
// the round, and a local array would be scratch memory of every lane of the launch)
// BOOST: ex_bonus / ex_bstate [i][KTOP] = the entry's phrase bonus and the automaton state after it
template <bool LM, bool BOOST = false>
NASR_LP_HD int round_step_t(Beam &b, int W, int S, bool prune, const float *lb, const int32_t *ex_tok, const float *ex_lp, const int *ex_n,
                            Node *nodes, long long node_cap, Child *children, bool *advanced, Hyp *sel, float wt, float tb, const double *ex_lm,
                            const int32_t *ex_state, const float *ex_bonus = nullptr, const int32_t *ex_bstate = nullptr) {
    *advanced = false;
    if (b.t >= b.T) return 0;
    for (int i = 0; i < b.na; i++) {
        Hyp h;
        copy_hyp<BOOST>(h, b.a[i]);
        h.score += (double)lb[i];
        c_arrive_t<LM, BOOST>(b, W, nodes, h, wt, tb);
    }
    if (b.v == S) {                                           // the frame is over: Beam_{t+1} = C
        for (int i = 0; i < b.nc; i++) copy_hyp<BOOST>(b.a[i], b.c[i]);
        b.na = b.nc; b.nc = 0; b.t++; b.v = 0;
        *advanced = true;
        return 0;
    }
    // the W best of D in arrival order; sel[].node = parent index in A, .slot = position in its expansion list, until the nodes are made
    int32_t ns = 0;
    const bool full = b.nc >= W;
    const double floor_c = full ? total_of<LM, BOOST>(b.c[W - 1], wt, tb) : 0.0;
    for (int i = 0; i < b.na; i++)
        for (int k = 0; k < ex_n[i]; k++) {
            Hyp h;
            h.score = b.a[i].score + (double)ex_lp[i * KTOP + k];
            h.len = b.a[i].len + 1;
            h.lm = LM ? b.a[i].lm + ex_lm[i * KTOP + k] : 0.0;
            h.lm_state = LM ? ex_state[i * KTOP + k] : 0;
            if (BOOST) { h.boost = b.a[i].boost + (double)ex_bonus[i * KTOP + k]; h.boost_state = ex_bstate[i * KTOP + k]; }
            if (prune && full && !(total_of<LM, BOOST>(h, wt, tb) > floor_c)) continue;
            h.hash = 0; h.node = i; h.slot = k;
            insert_sorted_t<LM, BOOST>(sel, ns, W, h, wt, tb);
        }
    unsigned used = 0;
    for (int i = 0; i < b.nc; i++) used |= 1u << b.c[i].slot;
    for (int i = 0; i < b.na; i++) used |= 1u << b.a[i].slot;
    if (b.n_nodes + ns > node_cap) return -1;
    for (int j = 0; j < ns; j++) {
        const Hyp &par = b.a[sel[j].node];
        const int tok = ex_tok[sel[j].node * KTOP + sel[j].slot];
        Node nd;
        nd.parent = par.node; nd.token = tok; nd.frame = b.t; nd.lp = ex_lp[sel[j].node * KTOP + sel[j].slot];
        nodes[b.n_nodes] = nd;
        children[j].parent_slot = par.slot; children[j].token = tok; children[j].slot = take_slot(used, W); children[j].pad = 0;
        if (children[j].slot < 0) return -1;                  // cannot happen: C, A and A's children hold at most 3 W slots
        Hyp h;
        h.score = sel[j].score; h.hash = hash_next(par.hash, tok); h.node = b.n_nodes; h.len = par.len + 1; h.slot = children[j].slot;
        h.lm_state = sel[j].lm_state; h.lm = sel[j].lm;
        if (BOOST) { h.boost = sel[j].boost; h.boost_state = sel[j].boost_state; }
        copy_hyp<BOOST>(sel[j], h);
        b.n_nodes++;
    }
    for (int j = 0; j < ns; j++) copy_hyp<BOOST>(b.a[j], sel[j]);
    b.na = ns; b.v++;
    return ns;
}

// the final order with an LM: rank[0 .. return value) = indices into a[0 .. na), the N best by score + weight * lm_final + token_bonus * len,
// stable on ties; total_final[i] = that key of a[i].  One thread runs it over <= 8 entries
// final_rank_t<LM, BOOST>: the same by the boosted key; LM = false: lm_final is not read and the key is score + boost
template <bool LM, bool BOOST>
NASR_LP_HD int final_rank_t(const Hyp *a, int na, int N, const double *lm_final, float weight, float token_bonus, int32_t *rank, double *total_final) {
    int32_t n = 0;
    for (int i = 0; i < na; i++) {
        Hyp h;
        copy_hyp<BOOST>(h, a[i]);
        if (LM) h.lm = lm_final[i];
        total_final[i] = total_of<LM, BOOST>(h, weight, token_bonus);
        int pos = n;
        while (pos > 0 && total_final[rank[pos - 1]] < total_final[i]) pos--;
        if (pos >= N) continue;
        const int last = n < N ? n : N - 1;
        for (int j = last; j > pos; j--) rank[j] = rank[j - 1];
        rank[pos] = i;
        if (n < N) n++;
    }
    return n;
}

template <bool BOOST = false>
NASR_LP_HD void beam_begin(Beam &b, int T, int lm_start = 0) {
    b.na = 1; b.nc = 0; b.t = 0; b.v = 0; b.n_nodes = 0; b.T = T;
    b.a[0].score = 0.0; b.a[0].hash = hash0(); b.a[0].node = -1; b.a[0].len = 0; b.a[0].slot = 0; b.a[0].lm_state = lm_start; b.a[0].lm = 0.0;
    if (BOOST) { b.a[0].boost = 0.0; b.a[0].boost_state = nasr_boost::STATE_ROOT; }
}

// tokens, frames and ln P of a hypothesis, from its last node back to the root
NASR_LP_HD void backtrace(const Node *nodes, int node, int len, int32_t *tokens, int32_t *frames, float *lps) {
    for (int i = len - 1; i >= 0 && node >= 0; i--) {
        tokens[i] = nodes[node].token; frames[i] = nodes[node].frame; lps[i] = nodes[node].lp;
        node = nodes[node].parent;
    }
}

}  // namespace nasr_beam

#if !defined(__HIPCC__)
#include <vector>
namespace nasr_beam {
struct Result {
    double score; std::vector<int32_t> tokens, frames; std::vector<float> lps;
    double lm = 0.0, lm_final = 0.0, total = 0.0;       // the fused search only (total = the final key; without an LM they stay 0)
    double boost = 0.0; std::vector<float> bonuses;     // the boosted search only (then total is the boosted key, with or without an LM)
    int32_t boost_state = 0;                            // ... the automaton state the search carried for the hypothesis
};
// the boost tables as the kernels see them: bonus / next [states][COLS] (nasr_boost::Automaton's vectors)
struct BoostTables { const float *bonus; const int32_t *next; int states; };
// A whole search on the host.  eval(t, tokens, len, &lb, top[KTOP], &m, &log_s) gives, for the state after `tokens`, ln P(blank), the row's 8
// largest packed keys in the alternatives' order (blank among them or not) and its softmax (m, log s): what the joint kernels leave per row.
// After every round it checks the slot binding: each child's slot lies in 0 .. 3 W - 1 and is held by no entry of C, no parent and no other
// child.  Returns the node count, -1 if the trie or the slots ran out, -2 if a slot was bound twice.
// lm != nullptr: the fused search (weight, token_bonus as in the header); *pruned = whether the prune was applied.
// BOOST (bt != nullptr): the boosted search.  eval(t, tokens, len, &lb, &raw, &m, &log_s) then gives the row's RAW logits (raw -> 1025 floats that
// stay valid until the next call) in place of the keys; the boosted list is expand_boost's
template <bool LM, bool BOOST = false, class Eval>
long long search_t(int T, int W, int N, int S, bool prune, Eval eval, std::vector<Result> &out, const nasr_lm::View *lm, float weight, float token_bonus,
                   bool *pruned, const BoostTables *bt = nullptr) {
    out.clear();
    if (LM) prune = prune && prune_allowed(token_bonus, lm->all_nonpositive != 0);
    if (BOOST) prune = prune && prune_allowed(0.0f, true, bt->states);
    if (pruned) *pruned = prune;
    const long long cap = node_bound(T > 0 ? T : 0, W, S);
    std::vector<Node> nodes((size_t)cap + 1);
    Beam b;
    beam_begin<BOOST>(b, T > 0 ? T : 0, LM ? lm->start : 0);
    for (long long r = 0; T > 0 && r < rounds(T, S); r++) {
        float lb[WMAX], ex_lp[WMAX * KTOP], ex_bonus[WMAX * KTOP];
        int32_t ex_tok[WMAX * KTOP], ex_state[WMAX * KTOP], ex_bstate[WMAX * KTOP];
        double ex_lm[WMAX * KTOP];
        int ex_n[WMAX];
        for (int i = 0; i < b.na; i++) {
            std::vector<int32_t> seq((size_t)b.a[i].len), fr((size_t)b.a[i].len);
            std::vector<float> lps((size_t)b.a[i].len);
            backtrace(nodes.data(), b.a[i].node, b.a[i].len, seq.data(), fr.data(), lps.data());
            float m = 0.0f, log_s = 0.0f;
            if constexpr (BOOST) {
                const float *raw = nullptr;
                eval(b.t, seq.data(), b.a[i].len, &lb[i], &raw, &m, &log_s);
                ex_n[i] = expand_boost(raw, bt->bonus, bt->next, b.a[i].boost_state, W, m, log_s, ex_tok + i * KTOP, ex_lp + i * KTOP, ex_bonus + i * KTOP,
                                       ex_bstate + i * KTOP);
            } else {
                nasr_topk::tkey top[KTOP];
                eval(b.t, seq.data(), b.a[i].len, &lb[i], top, &m, &log_s);
                ex_n[i] = expand(top, W, m, log_s, ex_tok + i * KTOP, ex_lp + i * KTOP);
            }
            for (int k = 0; LM && k < ex_n[i]; k++) ex_lm[i * KTOP + k] = nasr_lm::lookup(*lm, b.a[i].lm_state, ex_tok[i * KTOP + k], &ex_state[i * KTOP + k]);
        }
        unsigned parents = 0;
        for (int i = 0; i < b.na; i++) parents |= 1u << b.a[i].slot;
        Child ch[WMAX];
        Hyp sel[WMAX];
        bool adv;
        const int n = round_step_t<LM, BOOST>(b, W, S, prune, lb, ex_tok, ex_lp, ex_n, nodes.data(), cap, ch, &adv, sel, weight, token_bonus, ex_lm, ex_state,
                                              ex_bonus, ex_bstate);
        if (n < 0) return -1;
        unsigned held = parents;
        for (int i = 0; i < b.nc; i++) held |= 1u << b.c[i].slot;
        for (int j = 0; j < n; j++) {
            if (ch[j].slot < 0 || ch[j].slot >= n_slots(W) || (held & (1u << ch[j].slot)) || b.a[j].slot != ch[j].slot) return -2;
            held |= 1u << ch[j].slot;
        }
    }
    int32_t rank[WMAX];
    double lm_final[WMAX], total[WMAX];
    int n_out = b.na < N ? b.na : N;
    for (int i = 0; i < n_out; i++) rank[i] = i;
    if (LM) {
        for (int i = 0; i < b.na; i++) {
            int32_t next;
            lm_final[i] = lm->has_eos ? b.a[i].lm + nasr_lm::lookup(*lm, b.a[i].lm_state, nasr_lm::EOS, &next) : b.a[i].lm;
        }
    }
    if (LM || BOOST) n_out = final_rank_t<LM, BOOST>(b.a, b.na, N, lm_final, weight, token_bonus, rank, total);
    for (int j = 0; j < n_out; j++) {
        const Hyp &h = b.a[rank[j]];
        Result r;
        r.score = h.score;
        r.tokens.resize((size_t)h.len); r.frames.resize((size_t)h.len); r.lps.resize((size_t)h.len);
        backtrace(nodes.data(), h.node, h.len, r.tokens.data(), r.frames.data(), r.lps.data());
        if (LM) { r.lm = h.lm; r.lm_final = lm_final[rank[j]]; }
        if (LM || BOOST) r.total = total[rank[j]];
        if (BOOST) {                                          // the per-token bonuses, by the tables, from the root
            r.boost = h.boost; r.boost_state = h.boost_state;
            int st = nasr_boost::STATE_ROOT;
            for (int32_t tk : r.tokens) { r.bonuses.push_back(nasr_boost::bonus_of(bt->bonus, st, tk)); st = nasr_boost::next_of(bt->next, st, tk); }
        }
        out.push_back(r);
    }
    return b.n_nodes;
}
template <class Eval>
long long search(int T, int W, int N, int S, bool prune, Eval eval, std::vector<Result> &out) {
    return search_t<false>(T, W, N, S, prune, eval, out, nullptr, 0.0f, 0.0f, nullptr);
}
template <class Eval>
long long search(int T, int W, int N, int S, bool prune, Eval eval, std::vector<Result> &out, const nasr_lm::View &lm, float weight, float token_bonus,
                 bool *pruned = nullptr) {
    return search_t<true>(T, W, N, S, prune, eval, out, &lm, weight, token_bonus, pruned);
}
// the boosted searches (eval gives raw logits, see search_t)
template <class Eval>
long long search_boost(int T, int W, int N, int S, bool prune, Eval eval, std::vector<Result> &out, const BoostTables &bt, bool *pruned = nullptr) {
    return search_t<false, true>(T, W, N, S, prune, eval, out, nullptr, 0.0f, 0.0f, pruned, &bt);
}
template <class Eval>
long long search_boost(int T, int W, int N, int S, bool prune, Eval eval, std::vector<Result> &out, const BoostTables &bt, const nasr_lm::View &lm, float weight,
                       float token_bonus, bool *pruned = nullptr) {
    return search_t<true, true>(T, W, N, S, prune, eval, out, &lm, weight, token_bonus, pruned, &bt);
}
}  // namespace nasr_beam
#endif
