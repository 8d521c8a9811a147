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
// alignment tests' checkpoint).  Phrase boosting is not applied: the scores are the model's probabilities, as in alignment.
// T == 0 gives one hypothesis: empty, score 0.
//
// Trie: every child selected into A is a node (parent, token, frame, ln P).  At most W nodes per round with v < S, so an utterance of T
// frames needs at most T * S * W nodes (node_bound); a sub-batch's pool is the sum.
// Slots: a hypothesis owns one decoder slot (committed LSTM state, candidate, g).  A hypothesis parked in C keeps its slot while A's slots are
// reused, so an utterance has 3 W slots: <= W in C, <= W in A, <= W for A's children.
#pragma once
#include "nasr_topk.h"

namespace nasr_beam {

constexpr int WMAX = 8, SMAX = 10, S_DEFAULT = 4, KTOP = nasr_topk::KMAX, BLANK_ID = nasr_lp::LP_VOCAB - 1;
constexpr int SLOTS_PER_W = 3;
static_assert(KTOP == 8, "the expansion reads the alternatives' 8 keys");

struct Node { int32_t parent, token, frame; float lp; };                  // parent = -1: the root (empty sequence)
struct Hyp {
    double score;
    unsigned long long hash;            // of the token sequence: a pre-filter for same_seq
    int32_t node, len;                  // last trie node (-1: empty), tokens
    int32_t slot, pad;                  // decoder slot within the utterance, 0 .. 3 W - 1
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

// place h behind the entries of list[0 .. n) whose score is not lower; the list keeps at most W entries.  Returns false when h fell off
NASR_LP_HD bool insert_sorted(Hyp *list, int32_t &n, int W, const Hyp &h) {
    int pos = n;
    while (pos > 0 && list[pos - 1].score < h.score) pos--;
    if (pos >= W) return false;
    const int last = n < W ? n : W - 1;
    for (int i = last; i > pos; i--) list[i] = list[i - 1];
    list[pos] = h;
    if (n < W) n++;
    return true;
}

// an arrival in C: merge with the entry of the same sequence (strictly greater replaces), else insert and keep the W best
NASR_LP_HD void c_arrive(Beam &b, int W, const Node *nodes, const Hyp &h) {
    for (int i = 0; i < b.nc; i++) {
        if (b.c[i].hash != h.hash || !same_seq(nodes, b.c[i].node, b.c[i].len, h.node, h.len)) continue;
        if (!(h.score > b.c[i].score)) return;
        for (int j = i; j + 1 < b.nc; j++) b.c[j] = b.c[j + 1];
        b.nc--;
        break;
    }
    insert_sorted(b.c, b.nc, W, h);
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
NASR_LP_HD int round_step(Beam &b, int W, int S, bool prune, const float *lb, const int32_t *ex_tok, const float *ex_lp, const int *ex_n,
                          Node *nodes, long long node_cap, Child *children, bool *advanced, Hyp *sel) {
    *advanced = false;
    if (b.t >= b.T) return 0;
    for (int i = 0; i < b.na; i++) {
        Hyp h = b.a[i];
        h.score += (double)lb[i];
        c_arrive(b, W, nodes, h);
    }
    if (b.v == S) {                                           // the frame is over: Beam_{t+1} = C
        for (int i = 0; i < b.nc; i++) b.a[i] = b.c[i];
        b.na = b.nc; b.nc = 0; b.t++; b.v = 0;
        *advanced = true;
        return 0;
    }
    // the W best of D in arrival order; sel[].node = parent index in A, .len = position in its expansion list, until the nodes are made
    int32_t ns = 0;
    const bool full = b.nc >= W;
    const double floor_c = full ? b.c[W - 1].score : 0.0;
    for (int i = 0; i < b.na; i++)
        for (int k = 0; k < ex_n[i]; k++) {
            Hyp h;
            h.score = b.a[i].score + (double)ex_lp[i * KTOP + k];
            if (prune && full && !(h.score > floor_c)) continue;
            h.hash = 0; h.node = i; h.len = k; h.slot = 0; h.pad = 0;
            insert_sorted(sel, ns, W, h);
        }
    unsigned used = 0;
    for (int i = 0; i < b.nc; i++) used |= 1u << b.c[i].slot;
    for (int i = 0; i < b.na; i++) used |= 1u << b.a[i].slot;
    if (b.n_nodes + ns > node_cap) return -1;
    for (int j = 0; j < ns; j++) {
        const Hyp &par = b.a[sel[j].node];
        const int tok = ex_tok[sel[j].node * KTOP + sel[j].len];
        Node nd;
        nd.parent = par.node; nd.token = tok; nd.frame = b.t; nd.lp = ex_lp[sel[j].node * KTOP + sel[j].len];
        nodes[b.n_nodes] = nd;
        children[j].parent_slot = par.slot; children[j].token = tok; children[j].slot = take_slot(used, W); children[j].pad = 0;
        if (children[j].slot < 0) return -1;                  // cannot happen: C, A and A's children hold at most 3 W slots
        Hyp h;
        h.score = sel[j].score; h.hash = hash_next(par.hash, tok); h.node = b.n_nodes; h.len = par.len + 1; h.slot = children[j].slot; h.pad = 0;
        sel[j] = h;
        b.n_nodes++;
    }
    for (int j = 0; j < ns; j++) b.a[j] = sel[j];
    b.na = ns; b.v++;
    return ns;
}

NASR_LP_HD void beam_begin(Beam &b, int T) {
    b.na = 1; b.nc = 0; b.t = 0; b.v = 0; b.n_nodes = 0; b.T = T;
    b.a[0].score = 0.0; b.a[0].hash = hash0(); b.a[0].node = -1; b.a[0].len = 0; b.a[0].slot = 0; b.a[0].pad = 0;
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
struct Result { double score; std::vector<int32_t> tokens, frames; std::vector<float> lps; };
// A whole search on the host.  eval(t, tokens, len, &lb, top[KTOP], &m, &log_s) gives, for the state after `tokens`, ln P(blank), the row's 8
// largest packed keys in the alternatives' order (blank among them or not) and its softmax (m, log s): what the joint kernels leave per row.
// After every round it checks the slot binding: each child's slot lies in 0 .. 3 W - 1 and is held by no entry of C, no parent and no other
// child.  Returns the node count, -1 if the trie or the slots ran out, -2 if a slot was bound twice
template <class Eval>
long long search(int T, int W, int N, int S, bool prune, Eval eval, std::vector<Result> &out) {
    out.clear();
    if (T <= 0) { out.push_back(Result{0.0, {}, {}, {}}); return 0; }
    const long long cap = node_bound(T, W, S);
    std::vector<Node> nodes((size_t)cap);
    Beam b;
    beam_begin(b, T);
    for (long long r = 0; r < rounds(T, S); r++) {
        float lb[WMAX], ex_lp[WMAX * KTOP];
        int32_t ex_tok[WMAX * KTOP];
        int ex_n[WMAX];
        for (int i = 0; i < b.na; i++) {
            std::vector<int32_t> seq((size_t)b.a[i].len), fr((size_t)b.a[i].len);
            std::vector<float> lps((size_t)b.a[i].len);
            backtrace(nodes.data(), b.a[i].node, b.a[i].len, seq.data(), fr.data(), lps.data());
            nasr_topk::tkey top[KTOP];
            float m = 0.0f, log_s = 0.0f;
            eval(b.t, seq.data(), b.a[i].len, &lb[i], top, &m, &log_s);
            ex_n[i] = expand(top, W, m, log_s, ex_tok + i * KTOP, ex_lp + i * KTOP);
        }
        unsigned parents = 0;
        for (int i = 0; i < b.na; i++) parents |= 1u << b.a[i].slot;
        Child ch[WMAX];
        Hyp sel[WMAX];
        bool adv;
        const int n = round_step(b, W, S, prune, lb, ex_tok, ex_lp, ex_n, nodes.data(), cap, ch, &adv, sel);
        if (n < 0) return -1;
        unsigned held = parents;
        for (int i = 0; i < b.nc; i++) held |= 1u << b.c[i].slot;
        for (int j = 0; j < n; j++) {
            if (ch[j].slot < 0 || ch[j].slot >= n_slots(W) || (held & (1u << ch[j].slot)) || b.a[j].slot != ch[j].slot) return -2;
            held |= 1u << ch[j].slot;
        }
    }
    for (int i = 0; i < b.na && i < N; i++) {
        Result r;
        r.score = b.a[i].score;
        r.tokens.resize((size_t)b.a[i].len); r.frames.resize((size_t)b.a[i].len); r.lps.resize((size_t)b.a[i].len);
        backtrace(nodes.data(), b.a[i].node, b.a[i].len, r.tokens.data(), r.frames.data(), r.lps.data());
        out.push_back(r);
    }
    return b.n_nodes;
}
}  // namespace nasr_beam
#endif
