"""float64 reference of the back-off n-gram language model of the beam search's shallow fusion (csrc/nasr_lm.h), straight from the n-gram
dictionary: the recursive ARPA definition, no states and no hash table.  No GPU here.

    P(w | ctx) = p(ctx w) if that n-gram is in the set, else backoff(ctx) * P(w | ctx without its oldest token); backoff = 1 for a context
    that is not in the set; at the empty context the dense unigram (own value, else unk_logprob).

ngrams: {token tuple: (logprob, backoff)}, natural logs.  Every value is taken as float32 and the terms are summed in double in the order
met -- the backoffs passed, longest context first, then the n-gram's logprob -- which is what nasr_lm::lookup returns, so results are
compared exactly.  A context that is not in the set adds nothing (not even + 0.0).  The reference state machine below gives the context the
compiled form must be in after a token: the longest suffix of (history + token), of at most order - 1 tokens, that is in the set."""
import numpy as np

BLANK, BOS, EOS = 1024, 1025, 1026


def f32(x):
    return float(np.float32(x))


class RefLM:
    def __init__(self, ngrams, order, unk_logprob):
        self.order = int(order)
        self.unk = f32(unk_logprob)
        self.g = {}
        for k, v in ngrams.items():
            lp, bo = (v, 0.0) if np.isscalar(v) else v
            self.g[tuple(int(t) for t in k)] = (f32(lp), f32(bo))
        self.has_eos = any(k[-1] == EOS for k in self.g)
        self.all_nonpositive = all(lp <= 0.0 and bo <= 0.0 for lp, bo in self.g.values())

    def start(self):
        """the history before the first token: (BOS,) -- equivalent to () when no n-gram starts with BOS"""
        return (BOS,)

    def term(self, history, w):
        """ln P(w | history): the recursive definition, accumulated in the order met"""
        ctx = tuple(history)[-(self.order - 1):] if self.order > 1 else ()
        acc = 0.0
        while True:
            if ctx + (w,) in self.g and len(ctx) > 0:
                return acc + self.g[ctx + (w,)][0]
            if len(ctx) == 0:
                return acc + (self.g[(w,)][0] if (w,) in self.g else self.unk)
            if ctx in self.g:
                acc += self.g[ctx][1]
            ctx = ctx[1:]

    def context_after(self, history, w):
        """the reference state machine: the longest suffix of history + (w,), of at most order - 1 tokens, that is in the set (() if none)"""
        seq = tuple(history) + (w,)
        for n in range(min(self.order - 1, len(seq)), 0, -1):
            if seq[-n:] in self.g:
                return seq[-n:]
        return ()

    def score(self, tokens, eos=None):
        """-> (lm, per-token terms): the sum of the tokens' terms in token order; eos (default: has_eos) adds the EOS term at the end"""
        hist, lm, terms = self.start(), 0.0, []
        for k in tokens:
            t = self.term(hist, int(k))
            terms.append(t)
            lm += t
            hist += (int(k),)
        if self.has_eos if eos is None else eos:
            lm += self.term(hist, EOS)
        return lm, terms


def random_lm(rng, order, n_tokens, tokens=None, bos=True, eos=True, positive_backoff=False, density=0.5, max_per_level=400):
    """a random valid set: every context of an n-gram is in the set.  tokens: the ids to draw from (default: n_tokens random ids)"""
    ids = [int(t) for t in (tokens if tokens is not None else rng.choice(1024, size=n_tokens, replace=False))]
    first = ids + ([BOS] if bos else [])
    g = {}
    for w in ids:
        if rng.random() < 0.85:
            g[(w,)] = None
    if bos:
        g[(BOS,)] = None
    if eos and rng.random() < 0.7:
        g[(EOS,)] = None
    level = [k for k in g if k[-1] != EOS]
    for n in range(2, order + 1):
        nxt = []
        for _ in range(min(max_per_level, int(density * len(level) * len(ids)) + 1)):
            if not level:
                break
            ctx = level[int(rng.integers(len(level)))]
            w = EOS if (eos and rng.random() < 0.15) else ids[int(rng.integers(len(ids)))]
            k = ctx + (w,)
            if k not in g:
                g[k] = None
                if w != EOS:
                    nxt.append(k)
        level = nxt
    out = {}
    for k in g:
        lp = -float(rng.random()) * 6.0 - 0.01
        bo = float(rng.standard_normal()) * 0.7
        bo = bo if positive_backoff else -abs(bo)
        if len(k) == order or k[-1] == EOS:
            bo = 0.0
        out[k] = (f32(lp), f32(bo))
    if eos and not any(k[-1] == EOS for k in out):
        out[(EOS,)] = (f32(-2.5), 0.0)
    if positive_backoff and not any(bo > 0 for _, bo in out.values()):
        k = next(k for k in out if len(k) < order and k[-1] != EOS) if order > 1 else None
        if k is not None:
            out[k] = (out[k][0], f32(0.375))
    return out
