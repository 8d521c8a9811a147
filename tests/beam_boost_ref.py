"""float64 reference of the beam search with phrase boosting, with and without shallow fusion (the BOOST rules of csrc/nasr_beam.h), built
on tests/beam_ref.py, tests/beam_lm_ref.py and a brute-force bonus taken from the definition in csrc/nasr_boost.h, not from the automaton.
No GPU here.

    bonus(h, v) = max { w_i : 0 <= k < len(p_i), p_i[0:k] is a suffix of h, p_i[k] == v }         (0 if there is no such pair; never for blank)

A hypothesis also carries boost = the sum of bonus(y[:i], y[i]) over its tokens.  Its expansion list comes from the row's outputs ordered by
float32(logit) + float32(bonus) (one float32 add, descending, the lower id first among equal values): the first 8, blank dropped, the first W
of the rest.  ln P of a child stays the model's.  Everything beam_lm_ref.search orders by total is ordered by
    key = (score + weight * lm + token_bonus * len) + boost                      (score + boost without an LM)
The prune is applied only where beam_lm_ref applies it AND the phrase set is empty.

search() reports the same `stats` as beam_lm_ref.search, with `margin` and `merge_margin` on the boosted key and `expand_margin` measured on
logit + bonus (the float32 sums: what the expansion cut compares), plus `proposed_by_boost`: the number of selected children (entries of A)
whose token was outside the 8 largest RAW outputs of their parent's row."""
import numpy as np

from tests import beam_lm_ref as blr
from tests import beam_ref as br
from tests import lm_ref

BLANK, V = br.BLANK, br.V


class Phrases:
    """a boost set: [(tokens, bonus)]; bonus_row(history) by brute force over every phrase and every prefix length"""

    def __init__(self, phrases):
        self.items = [(tuple(int(t) for t in p), float(np.float32(w))) for p, w in phrases]
        self.maxlen = max((len(p) for p, _ in self.items), default=1)
        self.memo = {}

    def __len__(self):
        return len(self.items)

    def bonus_row(self, hist):
        """float32 [1025]: the bonus of every vocabulary entry after the emitted history `hist`"""
        tail = tuple(hist)[-(self.maxlen - 1):] if self.maxlen > 1 else ()
        if tail not in self.memo:
            row = np.zeros(V, np.float32)
            for p, w in self.items:
                for k in range(len(p)):
                    if k <= len(tail) and (k == 0 or tail[len(tail) - k:] == p[:k]):
                        row[p[k]] = max(row[p[k]], np.float32(w))
            self.memo[tail] = row
        return self.memo[tail]

    def bonuses(self, tokens):
        """the per-token bonuses of a token sequence from the empty history"""
        return [float(self.bonus_row(tokens[:i])[tokens[i]]) for i in range(len(tokens))]


def key_of(score, lm, n, weight, bonus, boost, with_lm):
    base = blr.total_of(score, lm, n, weight, bonus) if with_lm else score
    return base + boost


class Hyp:
    __slots__ = ("y", "frames", "lps", "score", "lm", "hist", "boost")

    def __init__(self, y, frames, lps, score, lm, hist, boost):
        self.y, self.frames, self.lps, self.score, self.lm, self.hist, self.boost = y, frames, lps, score, lm, hist, boost


def search(joint, T, W, N=None, S=4, prune=False, logsoftmax=br.log_softmax64, phrases=None, lm=None, weight=0.0, bonus=0.0):
    """phrases: a Phrases; lm: a lm_ref.RefLM or None.  -> (hyps, stats); hyps = [dict(score, tokens, frames, lps, lm, lm_final, total, boost,
    bonuses)] best first"""
    N = W if N is None else N
    assert 1 <= W <= 8 and 1 <= N <= W and 1 <= S <= 10 and phrases is not None
    with_lm = lm is not None
    prune = bool(prune and len(phrases) == 0 and (not with_lm or (float(np.float32(bonus)) == 0.0 and lm.all_nonpositive)))
    stats = dict(margin=np.inf, merge_margin=np.inf, expand_margin=np.inf, merges=0, evals=0, pruned=prune, proposed_by_boost=0)
    key = lambda h: key_of(h.score, h.lm, len(h.y), weight, bonus, h.boost, with_lm)
    ensure_child = getattr(joint, "ensure_child", None)

    def insert(lst, h, keep):
        pos = len(lst)
        while pos > 0 and key(lst[pos - 1]) < key(h):
            pos -= 1
        lst.insert(pos, h)
        if keep and len(lst) > W:
            dropped = lst.pop()
            stats["margin"] = min(stats["margin"], key(lst[W - 1]) - key(dropped))

    def arrive(C, h):
        for i, g in enumerate(C):
            if g.y == h.y:
                stats["merge_margin"] = min(stats["merge_margin"], abs(key(h) - key(g)))
                stats["merges"] += 1
                if not key(h) > key(g):
                    return
                del C[i]
                break
        insert(C, h, True)

    beam = [Hyp((), (), (), 0.0, 0.0, lm.start() if with_lm else (), 0.0)]
    for t in range(T):
        A, C = beam, []
        for v in range(S + 1):
            rows = []
            for h in A:
                logits = np.asarray(joint(t, h.y))
                stats["evals"] += 1
                rows.append((logits, logsoftmax(logits)))
            for h, (logits, lp) in zip(A, rows):
                arrive(C, Hyp(h.y, h.frames, h.lps, h.score + float(lp[BLANK]), h.lm, h.hist, h.boost))
            if v == S:
                break
            full = len(C) >= W
            floor_c = key(C[W - 1]) if full else None
            sel = []
            for h, (logits, lp) in zip(A, rows):
                brow = phrases.bonus_row(h.y)
                boosted = np.asarray(logits, np.float32) + brow                       # one float32 add per entry
                order = br.top_order(boosted)
                for k in [int(k) for k in order[:8] if k != BLANK][:W]:
                    c = Hyp(h.y + (k,), h.frames + (t,), h.lps + (float(lp[k]),), h.score + float(lp[k]),
                            h.lm + lm.term(h.hist, k) if with_lm else 0.0, h.hist + (k,) if with_lm else (), h.boost + float(brow[k]))
                    if prune and full and not key(c) > floor_c:
                        continue
                    insert(sel, c, False)
                nonblank = [int(k) for k in order[:10] if k != BLANK]
                last, first_out = (order[7], order[8]) if W == 8 else (nonblank[W - 1], nonblank[W])
                stats["expand_margin"] = min(stats["expand_margin"], float(boosted[last]) - float(boosted[first_out]))
            if not prune and len(sel) > W:
                stats["margin"] = min(stats["margin"], key(sel[W - 1]) - key(sel[W]))
            A = sel[:W]
            for c in A:
                parent, k = c.y[:-1], c.y[-1]
                parent_row = np.asarray(joint(t, parent))
                if k not in set(int(x) for x in br.top_order(parent_row)[:8]):
                    stats["proposed_by_boost"] += 1
                if ensure_child is not None:
                    ensure_child(parent, k)
        beam = C
    final = []
    for h in beam:
        lm_final = h.lm + lm.term(h.hist, lm_ref.EOS) if with_lm and lm.has_eos else h.lm
        final.append((h, lm_final, key_of(h.score, lm_final, len(h.y), weight, bonus, h.boost, with_lm)))
    ranked = []
    for item in final:                                        # stable: behind the entries whose key is not lower
        pos = len(ranked)
        while pos > 0 and ranked[pos - 1][2] < item[2]:
            pos -= 1
        ranked.insert(pos, item)
    for a, b in zip(ranked[:N], ranked[1:N + 1]):
        stats["margin"] = min(stats["margin"], a[2] - b[2])
    hyps = [dict(score=h.score, tokens=list(h.y), frames=list(h.frames), lps=list(h.lps), lm=h.lm, lm_final=lf, total=tot, boost=h.boost,
                 bonuses=phrases.bonuses(h.y)) for h, lf, tot in ranked[:N]]
    return hyps, stats


class OracleJoint(br.OracleJoint):
    """beam_ref.OracleJoint that can also grow the state of a child outside its parent's 9 largest outputs (a boosted proposal): the
    prediction-network state after y + (k,) is the candidate state of y's evaluation consuming k next, whatever the encoder row"""

    def __init__(self, om, enc):
        super().__init__(om, enc)
        self.cand = {}

    def __call__(self, t, y):
        y = tuple(int(k) for k in y)
        if (t, y) not in self.rows:
            h, c, prev = self.state[y]
            logits, hn, cn = self.om.decoder_joint(prev, h, c, self.enc[t])
            self.rows[(t, y)] = np.asarray(logits)
            self.cand.setdefault(y, (hn, cn))
            for k in br.top_order(logits)[:9]:
                if int(k) != BLANK:
                    self.state.setdefault(y + (int(k),), (hn, cn, int(k)))
        return self.rows[(t, y)]

    def ensure_child(self, y, k):
        y = tuple(int(v) for v in y)
        if y + (int(k),) not in self.state:
            hn, cn = self.cand[y]
            self.state[y + (int(k),)] = (hn, cn, int(k))
