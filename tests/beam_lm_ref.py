"""float64 reference of the beam search with shallow fusion (the fused rules of csrc/nasr_beam.h), built on tests/beam_ref.py and
tests/lm_ref.py.  No GPU here.

A hypothesis also carries lm (the sum of its tokens' LM terms) and everything beam_ref.search orders by score is ordered by
    total = score + weight * lm + token_bonus * len
evaluated as that expression in double (weight and token_bonus as float32 values).  The expansion list is unchanged.  The prune is applied
only when token_bonus == 0 and no logprob or backoff is positive.  At the end, when some n-gram ends in EOS, lm_final = lm + the EOS term,
and the N best of Beam_T are taken by score + weight * lm_final + token_bonus * len, stable on ties.

search() reports, as beam_ref.search does, `margin` (the smallest decision margin, here on TOTALS: every keep-W of C and D and the
neighbours of the final order, first dropped entry included), `merge_margin` (the smallest gap of two totals that met in a merge; lm and len
are equal there, so it is the gap of the scores) and `expand_margin` (the expansion-cut distance, a property of one row)."""
import numpy as np

from tests import beam_ref as br
from tests import lm_ref

BLANK = br.BLANK


class Hyp:
    __slots__ = ("y", "frames", "lps", "score", "lm", "hist")

    def __init__(self, y, frames, lps, score, lm, hist):
        self.y, self.frames, self.lps, self.score, self.lm, self.hist = y, frames, lps, score, lm, hist


def total_of(score, lm, n, weight, bonus):
    a = float(np.float32(weight)) * lm
    b = float(np.float32(bonus)) * float(n)
    return score + a + b


def search(joint, T, W, N=None, S=4, prune=False, logsoftmax=br.log_softmax64, lm=None, weight=0.0, bonus=0.0):
    """lm: a lm_ref.RefLM.  -> (hyps, stats); hyps = [dict(score, tokens, frames, lps, lm, lm_final, total)] best first; stats as
    beam_ref.search plus `pruned` (whether the prune was applied)"""
    N = W if N is None else N
    assert 1 <= W <= 8 and 1 <= N <= W and 1 <= S <= 10 and lm is not None
    prune = bool(prune and float(np.float32(bonus)) == 0.0 and lm.all_nonpositive)
    stats = dict(margin=np.inf, merge_margin=np.inf, expand_margin=np.inf, merges=0, evals=0, pruned=prune)
    key = lambda h: total_of(h.score, h.lm, len(h.y), weight, bonus)

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

    beam = [Hyp((), (), (), 0.0, 0.0, lm.start())]
    for t in range(T):
        A, C = beam, []
        for v in range(S + 1):
            rows = []
            for h in A:
                logits = np.asarray(joint(t, h.y))
                stats["evals"] += 1
                rows.append((logits, logsoftmax(logits)))
            for h, (logits, lp) in zip(A, rows):
                arrive(C, Hyp(h.y, h.frames, h.lps, h.score + float(lp[BLANK]), h.lm, h.hist))
            if v == S:
                break
            full = len(C) >= W
            floor_c = key(C[W - 1]) if full else None
            sel = []
            for h, (logits, lp) in zip(A, rows):
                order = br.top_order(logits)
                for k in [int(k) for k in order[:8] if k != BLANK][:W]:
                    c = Hyp(h.y + (k,), h.frames + (t,), h.lps + (float(lp[k]),), h.score + float(lp[k]), h.lm + lm.term(h.hist, k), h.hist + (k,))
                    if prune and full and not key(c) > floor_c:
                        continue
                    insert(sel, c, False)
                nonblank = [int(k) for k in order[:10] if k != BLANK]
                last, first_out = (order[7], order[8]) if W == 8 else (nonblank[W - 1], nonblank[W])
                stats["expand_margin"] = min(stats["expand_margin"], float(lp[last]) - float(lp[first_out]))
            if not prune and len(sel) > W:
                stats["margin"] = min(stats["margin"], key(sel[W - 1]) - key(sel[W]))
            A = sel[:W]
        beam = C
    final = []
    for h in beam:
        lm_final = h.lm + lm.term(h.hist, lm_ref.EOS) if lm.has_eos else h.lm
        final.append((h, lm_final, total_of(h.score, lm_final, len(h.y), weight, bonus)))
    ranked = []
    for item in final:                                        # stable: behind the entries whose total is not lower
        pos = len(ranked)
        while pos > 0 and ranked[pos - 1][2] < item[2]:
            pos -= 1
        ranked.insert(pos, item)
    for a, b in zip(ranked[:N], ranked[1:N + 1]):
        stats["margin"] = min(stats["margin"], a[2] - b[2])
    hyps = [dict(score=h.score, tokens=list(h.y), frames=list(h.frames), lps=list(h.lps), lm=h.lm, lm_final=lf, total=tot) for h, lf, tot in ranked[:N]]
    return hyps, stats
