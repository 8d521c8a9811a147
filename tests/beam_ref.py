"""float64 reference of the frame-synchronous beam search (nasr_engine_transcribe_beam*; the rules are csrc/nasr_beam.h) over any
`joint(t, y) -> 1025 logits` callable, y a tuple of token ids.  No GPU here.

    Beam_0 = {((), 0)};  per frame t: A = Beam_t, C = {};  for v = 0 .. S: every h of A arrives in C with h.score + lb(t, h), C keeps
    its W best; if v == S stop; D = children (h.y + k) over expand(h); A = the W best of D.  Beam_{t+1} = C.  Result: the N best of Beam_T.

expand(h): the 8 largest outputs (descending logit, lower id first among equal logits), blank dropped, the first W of the rest.  Arrivals in
C with the same sequence merge: the higher score stays with its frames, a later arrival replaces only when strictly greater.  Among equal
scores the earlier arrival wins.  Beam 1 is not the greedy decode.

search() also records how close its decisions were: `margin` = the smallest gap between the last kept and the first dropped candidate over
every keep-W (C and D) and between neighbours of the final order; `merge_margin` = the smallest |difference| of two scores that met in a
merge (it decides frames, not tokens); `expand_margin` = the smallest gap, in ln P of ONE row, between the last output an expansion list takes
and the first it leaves out (W <= 7: the W-th and (W + 1)-th non-blank outputs; W = 8: the 8th and 9th outputs, blank included, which also
decides whether blank is among the 8).  The first two compare sums along different paths; the third compares two values of the same cell."""
import numpy as np

BLANK, V = 1024, 1025


def log_softmax64(logits):
    x = np.asarray(logits, np.float64)
    return x - np.logaddexp.reduce(x)


def log_softmax32(logits):
    """ln-softmax values rounded to f32, as the engine's cells are"""
    return log_softmax64(logits).astype(np.float32).astype(np.float64)


def top_order(logits):
    """vocabulary ids by descending logit, lower id first among equal logits (the alternatives' order)"""
    x = np.asarray(logits)
    return np.lexsort((np.arange(x.size), -x.astype(np.float64)))


class Hyp:
    __slots__ = ("y", "frames", "lps", "score")

    def __init__(self, y, frames, lps, score):
        self.y, self.frames, self.lps, self.score = y, frames, lps, score


def _insert(lst, h, W, stats):
    """behind the entries whose score is not lower; keep W"""
    pos = len(lst)
    while pos > 0 and lst[pos - 1].score < h.score:
        pos -= 1
    lst.insert(pos, h)
    if len(lst) > W:
        dropped = lst.pop()
        stats["margin"] = min(stats["margin"], lst[W - 1].score - dropped.score)


def _arrive(C, h, W, stats):
    for i, g in enumerate(C):
        if g.y == h.y:
            stats["merge_margin"] = min(stats["merge_margin"], abs(h.score - g.score))
            stats["merges"] += 1
            if not h.score > g.score:
                return
            del C[i]
            break
    _insert(C, h, W, stats)


def search(joint, T, W, N=None, S=4, prune=False, logsoftmax=log_softmax64):
    """-> (hyps, stats): hyps = [dict(score, tokens, frames, lps)] best first, at most N; stats = dict(margin, merge_margin, expand_margin, merges, evals)"""
    N = W if N is None else N
    assert 1 <= W <= 8 and 1 <= N <= W and 1 <= S <= 10
    stats = dict(margin=np.inf, merge_margin=np.inf, expand_margin=np.inf, merges=0, evals=0)
    beam = [Hyp((), (), (), 0.0)]
    for t in range(T):
        A, C = beam, []
        for v in range(S + 1):
            rows = []
            for h in A:
                logits = np.asarray(joint(t, h.y))
                stats["evals"] += 1
                rows.append((logits, logsoftmax(logits)))
            for h, (logits, lp) in zip(A, rows):
                _arrive(C, Hyp(h.y, h.frames, h.lps, h.score + float(lp[BLANK])), W, stats)
            if v == S:
                break
            full = len(C) >= W
            floor_c = C[W - 1].score if full else None
            D = []
            for h, (logits, lp) in zip(A, rows):
                order = top_order(logits)
                ex = [int(k) for k in order[:8] if k != BLANK][:W]
                for k in ex:
                    s = h.score + float(lp[k])
                    if prune and full and not s > floor_c:
                        continue
                    D.append(Hyp(h.y + (k,), h.frames + (t,), h.lps + (float(lp[k]),), s))
                nonblank = [int(k) for k in order[:10] if k != BLANK]
                last, first_out = (order[7], order[8]) if W == 8 else (nonblank[W - 1], nonblank[W])
                stats["expand_margin"] = min(stats["expand_margin"], float(lp[last]) - float(lp[first_out]))
            sel = []
            for h in D:                                          # arrival order: parent by parent, each in its expansion order
                pos = len(sel)
                while pos > 0 and sel[pos - 1].score < h.score:
                    pos -= 1
                sel.insert(pos, h)
            kept = sel[:W]
            if not prune and len(sel) > W:
                stats["margin"] = min(stats["margin"], kept[-1].score - sel[W].score)
            A = kept
        beam = C
    for a, b in zip(beam[:N], beam[1:N + 1]):
        stats["margin"] = min(stats["margin"], a.score - b.score)
    hyps = [dict(score=h.score, tokens=list(h.y), frames=list(h.frames), lps=list(h.lps)) for h in beam[:N]]
    return hyps, stats


def greedy(joint, T, max_symbols=10):
    """the greedy decode over the same callable (arg-max, first maximum; at most max_symbols tokens per frame)"""
    y, frames = (), []
    for t in range(T):
        for _ in range(max_symbols):
            k = int(top_order(joint(t, y))[0])
            if k == BLANK:
                break
            y += (k,)
            frames.append(t)
    return list(y), frames


class OracleJoint:
    """joint(t, y) over the oracle's decoder + joint (oracle.binding.OracleModel.decoder_joint) and given encoder rows [T][1024]: the
    prediction-network state after blank, y_0 .. y_{n-1} from the zero state, grown token by token and kept per sequence"""

    def __init__(self, om, enc):
        self.om = om
        self.enc = np.asarray(enc, np.float32).reshape(-1, 1024)
        self.state = {(): (np.zeros(1280, np.float32), np.zeros(1280, np.float32), BLANK)}     # committed h, c and the token to consume
        self.rows = {}

    def __call__(self, t, y):
        y = tuple(int(k) for k in y)
        if (t, y) not in self.rows:
            h, c, prev = self.state[y]
            logits, hn, cn = self.om.decoder_joint(prev, h, c, self.enc[t])
            self.rows[(t, y)] = np.asarray(logits)
            for k in top_order(logits)[:9]:                      # the children the search can make of y
                if int(k) != BLANK:
                    self.state.setdefault(y + (int(k),), (hn, cn, int(k)))
        return self.rows[(t, y)]
