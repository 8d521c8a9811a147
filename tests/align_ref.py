"""float64 reference of forced alignment / transcript scoring on the RNN-T lattice (nasr_engine_align*): the oracle's decoder + joint
(oracle.binding.OracleModel.decoder_joint) teacher-forced over a transcript for every (frame, label position) cell, the log-softmax
and both recursions in float64.  No GPU here; tests/test_gpu_align.py feeds it the engine's own encoder rows."""
import numpy as np

BLANK, V = 1024, 1025


def lattice(om, enc, y):
    """(lb, ly), each [T][U + 1] float64: ln softmax at blank / at y[u] of the joint of frame t and the prediction-network state after
    blank, y[0] .. y[u - 1] from the zero state; column U of ly is -inf.  T * (U + 1) oracle calls."""
    enc = np.asarray(enc, np.float32).reshape(-1, 1024)
    T, U = enc.shape[0], len(y)
    lb, ly = np.zeros((T, U + 1)), np.full((T, U + 1), -np.inf)
    h, c, prev = np.zeros(1280, np.float32), np.zeros(1280, np.float32), BLANK
    for u in range(U + 1):
        hn = cn = None
        for t in range(T):
            logits, hn, cn = om.decoder_joint(prev, h, c, enc[t])
            x = logits.astype(np.float64)
            lse = np.logaddexp.reduce(x)
            lb[t, u] = x[BLANK] - lse
            if u < U:
                ly[t, u] = x[y[u]] - lse
        if u < U and T > 0:
            prev, h, c = int(y[u]), hn, cn
    return lb, ly


def recursions(lb, ly):
    """-> dict(loglik, best, frames, margin): the standard RNN-T lattice.  Tie rule: the token move (t, u - 1) -> (t, u) is taken only
    when its score is strictly greater than the blank move's.  margin = the smallest |token-move score - blank-move score| over the
    cells the backtrace visits (inf where a cell has one predecessor only)."""
    lb, ly = np.asarray(lb, np.float64), np.asarray(ly, np.float64)
    T, U = lb.shape[0], lb.shape[1] - 1
    if T == 0:
        v = 0.0 if U == 0 else -np.inf
        return dict(loglik=v, best=v, frames=[-1] * U, margin=np.inf)
    alpha, delta = np.full((T, U + 1), -np.inf), np.full((T, U + 1), -np.inf)
    tok = np.zeros((T, U + 1), bool)
    gap = np.full((T, U + 1), np.inf)
    alpha[0, 0] = delta[0, 0] = 0.0
    for t in range(T):
        for u in range(U + 1):
            if t == 0 and u == 0:
                continue
            ab = alpha[t - 1, u] + lb[t - 1, u] if t > 0 else -np.inf
            at = alpha[t, u - 1] + ly[t, u - 1] if u > 0 else -np.inf
            sb = delta[t - 1, u] + lb[t - 1, u] if t > 0 else -np.inf
            st = delta[t, u - 1] + ly[t, u - 1] if u > 0 else -np.inf
            alpha[t, u] = np.logaddexp(ab, at)
            tok[t, u] = u > 0 and (t == 0 or st > sb)
            delta[t, u] = st if tok[t, u] else sb
            if t > 0 and u > 0:
                gap[t, u] = abs(st - sb)
    frames, margin = [0] * U, np.inf
    t, u = T - 1, U
    while u > 0:
        margin = min(margin, gap[t, u])
        if tok[t, u]:
            u -= 1
            frames[u] = t
        else:
            t -= 1
    return dict(loglik=float(alpha[T - 1, U] + lb[T - 1, U]), best=float(delta[T - 1, U] + lb[T - 1, U]), frames=frames, margin=float(margin))


def path_score(lb, ly, frames):
    """the score of the path that emits token i at frames[i] (non-decreasing), the final blank included"""
    T, U = lb.shape[0], lb.shape[1] - 1
    assert len(frames) == U
    s, t = 0.0, 0
    for u, f in enumerate(frames):
        assert t <= f < T
        s += lb[t:f, u].sum() + ly[f, u]
        t = f
    return float(s + lb[t:T, U].sum())
