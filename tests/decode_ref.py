"""float64 references of the RNN-T decode's operations (kernels_decode.hip), plain numpy: the two-layer LSTM candidate, the prediction projection,
the joint with its arg-max key, softmax parts, alternatives and entropy terms, one commit of one stream, build_lists, and the per-stream greedy loop.
Everything is written from the operation's definition (the reference's rules: gates in the order i, f, g, o, c' = sigm(f) c + sigm(i) tanh(g),
h' = sigm(o) tanh(c'); logits = W_out relu(enc + g) + b; first maximum wins; at most 10 symbols per frame), not from the kernels."""
from __future__ import annotations

import numpy as np

HID = JNT = 640
VOCAB, BLANK = 1025, 1024
COLS = 1040                      # the padded vocabulary: 65 tiles of 16
TOK_CAP = FRAME_CAP = 4096
MAX_SYMBOLS = 10
SMALL_ROWS, TILE_PARTS, WG_PARTS = 64, 65, 17
DEC_CTRL = ("t", "n_frames", "symbols", "prev_token", "cur", "n_tok", "active", "iterations", "row", "dirty", "frame0", "frame_next")
CT = {n: i for i, n in enumerate(DEC_CTRL)}


_F64 = {}


def f64(a, absolute=False):
    """a as float64 (its absolute value), converted once per array: the weight matrices are used by every evaluation of a trajectory"""
    k = (id(a), absolute)
    if k not in _F64 or _F64[k][0] is not a:
        v = a.astype(np.float64)
        _F64[k] = (a, np.abs(v) if absolute else v)
    return _F64[k][1]


def sigm(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def lstm_gates(W_ih, W_hh, b_ih, b_hh, x, h):
    """pre-activations [n][4][HID], gate order i, f, g, o (row j * HID + unit of the [4 HID][HID] matrices)"""
    f = np.float64
    g = x.astype(f) @ f64(W_ih).T + h.astype(f) @ f64(W_hh).T + b_ih.astype(f) + b_hh.astype(f)
    return g.reshape(len(x), 4, HID)


def lstm_cell(gates, c):
    i, f, g, o = (gates[:, j] for j in range(4))
    c2 = sigm(f) * c.astype(np.float64) + sigm(i) * np.tanh(g)
    return sigm(o) * np.tanh(c2), c2


def candidates(w, x0, h, c):
    """w: dict of row-major matrices; x0 [n][HID] = embed[prev_token]; h, c [n][2][HID] committed -> h' [n][2][HID], c' [n][2][HID], g [n][JNT]"""
    h0, c0 = lstm_cell(lstm_gates(w["w_ih0"], w["w_hh0"], w["b_ih0"], w["b_hh0"], x0, h[:, 0]), c[:, 0])
    h1, c1 = lstm_cell(lstm_gates(w["w_ih1"], w["w_hh1"], w["b_ih1"], w["b_hh1"], h0, h[:, 1]), c[:, 1])
    g = h1 @ f64(w["pred_w"]).T + w["pred_b"].astype(np.float64)
    return np.stack([h0, h1], 1), np.stack([c0, c1], 1), g


def joint(enc, g, out_w, out_b):
    """logits [n][VOCAB] of rows enc [n][JNT] against g [n][JNT]"""
    x = np.maximum(enc.astype(np.float64) + g.astype(np.float64), 0.0)
    return x @ f64(out_w).T + out_b.astype(np.float64)


# ---- the packed arg-max key: (order-preserving image of the f32 logit's bits) << 32 | (0xffffffff - index) -------------------------------------
def pack_key(v, idx):
    u = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xffffffff), u | np.uint64(0x80000000))
    return (u << np.uint64(32)) | (np.uint64(0xffffffff) - np.asarray(idx).astype(np.uint64))


def key_index(key):
    return (np.uint64(0xffffffff) - (np.asarray(key, np.uint64) & np.uint64(0xffffffff))).astype(np.int64)


def key_logit(key):
    u = (np.asarray(key, np.uint64) >> np.uint64(32)).astype(np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7fffffff), ~u).astype(np.uint32).view(np.float32)


def first_argmax(x):
    """index of the first maximum of every row"""
    return np.argmax(x, axis=-1)            # numpy returns the first occurrence


def n_parts(step_rows):
    return TILE_PARTS if step_rows <= SMALL_ROWS else WG_PARTS


def part_width(parts):
    return 16 if parts == TILE_PARTS else 64


def padded(logits, fill=-np.inf):
    n = logits.shape[0]
    out = np.full((n, 68 * 16), fill, np.float64)
    out[:, :VOCAB] = logits
    return out


def parts_of(logits, parts):
    """(m, s) [n][parts] of the slices of width 16 or 64: m = the slice's maximum, s = sum exp(x - m)"""
    w = part_width(parts)
    p = padded(logits)[:, :parts * w].reshape(len(logits), parts, w)
    m = p.max(-1)
    with np.errstate(invalid="ignore"):
        s = np.where(np.isfinite(m), np.exp(p - np.where(np.isfinite(m), m, 0.0)[..., None]).sum(-1), 0.0)
    return m, s


def log_softmax(logits):
    m = logits.max(-1, keepdims=True)
    return logits - (m + np.log(np.exp(logits - m).sum(-1, keepdims=True)))


def entropy(logits, alpha):
    lp = log_softmax(logits)
    p = np.exp(lp)
    if alpha == 1.0:
        return -(p * lp).sum(-1)
    return np.log((p ** alpha).sum(-1)) / (1.0 - alpha)


def ent_terms(logits, parts, alpha):
    """the entropy term beside every part: sum exp(x - m)(x - m) (alpha = 1) or sum exp(alpha (x - m)), m the part's maximum"""
    w = part_width(parts)
    p = padded(logits)[:, :parts * w].reshape(len(logits), parts, w)
    m = p.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        d = np.where(np.isfinite(p), p - np.where(np.isfinite(m), m, 0.0), -np.inf)
        t = np.where(np.isfinite(d), np.exp(d) * np.where(np.isfinite(d), d, 0.0), 0.0) if alpha == 1.0 else np.where(np.isfinite(d), np.exp(alpha * d), 0.0)
    return t.sum(-1)


def top_keys(values_f32, parts, k):
    """the k largest keys of every slice [n][parts][k], descending, 0 where the slice has fewer entries; values are the f32 numbers the keys are made of"""
    n = len(values_f32)
    w = part_width(parts)
    keys = np.zeros((n, parts * w), np.uint64)
    keys[:, :VOCAB] = pack_key(values_f32, np.arange(VOCAB)[None, :].repeat(n, 0))
    keys = np.sort(keys.reshape(n, parts, w), -1)[..., ::-1]
    return np.ascontiguousarray(keys[..., :k])


# ---- the work lists and one commit of one stream -------------------------------------------------------------------------------------------------
def build_lists(ctrl, slots):
    """ctrl [n_slots][12], slots [B] -> n_active, dlist (set), rowmap (set of frame << 16 | b)"""
    dl, rm, na = set(), set(), 0
    for b, s in enumerate(slots):
        ct = ctrl[s]
        if not ct[CT["active"]]:
            continue
        na += 1
        if ct[CT["dirty"]]:
            dl.add(b)
        for f in range(ct[CT["t"]], ct[CT["n_frames"]]):
            rm.add((f << 16) | b)
    return na, dl, rm


def commit_stream(ct, best_of_frame):
    """one commit of one ACTIVE stream.  ct: its control block (a dict, changed in place); best_of_frame(f) -> arg-max of frame f this iteration.
    Returns (token or None, frame of the token, first frame left, one past the last frame left): blanks are skipped with the state untouched, the first
    non-blank is emitted at its frame; the frame is left when it has MAX_SYMBOLS symbols; `symbols` counts the symbols of the current frame only."""
    t0, nf = ct["t"], ct["n_frames"]
    f = t0
    while f < nf and best_of_frame(f) == BLANK:
        f += 1
    if f == nf:
        ct["iterations"] += nf - t0
        ct.update(t=nf, symbols=0, active=0)
        return None, None, t0, nf
    tok = best_of_frame(f)
    ct["iterations"] += f - t0 + 1
    sym = (ct["symbols"] if f == t0 else 0) + 1
    ct["n_tok"] += 1
    ct["prev_token"] = tok
    ct["cur"] ^= 1
    ct["dirty"] = 1
    t = f
    if sym >= MAX_SYMBOLS:
        t, sym = f + 1, 0
    ct.update(t=t, symbols=sym)
    if t >= nf:
        ct["active"] = 0
    return tok, f, t0, t


def greedy_stream(w, enc, n_dec, h, c, prev_token, symbols=0, bonus=None):
    """the reference's per-stream loop in float64: enc [T][JNT] (joint.enc applied), h, c [2][HID].  Returns tokens, frames, iterations, h, c, prev_token,
    symbols, and the smallest margin of an arg-max over its runner-up along the trajectory with the logits of every evaluation [(frame, logits)]"""
    toks, frames, evals, it = [], [], [], 0
    t = 0
    while t < n_dec:
        x0 = w["embed"][prev_token][None].astype(np.float64)
        h2, c2, g = candidates(w, x0, h[None], c[None])
        lg = joint(enc[t][None], g, w["out_w"], w["out_b"])[0]
        it += 1
        evals.append((t, lg))
        v = lg + (bonus if bonus is not None else 0.0)
        best = int(first_argmax(v))
        if best == BLANK:
            t, symbols = t + 1, 0
            continue
        toks.append(best)
        frames.append(t)
        prev_token, h, c = best, h2[0], c2[0]
        symbols += 1
        if symbols >= MAX_SYMBOLS:
            t, symbols = t + 1, 0
    return toks, frames, it, h, c, prev_token, symbols, evals
