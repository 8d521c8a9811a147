"""The cases of tests/test_gpu_decode_kernels.py: layouts, operands, poison, expectations and the terms of the bounds, numpy only.
tests/test_decode_kernel_ref.py checks them without a GPU (the exact-mode expectations against tests/decode_ref.py, every margin and cap condition)."""
from __future__ import annotations

import zlib

import numpy as np

from tests import decode_ref as DR
from tests.decode_ref import BLANK, COLS, CT, DEC_CTRL, HID, JNT, VOCAB

U24 = 2.0 ** -24
SENT_U32 = np.uint32(0xFFC5FFC5)            # the sentinel as a 32-bit pattern: NaN as f32, -3801147 as i32
POOL = 136                                  # decoder slots of the candidate cases
ND_SWEEP = (1, 16, 17, 32, 33, 64, 65, 80, 97, 130)
SMALL_ROWS_SWEEP = (1, 15, 16, 17, 32, 33, 48, 49, 64)
TILED_ROWS_SWEEP = (1, 63, 64, 65, 80, 81, 127, 128, 129, 200)
ENCPROJ_M = (1, 16, 17, 63, 64, 65, 130)
# (K, N) of every launch_encproj call site: nasr_encoder.hip (D, JNT); nasr_diar.hip: the SE gates (cout, cout / 8) and (cout / 8, cout) of the TitaNet
# blocks, cout = 1024 and 3072, and the embedding (2 SPK_C, SPK_EMB)
ENCPROJ_SITES = ((1024, 640), (1024, 128), (128, 1024), (3072, 384), (384, 3072), (6144, 192))
LSTM_CONFIGS = ("g", "f", "i", "o")         # the gate that is held fixed in an exact LSTM run (the other three vary per unit and per k read)
# ties of the row maximum, by what the pair spans (lane (q, j) of vocab tile nt holds entry 16 nt + 4 q + j; the tiled kernel's workgroup x holds
# tiles 4x .. 4x + 3, one per wave).  The last kind lets blank win alone
TIES = ((5, 6), (9, 13), (18, 26), (100, 116), (200, 264), (15, 16), (63, 64), (1023, 1024), (0, 1024), (1024,))
TIE_SPANS = ("one lane", "two lane groups (xor 16)", "two lane groups (xor 32)", "two tiles: workgroups of k_dec_joint, waves of k_dec_joint_tiled",
             "two workgroups of k_dec_joint_tiled", "tile border", "workgroup border", "last token against blank", "token 0 against blank", "blank alone")
TIE_GROUPS = ((5, 6), (9, 13), (18, 26), (100, 116), (200, 264), (15, 16), (63, 64), (0, 1023, 1024))      # rows of out_w that are equal outside the selector columns
SEL0 = JNT - len(TIES)                      # selector column of tie kind j: SEL0 + j
SEL_BIG = 4096.0


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def sent(shape, dtype=np.float32):
    return np.full(shape, SENT_U32, np.uint32).view(dtype)


# ---- weights ------------------------------------------------------------------------------------------------------------------------------------
def exact_weights(cfg="g"):
    """integers: every LSTM pre-activation is 0 (gate g only), >= +32 or <= -128; every projection and logit is an exact integer below 2^24"""
    r = rng_of("exact weights", cfg)
    w = {}
    embed = np.zeros((VOCAB, HID), np.float32)
    tok = np.arange(VOCAB)
    embed[tok, (tok * 37) % HID] = 1 + tok // HID                       # one-hot: token -> (column, value)
    w["embed"] = embed
    for L in range(2):
        A = r.integers(-1, 2, (4, HID, HID)).astype(np.float32) * 512
        Bm = r.integers(-1, 2, (4, HID, HID)).astype(np.float32) * 1024
        b_ih = np.full((4, HID), -200, np.float32)
        b_hh = np.full((4, HID), -100, np.float32)
        b_ih[2] = b_hh[2] = 0                                           # gate g: 0 or saturated
        j = "ifgo".index(cfg)
        A[j] = Bm[j] = 0
        if cfg == "f":
            b_ih[1], b_hh[1] = 200, 100                                 # held open
        w[f"w_ih{L}"], w[f"w_hh{L}"] = A.reshape(4 * HID, HID), Bm.reshape(4 * HID, HID)
        w[f"b_ih{L}"], w[f"b_hh{L}"] = b_ih.reshape(-1), b_hh.reshape(-1)
    w["pred_w"] = r.integers(-2, 3, (JNT, HID)).astype(np.float32)
    w["pred_b"] = r.integers(-4, 5, JNT).astype(np.float32)
    ow = r.integers(-2, 3, (VOCAB, JNT)).astype(np.float32)
    ob = r.integers(-8, 9, VOCAB).astype(np.float32)
    for grp in TIE_GROUPS:
        ow[list(grp[1:])] = ow[grp[0]]
        ob[list(grp[1:])] = ob[grp[0]]
    ow[:, SEL0:] = 0
    for j, tie in enumerate(TIES):
        ow[list(tie), SEL0 + j] = 2
    w["out_w"], w["out_b"] = ow, ob
    return w


def bounded_weights(seed=0):
    r = rng_of("bounded weights", seed)
    f = np.float32
    w = {"embed": r.standard_normal((VOCAB, HID)).astype(f)}
    for L in range(2):
        w[f"w_ih{L}"] = (r.standard_normal((4 * HID, HID)) * 0.06).astype(f)
        w[f"w_hh{L}"] = (r.standard_normal((4 * HID, HID)) * 0.06).astype(f)
        w[f"b_ih{L}"] = (r.standard_normal(4 * HID) * 0.5).astype(f)
        w[f"b_hh{L}"] = (r.standard_normal(4 * HID) * 0.5).astype(f)
    w["pred_w"] = (r.standard_normal((JNT, HID)) * 0.08).astype(f)
    w["pred_b"] = (r.standard_normal(JNT) * 0.3).astype(f)
    w["out_w"] = (r.standard_normal((VOCAB, JNT)) * 0.05).astype(f)
    w["out_b"] = (r.standard_normal(VOCAB) * 0.3).astype(f)
    return w


CHAIN_LIVE = 4            # vocabulary entries of the chained cases that compete with blank


def chain_weights(seed=0):
    """the chained cases' weights.  The issue's bounds carry an error through a matrix as |W| e, so a dense random layer multiplies it by its absolute row sum
    (about 30 here) three times over; these matrices are sparse (16 entries a row), and the ones an error comes back through with every symbol (w_hh, w_ih of
    layer 1) have an absolute row sum of about 0.5, which keeps the bound carried along a whole trajectory near the rounding it starts from.  CHAIN_LIVE tokens and blank have full-size output rows, the rest 1 / 50 of that: an arg-max is a contest of 5"""
    r = rng_of("chain weights", seed)
    f = np.float32

    def sparse(n, k, scale):
        m = np.zeros((n, k), f)
        cols = np.argsort(r.random((n, k)), 1)[:, :16]
        m[np.arange(n)[:, None], cols] = (r.standard_normal((n, 16)) * scale).astype(f)
        return m

    w = {"embed": r.standard_normal((VOCAB, HID)).astype(f)}
    for L in range(2):
        w[f"w_ih{L}"], w[f"w_hh{L}"] = sparse(4 * HID, HID, 0.25 if L == 0 else 0.04), sparse(4 * HID, HID, 0.04)
        w[f"b_ih{L}"], w[f"b_hh{L}"] = (r.standard_normal(4 * HID) * 0.3).astype(f), (r.standard_normal(4 * HID) * 0.3).astype(f)
    w["pred_w"], w["pred_b"] = sparse(JNT, HID, 0.15), (r.standard_normal(JNT) * 0.3).astype(f)
    ow = sparse(VOCAB, JNT, 0.5)
    live = np.concatenate([r.permutation(BLANK)[:CHAIN_LIVE], [BLANK]])
    quiet = np.ones(VOCAB, bool)
    quiet[live] = False
    ow[quiet] *= f(0.02)
    w["out_w"] = ow
    ob = np.zeros(VOCAB, f)
    ob[BLANK] = 1.0
    w["out_b"] = ob
    return w


# ---- the decoder state of a case ----------------------------------------------------------------------------------------------------------------------
def ctrl_rows(n):
    return np.zeros((n, len(DEC_CTRL)), np.int32)


def base_state(B, T, pool, seed, n_dec=None):
    """rows / ctrl / h / c / predg / lists of B streams on a pool of `pool` slots: rows[b].slot a permutation into the pool, every value of an unused slot
    the sentinel, every index a kernel may read in range"""
    r = rng_of("state", B, T, pool, seed)
    assert pool > B
    slots = r.permutation(pool)[:B]
    rows = np.zeros((B, 8), np.int32)
    rows[:, 0] = slots
    rows[:, 5] = T if n_dec is None else n_dec
    rows[:, 6] = -1
    st = {"B": B, "T": T, "pool": pool, "slots": slots, "rows": rows}
    ctrl = sent((pool, len(DEC_CTRL)), np.int32)
    ct = ctrl_rows(B)
    ct[:, CT["prev_token"]] = r.integers(0, VOCAB, B)
    ct[:, CT["cur"]] = r.integers(0, 2, B)
    ct[:, CT["n_frames"]] = rows[:, 5]
    ct[:, CT["row"]] = np.arange(B)
    ct[:, CT["n_tok"]] = r.integers(0, 50, B)
    ct[:, CT["iterations"]] = r.integers(0, 1000, B)
    ct[:, CT["frame0"]] = r.integers(0, 10000, B)
    ct[:, CT["frame_next"]] = ct[:, CT["frame0"]] + rows[:, 5]
    ctrl[slots] = ct
    st["ctrl"] = ctrl
    st["h"], st["c"], st["predg"] = sent((pool, 2, 2, HID)), sent((pool, 2, 2, HID)), sent((pool, JNT))
    st["encproj"] = sent((B * T, JNT))
    st["key"] = np.zeros(B * T, np.uint64)
    st["counters"] = np.zeros(3, np.int32)
    st["dlist"] = r.permutation(B).astype(np.int32)
    st["rowmap"] = np.zeros(B * T, np.uint32)
    st["tok_ring"], st["tok_frame"] = sent((pool, DR.TOK_CAP), np.int32), sent((pool, DR.TOK_CAP), np.int32)
    return st


def c_tags(pool):
    """c [slot][version][layer][unit] = +-4 (2048 + flat index): integers that name their place, |c| >= 8192 so tanhf(c) is exactly +-1"""
    idx = np.arange(pool * 4 * HID).reshape(pool, 2, 2, HID)
    sign = 1 - 2 * ((idx * 2654435761 >> 7) & 1)
    return (sign * 4 * (2048 + idx)).astype(np.float32)


# ---- candidates (k_dec_lstm<0>, k_dec_lstm<1>, k_dec_pred) --------------------------------------------------------------------------------------
def candidate_case(nd, exact, seed=0, B=None):
    """B streams of which the first nd entries of dlist are dirty; the others' state, both versions, must come back bit for bit"""
    B = B if B is not None else min(POOL - 2, nd + 5)
    st = base_state(B, 1, POOL, ("cand", nd, exact, seed))
    r = rng_of("cand", nd, exact, seed)
    slots, ctrl = st["slots"], st["ctrl"]
    cur = ctrl[slots, CT["cur"]]
    if exact:
        st["c"][slots] = c_tags(POOL)[slots]
        h = np.zeros((B, 2, 2, HID), np.float32)
        for L in range(2):
            h[np.arange(B), cur, L, (slots * 53 + L * 17 + 3) % HID] = 1            # the committed version: one-hot
            h[np.arange(B), cur ^ 1, L, (slots * 29 + L * 5 + 1) % HID] = 7         # the other one: a loud one-hot, overwritten for dirty streams
        st["h"][slots] = h
    else:
        st["h"][slots] = r.uniform(-1, 1, (B, 2, 2, HID)).astype(np.float32)
        st["c"][slots] = r.uniform(-2, 2, (B, 2, 2, HID)).astype(np.float32)
    st["predg"][slots] = r.integers(-9, 10, (B, JNT)).astype(np.float32)
    dirty = st["dlist"][:nd]
    poison = np.zeros(B, bool)
    poison[dirty] = True
    for name in ("h", "c"):                                                         # what the launch must overwrite starts as the sentinel
        v = st[name][slots]
        v[poison, cur[poison] ^ 1] = sent((int(poison.sum()), 2, HID))
        st[name][slots] = v
    pg = st["predg"][slots]
    pg[poison] = sent((int(poison.sum()), JNT))
    st["predg"][slots] = pg
    st["counters"][:] = (B, nd, 0)
    st["nd"], st["dirty"] = nd, dirty
    return st


def candidate_inputs(st, w):
    """x0, h, c (committed) of the dirty streams in dlist order"""
    d = st["dirty"]
    s = st["slots"][d]
    cur = st["ctrl"][s, CT["cur"]]
    x0 = w["embed"][st["ctrl"][s, CT["prev_token"]]]
    return s, cur, x0, st["h"][s, cur], st["c"][s, cur]


def exact_cell(pre, c):
    """the cell update where every pre-activation saturates: sigm is exactly 0 or 1, tanhf exactly 0 or +-1.  Returns h', c' and what the rule needs to hold"""
    ok = bool(np.all((pre >= 32) | (pre <= -128) | (pre == 0))) and bool(np.all(pre[:, [0, 1, 3]] != 0))
    si, sf, so = ((pre[:, j] >= 32).astype(np.float64) for j in (0, 1, 3))
    tg = np.sign(pre[:, 2])
    c2 = sf * c.astype(np.float64) + si * tg
    ok = ok and bool(np.all((np.abs(c2) >= 32) | (c2 == 0) | (so == 0)))           # tanhf(c') is exact wherever h' shows it
    return so * np.sign(c2), c2, ok


def exact_candidates(w, x0, h, c):
    pre0 = DR.lstm_gates(w["w_ih0"], w["w_hh0"], w["b_ih0"], w["b_hh0"], x0, h[:, 0])
    h0, c0, ok0 = exact_cell(pre0, c[:, 0])
    pre1 = DR.lstm_gates(w["w_ih1"], w["w_hh1"], w["b_ih1"], w["b_hh1"], h0, h[:, 1])
    h1, c1, ok1 = exact_cell(pre1, c[:, 1])
    g = h1 @ w["pred_w"].astype(np.float64).T + w["pred_b"]
    ok = ok0 and ok1 and max(np.abs(pre0).max(), np.abs(pre1).max()) < 2 ** 24 and np.abs(c0).max() < 2 ** 24
    return np.stack([h0, h1], 1), np.stack([c0, c1], 1), g, ok, (pre0, pre1)


def gate_bound(W_ih, W_hh, b_ih, b_hh, x, h, ex=None, eh=None):
    """(1280 + 8) u (|W_ih| |x| + |W_hh| |h| + |b_ih| + |b_hh|); inputs known only to ex / eh add |W_ih| ex + |W_hh| eh"""
    f = np.float64
    a = np.abs(x).astype(f) @ DR.f64(W_ih, True).T + np.abs(h).astype(f) @ DR.f64(W_hh, True).T + np.abs(b_ih).astype(f) + np.abs(b_hh).astype(f)
    e = (2 * HID + 8) * U24 * a
    if ex is not None:
        e = e + ex @ DR.f64(W_ih, True).T
    if eh is not None:
        e = e + eh @ DR.f64(W_hh, True).T
    return e.reshape(len(x), 4, HID)


def cell_bound(gates, eg, c, sigm_rel, tanhf_rel, ec_in=0.0):
    """first-order error of (h', c') from pre-activations known to eg: sigm has slope <= 1/4, tanh slope <= 1; products and sums round at u"""
    si, sf, so = (DR.sigm(gates[:, j]) for j in (0, 1, 3))
    e_si, e_sf, e_so = (eg[:, j] / 4 + sigm_rel * s for j, s in ((0, si), (1, sf), (3, so)))
    tg = np.tanh(gates[:, 2])
    e_tg = eg[:, 2] + tanhf_rel * np.abs(tg)
    c = c.astype(np.float64)
    c2 = sf * c + si * tg
    e_c = e_sf * np.abs(c) + e_si * np.abs(tg) + si * e_tg + 3 * U24 * (np.abs(sf * c) + np.abs(si * tg)) + sf * ec_in
    tc = np.tanh(c2)
    e_tc = e_c + tanhf_rel * np.abs(tc)
    e_h = e_so * np.abs(tc) + so * e_tc + 2 * U24 * np.abs(so * tc)
    return e_h, e_c


def candidate_bounds(w, x0, h, c, sigm_rel, tanhf_rel, eh=None, ec=None):
    """reference (h', c', g) and the bound of each element; eh, ec [n][2][HID]: what the committed state is known to (chained calls)"""
    eh_ = (lambda L: None) if eh is None else (lambda L: eh[:, L])
    ec_ = (lambda L: 0.0) if ec is None else (lambda L: ec[:, L])
    g0 = DR.lstm_gates(w["w_ih0"], w["w_hh0"], w["b_ih0"], w["b_hh0"], x0, h[:, 0])
    eh0, ec0 = cell_bound(g0, gate_bound(w["w_ih0"], w["w_hh0"], w["b_ih0"], w["b_hh0"], x0, h[:, 0], eh=eh_(0)), c[:, 0], sigm_rel, tanhf_rel, ec_(0))
    h0, c0 = DR.lstm_cell(g0, c[:, 0])
    g1 = DR.lstm_gates(w["w_ih1"], w["w_hh1"], w["b_ih1"], w["b_hh1"], h0, h[:, 1])
    eh1, ec1 = cell_bound(g1, gate_bound(w["w_ih1"], w["w_hh1"], w["b_ih1"], w["b_hh1"], h0, h[:, 1], ex=eh0, eh=eh_(1)), c[:, 1], sigm_rel, tanhf_rel, ec_(1))
    h1, c1 = DR.lstm_cell(g1, c[:, 1])
    aw = DR.f64(w["pred_w"], True)
    g = h1 @ DR.f64(w["pred_w"]).T + w["pred_b"]
    eg = (HID + 4) * U24 * (np.abs(h1) @ aw.T + np.abs(w["pred_b"])) + eh1 @ aw.T
    return (np.stack([h0, h1], 1), np.stack([c0, c1], 1), g), (np.stack([eh0, eh1], 1), np.stack([ec0, ec1], 1), eg)


# ---- encproj ---------------------------------------------------------------------------------------------------------------------------------------
def encproj_case(M, K, N, exact, seed=0):
    r = rng_of("encproj", M, K, N, exact, seed)
    if exact:
        x = r.integers(-4, 5, (M, K)).astype(np.float32)
        W = r.integers(-2, 3, (N, K)).astype(np.float32)
        W[:, np.arange(K) % 64 == 63] = 2                           # the last k-group of every 64 counts in every output
        b = r.integers(-8, 9, N).astype(np.float32)
    else:
        x = r.standard_normal((M, K)).astype(np.float32)
        W = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
        b = r.standard_normal(N).astype(np.float32)
    f = np.float64
    ref = x.astype(f) @ W.astype(f).T + b
    bound = (K + 4) * U24 * (np.abs(x).astype(f) @ np.abs(W).astype(f).T + np.abs(b))
    return x, W, b, ref, bound


# ---- the joint kernels --------------------------------------------------------------------------------------------------------------------------------
def joint_layout(B, T, n_rows, seed, ragged):
    """n_dec and t of every stream so that sum (n_dec - t) = n_rows: ragged: n_dec random below T; the rest of the rows counts as already decoded"""
    r = rng_of("layout", B, T, n_rows, seed, ragged)
    assert n_rows <= B * T
    n_dec = np.full(B, T)
    if ragged:
        n_dec = r.integers(0, T + 1, B)
        while n_dec.sum() < n_rows:
            n_dec[r.integers(0, B)] = T
    t = np.zeros(B, np.int64)
    extra = int(n_dec.sum()) - n_rows
    while extra > 0:
        b = r.integers(0, B)
        if t[b] < n_dec[b]:
            t[b] += 1
            extra -= 1
    return n_dec.astype(np.int32), t.astype(np.int32)


def joint_case(B, T, n_rows, exact, seed=0, ragged=False, pool=None, n_states=4):
    """a joint-alone call: n_active = n_dirty = 0, n_rows planted; rowmap = the frames [t, n_dec) of every stream in a shuffled order, the entries behind
    n_rows valid (the clamped lanes read entry i0 only, but no entry may be able to fault).  encproj rows of frames >= n_dec are the sentinel"""
    n_dec, t = joint_layout(B, T, n_rows, seed, ragged)
    pool = pool if pool is not None else B + 3
    st = base_state(B, T, pool, ("joint", B, T, n_rows, exact, seed), n_dec=n_dec)
    r = rng_of("joint", B, T, n_rows, exact, seed, ragged)
    slots = st["slots"]
    st["ctrl"][slots, CT["t"]] = t
    st["ctrl"][slots, CT["active"]] = (t < n_dec)
    pairs = [(f << 16) | b for b in range(B) for f in range(t[b], n_dec[b])]
    assert len(pairs) == n_rows
    rm = np.array(pairs, np.uint32)[r.permutation(n_rows)] if n_rows else np.zeros(0, np.uint32)
    fill = np.array([(f << 16) | b for b in range(B) for f in range(T)], np.uint32)
    st["rowmap"] = np.concatenate([rm, fill[r.integers(0, B * T, B * T - n_rows)]]).astype(np.uint32)
    st["counters"][:] = (0, 0, n_rows)
    st["n_rows"], st["rm"] = n_rows, rm
    rb, rf = (rm & 0xffff).astype(np.int64), (rm >> 16).astype(np.int64)
    st["rb"], st["rf"], st["ki"] = rb, rf, rb * T + rf
    # keys: 0 where the launch evaluates (atomicMax), a tag elsewhere
    key = (np.uint64(0x7777000000000000) + np.arange(B * T).astype(np.uint64))
    key[st["ki"]] = 0
    st["key"] = key
    valid = np.zeros((B, T), bool)
    for b in range(B):
        valid[b, :n_dec[b]] = True
    valid = valid.reshape(-1)
    enc = sent((B * T, JNT))
    if exact:
        kind = r.integers(0, len(TIES) + 3, B * T)                  # kinds >= len(TIES): no selector, the natural first maximum (ties happen among integers)
        if n_rows >= len(TIES):
            kind[st["ki"][:len(TIES)]] = np.arange(len(TIES))       # every kind at least once among the evaluated rows
        e = r.integers(-3, 4, (B * T, JNT)).astype(np.float32)
        e[:, SEL0:] = -SEL_BIG
        for j in range(len(TIES)):
            e[kind == j, SEL0 + j] = SEL_BIG
        g = r.integers(-3, 4, (pool, JNT)).astype(np.float32)
        g[:, SEL0:] = 0
        st["kind"] = kind
    else:
        e = r.standard_normal((B * T, JNT)).astype(np.float32)
        g = r.standard_normal((pool, JNT)).astype(np.float32)
    enc[valid] = e[valid]
    st["encproj"] = enc
    st["predg"][slots] = g[slots]
    st["h"][slots] = r.integers(-9, 10, (B, 2, 2, HID)).astype(np.float32)      # not read by a joint-alone call: must come back bit for bit
    st["c"][slots] = r.integers(-9, 10, (B, 2, 2, HID)).astype(np.float32)
    # bias tables (used by the forms that take them)
    bon = np.zeros((n_states, COLS), np.float32)
    bon[1:, :BLANK] = (r.integers(0, 4, (n_states - 1, BLANK)) * (r.random((n_states - 1, BLANK)) < 0.05)).astype(np.float32)
    if exact:
        bon[2, [6, 13, 116, 264, 16, 64]] = 1                       # state 2 turns the planted ties over: the second entry wins by its bonus
        bon[3, [5, 9, 100, 200, 15, 63, 1023]] = 3
    else:
        bon[1:] *= 0.25
    st["boost_bonus"] = bon
    nxt = r.integers(0, n_states, (n_states, COLS)).astype(np.int32)
    st["boost_next"] = nxt
    bs = sent(pool, np.int32)
    bs[:] = r.integers(0, n_states, pool)                           # an index: every slot's state is in range, the unused ones too
    st["boost_state"] = bs
    lm_row = sent((pool, COLS))
    lr = np.zeros((B, COLS), np.float32)
    lr[:, :BLANK] = -r.integers(0, 4, (B, BLANK)) * (r.random((B, BLANK)) < 0.3) * (1.0 if exact else 0.25)
    if exact:
        lr[::2, [5, 9, 100, 200, 15, 63, 1023, 0]] = -1             # every other slot turns the planted ties over
    lm_row[slots] = lr
    st["lm_row"] = lm_row
    return st


def joint_logits(st, w):
    """float64 logits [n_rows][VOCAB] of the evaluated rows in rowmap order"""
    return DR.joint(st["encproj"][st["ki"]], st["predg"][st["slots"][st["rb"]]], w["out_w"], w["out_b"])


def joint_bias(st, form):
    """the bias rows [n_rows][VOCAB] the arg-max key of a form adds (None: the plain key)"""
    s = st["slots"][st["rb"]]
    if form.get("LMF"):
        return st["lm_row"][s][:, :VOCAB].astype(np.float64)
    if form.get("BOOST"):
        return st["boost_bonus"][st["boost_state"][s]][:, :VOCAB].astype(np.float64)
    return None


def logit_bound(st, w):
    """(640 + 4) u (|W_out| x + |b|) + |W_out| (u |e + g|), x = relu(e + g)"""
    f = np.float64
    e, g = st["encproj"][st["ki"]].astype(f), st["predg"][st["slots"][st["rb"]]].astype(f)
    aw = np.abs(w["out_w"]).astype(f)
    return (JNT + 4) * U24 * (np.maximum(e + g, 0) @ aw.T + np.abs(w["out_b"])) + (U24 * np.abs(e + g)) @ aw.T


def plant_winners(st, w, seed=0, gain=12.0, blank_share=0.0):
    """bounded mode: every evaluated row gets a winner lifted over its runner-up -- enc[row] moves along relu-visible columns of out_w[winner].
    Returns the winners; the margin condition is asserted by the caller against logit_bound"""
    r = rng_of("winners", seed, st["n_rows"])
    win = r.integers(0, VOCAB, st["n_rows"])
    win[r.random(st["n_rows"]) < blank_share] = BLANK
    enc = st["encproj"]
    for i, ki in enumerate(st["ki"]):
        d = w["out_w"][win[i]].astype(np.float64)
        enc[ki] = (enc[ki].astype(np.float64) + gain * d / np.dot(d, d) * 2.0).astype(np.float32)
    return win


def margins(values):
    """winner's value minus the runner-up's, per row"""
    s = np.sort(values, -1)
    return s[:, -1] - s[:, -2]


# ---- the launch rules, restated ----------------------------------------------------------------------------------------------------------------------
def tf(*flags):
    return ",".join("true" if f else "false" for f in flags)


def joint_kernel(rows, LP=False, BOOST=False, ALT=False, LMF=False, ENT=False, BEAMB=False, beam=False):
    """launch_joint_commit / launch_decode_rows / launch_decode_rows_boost: B * T <= 64 takes k_dec_joint, the beam calls always the tiled kernel"""
    if beam:
        return f"k_dec_joint_tiled<{tf(True, BEAMB, True, BEAMB)}>" if BEAMB else "k_dec_joint_tiled<true,false,true>"
    if rows <= DR.SMALL_ROWS:
        return f"k_dec_joint<{tf(LP, BOOST, ALT, LMF, ENT)}>"
    return f"k_dec_joint_tiled<{tf(LP, BOOST, ALT, False, LMF, ENT)}>"


def commit_kernel(LP=False, BOOST=False, ALT=False, FB=False, LMF=False, ENT=False):
    return f"k_dec_commit<{tf(LP, BOOST, ALT, FB, LMF, ENT)}>"


def greedy_forms():
    """every (LP, BOOST, ALT, LMF, ENT, FB) launch_decode_iter can reach: lm_row -> LMF + BOOST; alt_key -> LP + ALT; ent_part, frame_blank ride on LP"""
    out = []
    for LMF in (False, True):
        for BOOST in ((True,) if LMF else (False, True)):
            for LP, ALT in ((False, False), (True, False), (True, True)):
                for ENT in ((False, True) if LP else (False,)):
                    for FB in ((False, True) if LP else (False,)):
                        out.append(dict(LP=LP, BOOST=BOOST, ALT=ALT, LMF=LMF, ENT=ENT, FB=FB))
    return out


def joint_forms():
    seen, out = set(), []
    for f in greedy_forms():
        k = (f["LP"], f["BOOST"], f["ALT"], f["LMF"], f["ENT"])
        if k not in seen:
            seen.add(k)
            out.append({n: v for n, v in f.items() if n != "FB"})
    return out


PLAIN = dict(LP=False, BOOST=False, ALT=False, LMF=False, ENT=False)
RICH = dict(LP=True, BOOST=True, ALT=True, LMF=False, ENT=True)
RICH_LMF = dict(LP=True, BOOST=True, ALT=True, LMF=True, ENT=True)


def form_id(f):
    return "+".join(n for n in ("LP", "BOOST", "ALT", "LMF", "ENT", "FB", "BEAMB") if f.get(n)) or "plain"
