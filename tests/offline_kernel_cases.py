"""The cases of tests/test_gpu_offline_kernels.py, numpy only (no GPU, no library): packed layouts, the selector-mode operands with the expectation computed from
the definition, the bounded-mode attention operands with their float64 reference and the terms of the bound, and the conv0 + dw batch with its reference,
bound and float32 restatement.  tests/test_offline_kernel_ref.py checks them with the references alone; the conventions are stated in the GPU test's docstring."""
from __future__ import annotations

import zlib

import numpy as np

from tests import gemm_ref as R
from tests import offline_kernel_ref as OR

D, NH, DH, MAX_T, NREL, QKV_LD, SUBC, NMEL = 1024, 8, 128, 2048, 4095, 3072, 256, 128
U24 = 2.0 ** -24


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ==== attention =================================================================================================================================
class Packed:
    """utterances of Ts frames packed back to back, as the driver packs them"""

    def __init__(self, Ts):
        self.Ts = [int(t) for t in Ts]
        self.offs = [int(x) for x in np.concatenate([[0], np.cumsum(self.Ts)[:-1]])]
        self.M = int(sum(self.Ts))
        self.utt = np.repeat(np.arange(len(self.Ts)), self.Ts)             # utterance of packed row m
        self.frame = np.concatenate([np.arange(t) for t in self.Ts])       # its frame there: the driver's tpos

    def items(self, qb, only=None):
        """the driver's work items: for every utterance, one (off, T, q0, 0) per qb query rows"""
        return np.array([(off, T, q0, 0) for k, (off, T) in enumerate(zip(self.offs, self.Ts)) if only is None or k in only
                         for q0 in range(0, T, qb)], np.int32).reshape(-1, 4)

    def rows_of(self, only=None):
        return np.isin(self.utt, np.arange(len(self.Ts)) if only is None else list(only))


def v_marks(lay: Packed):
    """V[m][column]: small integers (exact in bf16) that name (utterance, frame, column); two frames below 2048 differ on the even or on the odd columns"""
    k, t, d = lay.utt[:, None], lay.frame[:, None], np.arange(D)[None, :]
    even = (t % 251 + 11 * d + 101 * k) % 255 - 127
    odd = ((t // 8) * 37 + 11 * d + 101 * k) % 255 - 127
    return np.where(d % 2 == 0, even, odd).astype(np.float32)


def _place(rank, where, value):
    """swap so that rank[where] == value (rank stays a permutation)"""
    j = int(np.flatnonzero(rank == value)[0])
    rank[j], rank[where] = rank[where], rank[j]


CONTENT_TARGETS = ("first_rows", "last_rows", "key63", "key64")
POSITION_TARGETS = ("rel_plus", "rel_zero", "rel_minus")


def selector_ranks(lay: Packed, run, seed, target):
    """content: [8][M] rank of every packed row; position: [8][4095] rank of every table row"""
    rng = rng_of("off-ranks", tuple(lay.Ts), run, seed, target)
    n = len(lay.Ts)
    if run == "content":
        rank = np.stack([rng.permutation(lay.M) for _ in range(NH)])
        for h in range(NH):
            for k, (off, T) in enumerate(zip(lay.offs, lay.Ts)):
                if target == "first_rows":                                   # rising with k: row off + T outranks every key of utterance k
                    _place(rank[h], off, lay.M - n + k)
                elif target == "last_rows":                                  # falling with k: row off - 1 outranks every key of utterance k
                    _place(rank[h], off + T - 1, lay.M - 1 - k)
                elif target in ("key63", "key64") and T > int(target[3:]):  # the utterance's own top rank onto that key
                    _place(rank[h], off + int(target[3:]), int(rank[h, off:off + T].max()))
        return rank
    rank = np.stack([rng.permutation(NREL) for _ in range(NH)])
    # longest first: row 2048 - T (2046 + T) is reached by the utterances of at least T frames, at j - i = -(T - 1) (T - 1), so of the rows an utterance reaches
    # its own carries the highest rank: its query T - 1 selects key 0 under rel_plus, its query 0 key T - 1 under rel_minus
    Ts = sorted(set(lay.Ts), reverse=True)
    rows = {None: [], "rel_plus": [MAX_T - T for T in Ts], "rel_zero": [MAX_T - 1], "rel_minus": [MAX_T - 2 + T for T in Ts]}[target]
    for h in range(NH):
        for x, r in enumerate(dict.fromkeys(rows)):
            _place(rank[h], r, NREL - 1 - x)
    return rank


def rank_columns(rank):
    """rho = a + 256 b -> (64 a, 16384 b)"""
    return 64.0 * (rank % 256), 16384.0 * (rank // 256)


def selector_case(lay: Packed, run, seed, target=None):
    """-> (qkv values [M][3072], pos values [4095][1024], bias_u, bias_v, expected ctx [M][1024])"""
    assert lay.M <= 4096
    rank = selector_ranks(lay, run, seed, target)
    qkv, pos = np.zeros((lay.M, QKV_LD), np.float32), np.zeros((NREL, D), np.float32)
    V = v_marks(lay)
    qkv[:, 2 * D:] = V
    bu, bv = np.zeros(D, np.float32), np.zeros(D, np.float32)
    bu[0::DH], bu[2::DH], bv[1::DH], bv[3::DH] = 32.0, 32.0, 32.0, 32.0
    exp = np.zeros((lay.M, D), np.float32)
    for h in range(NH):
        sl = slice(h * DH, (h + 1) * DH)
        if run == "content":
            qkv[:, D + h * DH], qkv[:, D + h * DH + 2] = rank_columns(rank[h])
        else:
            pos[:, h * DH + 1], pos[:, h * DH + 3] = rank_columns(rank[h])
        for off, T in zip(lay.offs, lay.Ts):
            if run == "content":                                             # the same key for every query: the highest rank among the utterance's own T keys
                win = np.full(T, int(np.argmax(rank[h, off:off + T])))
            else:                                                            # query i, key j: table row j - i + 2047
                i, j = np.arange(T)[:, None], np.arange(T)[None, :]
                win = np.argmax(rank[h][j - i + (MAX_T - 1)], axis=1)
            exp[off:off + T, sl] = V[off + win, sl]
    return qkv, pos, bu, bv, exp


BOUNDED_NEIGHBOURS = {1: (3, 1), 2: (1, 2), 15: (64, 3), 16: (5, 1), 17: (2, 65), 63: (1, 1), 64: (7, 3), 65: (16, 2), 129: (3, 5), 200: (1, 4)}


def bounded_rows(T):
    """the query rows compared at T: all, or at 2048 the first and the last query block of the bf16 kernel and 64 random rows"""
    if T < MAX_T:
        return np.arange(T)
    mid = rng_of("rows", T).choice(np.arange(64, T - 64), 64, replace=False)
    return np.sort(np.concatenate([np.arange(64), mid, np.arange(T - 64, T)]))


def bounded_case(T, bf16):
    """-> (layout, index of the utterance under test, qkv values, pos values, bias_u, bias_v, rows compared, ref [rows][1024], Delta_i [rows][8],
    sum_j w_j |V_jd| [rows][1024]); `attention_bound` makes the bound of them"""
    rng = rng_of("off-attn-bounded", T, bf16)
    rnd = R.bf16_round if bf16 else (lambda x: x)
    lay = Packed([T]) if T == MAX_T else Packed([BOUNDED_NEIGHBOURS[T][0], T, BOUNDED_NEIGHBOURS[T][1]])
    k = 0 if T == MAX_T else 1
    off = lay.offs[k]
    # one direction per head and term: content on the even dimensions, position on the odd ones; |g|^2 = S sqrt(128) makes a score coefficient x S
    S_CONTENT, S_POS, NOISE = 12.0, 3.0, 0.04
    even = (np.arange(DH) % 2 == 0).astype(np.float64)
    g = np.sqrt(S_CONTENT * np.sqrt(DH) / (DH / 2)) * rng.choice([-1.0, 1.0], (NH, DH)) * even
    g2 = np.sqrt(S_POS * np.sqrt(DH) / (DH / 2)) * rng.choice([-1.0, 1.0], (NH, DH)) * (1 - even)
    a, b = rng.choice([-1.0, 1.0], (T, NH)), rng.choice([-1.0, 1.0], (T, NH))
    c = 0.05 * rng.standard_normal((T, NH))
    for h in range(NH):                                                      # the salient keys of the head: distinct sizes in [0.5, 1], either sign
        sal = rng.choice(T, min(T, 8), replace=False)
        c[sal, h] = rng.uniform(0.5, 1.0, len(sal)) * rng.choice([-1.0, 1.0], len(sal))
    p = rng.uniform(-1.0, 1.0, (NREL, NH))
    q = a[:, :, None] * g[None] + b[:, :, None] * g2[None] + NOISE * rng.standard_normal((T, NH, DH))
    K = c[:, :, None] * g[None] + NOISE * rng.standard_normal((T, NH, DH))
    P = p[:, :, None] * g2[None] + NOISE * rng.standard_normal((NREL, NH, DH))
    bu = (0.25 * g + 0.1 * g2 / np.sqrt(S_POS) + NOISE * rng.standard_normal((NH, DH))).reshape(D).astype(np.float32)
    bv = (-0.25 * g2 - 0.1 * g / np.sqrt(S_CONTENT) + NOISE * rng.standard_normal((NH, DH))).reshape(D).astype(np.float32)
    qkv = (64.0 * rng.choice([-1.0, 1.0], (lay.M, QKV_LD))).astype(np.float32)          # the neighbours: loud
    qkv[off:off + T, :D] = rnd(q.reshape(T, D).astype(np.float32))
    qkv[off:off + T, D:2 * D] = rnd(K.reshape(T, D).astype(np.float32))
    qkv[off:off + T, 2 * D:] = rnd(rng.standard_normal((T, D)).astype(np.float32))
    pos = rnd(P.reshape(NREL, D).astype(np.float32))
    far = np.ones(NREL, bool)
    far[MAX_T - T:MAX_T - 1 + T] = False                                     # the rows of rel = T - 1 .. -(T - 1)
    pos[far] = 64.0 * rng.choice([-1.0, 1.0], (int(far.sum()), D))
    rho = 2.0 ** -9 if bf16 else 0.0
    rows, scale = bounded_rows(T), 1.0 / np.sqrt(float(DH))
    ref, wabsv, delta, peak = np.zeros((len(rows), D)), np.zeros((len(rows), D)), np.zeros((len(rows), NH)), []
    for h in range(NH):
        sl = slice(h * DH, (h + 1) * DH)
        qh, Kh, Vh = qkv[off:off + T, sl], qkv[off:off + T, D + h * DH:D + (h + 1) * DH], qkv[off:off + T, 2 * D + h * DH:2 * D + (h + 1) * DH]
        ctx, w, (qu, qv) = OR.attention(qh, Kh, Vh, pos[:, sl], bu[sl], bv[sl], rows)
        a1 = np.abs(qu) @ np.abs(Kh.astype(np.float64)).T
        a2 = OR.pos_scores(np.abs(qv), np.abs(pos[:, sl]), rows, T)
        delta[:, h] = (scale * (rho + 256 * U24) * (a1 + a2)).max(-1)
        ref[:, sl] = ctx
        wabsv[:, sl] = w @ np.abs(Vh.astype(np.float64))
        peak.append(w.max(-1))
    assert float(delta.max()) <= 0.05, delta.max()
    assert float(np.median(np.concatenate(peak))) >= 0.2, f"near-uniform weights hide index errors: median largest weight {np.median(np.concatenate(peak))}"
    return lay, k, qkv, pos, bu, bv, rows, ref, delta, wabsv


def attention_bound(ref, delta, wabsv, T, bf16, expf_rel):
    """(2 Delta_i + omega + expf_rel) sum_j w_j |V_jd| + o |ref|: omega = 2^-8 (weights rounded to bf16) or 2^-23 T, o = 2^-8 or 2^-23"""
    omega = 2.0 ** -8 if bf16 else 2.0 ** -23 * T
    o_rel = 2.0 ** -8 if bf16 else 2.0 ** -23
    return np.repeat(2 * delta + omega + expf_rel, DH, axis=1) * wabsv + o_rel * np.abs(ref)


SELECTOR_BATCHES = [(1, 15, 64, 2), (16, 129, 17), (63, 200, 65)]
BOUNDED_T = (1, 2, 15, 16, 17, 63, 64, 65, 129, 200)
SEEDS = (0, 1, 2)


def selector_runs(seeds=SEEDS):
    return [(run, s, None) for run in ("content", "position") for s in seeds] + [("content", 9, t) for t in CONTENT_TARGETS] + [("position", 9, t) for t in POSITION_TARGETS]


# ==== conv0 + ReLU + depthwise 3x3 =================================================================================================================
CONV0_N_MEL = (0, 1, 2, 3, 4, 5, 7, 8, 9, 33)
LOUD_MEL = 5
G10 = 10 * U24 / (1 - 10 * U24)


def sub_h2(n_mel):
    return 0 if n_mel <= 0 else OR.sub_len(OR.sub_len(n_mel))


class SubSetup:
    """[loud | n_0 | loud | n_1 | ... | loud]: mel packed back to back, output rows as the driver counts them but one row apart (that row stays the sentinel)"""

    def __init__(self, seed=0):
        rng = rng_of("off-conv0", seed)
        self.n_mel, self.tested = [], []
        for n in CONV0_N_MEL:
            self.n_mel += [LOUD_MEL, n]
            self.tested.append(len(self.n_mel) - 1)
        self.n_mel.append(LOUD_MEL)
        self.B = len(self.n_mel)
        self.mel_off = [int(x) for x in np.concatenate([[0], np.cumsum(self.n_mel)[:-1]])]
        self.h2 = [sub_h2(n) for n in self.n_mel]
        self.out_row = [int(x) + k for k, x in enumerate(np.concatenate([[0], np.cumsum(self.h2)[:-1]]))]
        self.out_rows = self.out_row[-1] + self.h2[-1] + 1
        self.max_h2 = max(self.h2)
        self.mel = (64.0 * rng.choice([-1.0, 1.0], (sum(self.n_mel), NMEL))).astype(np.float32)
        for k in self.tested:
            self.mel[self.mel_off[k]:self.mel_off[k] + self.n_mel[k]] = (2.0 * rng.standard_normal((self.n_mel[k], NMEL))).astype(np.float32)
        self.w0, self.b0 = (rng.standard_normal((SUBC, 3, 3)) / 3).astype(np.float32), (0.3 * rng.standard_normal(SUBC)).astype(np.float32)
        self.w2, self.b2 = (rng.standard_normal((SUBC, 3, 3)) / 3).astype(np.float32), (0.3 * rng.standard_normal(SUBC)).astype(np.float32)
        self.desc = np.array([(self.mel_off[k], self.n_mel[k], self.out_row[k], 0) for k in range(self.B)], np.int32)

    def wt(self, w):
        """[256][3][3] -> the engine's [9][256]"""
        return np.ascontiguousarray(w.reshape(SUBC, 9).T)

    def utterance(self, k):
        return self.mel[self.mel_off[k]:self.mel_off[k] + self.n_mel[k]]

    def reference(self, k):
        """-> (ref [H2][33][256], bound before the output's type)"""
        mel = self.utterance(k)
        ref, a0 = OR.conv_front(mel, self.w0, self.b0, self.w2, self.b2, parts=True)
        if len(ref) == 0:
            return ref, ref
        zero = np.zeros(SUBC)
        e0 = G10 * (OR.conv3x3_s2(np.abs(mel), np.abs(self.w0), zero, False) + np.abs(self.b0.astype(np.float64)))
        bound = OR.conv3x3_s2(e0, np.abs(self.w2), zero, True) + G10 * (OR.conv3x3_s2(a0, np.abs(self.w2), zero, True) + np.abs(self.b2.astype(np.float64)))
        return ref, bound


def conv_front_f32(mel, w0t, b0, w2t, b2):
    """k_sub_conv0_dw's documented contract in float32, operation for operation: conv0 sums its nine taps from 0 in (kh, kw) order with a separate multiply
    and add, a tap in the padding adding w x 0; + bias, ReLU; the depthwise conv sums its taps inside conv0's image in (kh2, kw2) order from 0; + bias"""
    n_mel = len(mel)
    H1 = OR.sub_len(n_mel)
    H2 = OR.sub_len(H1)
    mp = np.zeros((max(4 * H2 + 8, n_mel + 6), 4 * 33 + 12), np.float32)                     # mel row ih at mp[ih + 6], column iw at mp[:, iw + 6]
    mp[6:6 + n_mel, 6:6 + NMEL] = mel
    t2, f2 = np.arange(H2)[:, None, None], np.arange(33)[None, :, None]
    acc2 = np.zeros((H2, 33, SUBC), np.float32)
    for kh2 in range(3):
        for kw2 in range(3):
            t, f = 2 * t2 + kh2 - 2, 2 * f2 + kw2 - 2
            inside = (t >= 0) & (t < H1) & (f >= 0) & (f < 65)
            acc = np.zeros((H2, 33, SUBC), np.float32)
            for kh in range(3):
                for kw in range(3):
                    x = mp[4 * t2 + 2 * kh2 + kh, 4 * f2 + 2 * kw2 + kw]     # [H2][33][1]
                    acc = acc + w0t[kh * 3 + kw][None, None, :] * x
            a0 = np.maximum(acc + b0[None, None, :], np.float32(0))
            acc2 = np.where(inside, acc2 + w2t[kh2 * 3 + kw2][None, None, :] * a0, acc2)
    return acc2 + b2[None, None, :]
