"""Operands, expectations and bound terms of tests/test_gpu_spk_kernels.py, numpy only (checked without a GPU by tests/test_spk_kernel_ref.py).

Two modes per kernel.
  exact    small integers: every f32 sum is an integer below 2^24 in any order and with or without fma contraction, every bf16 output an integer below 256.
           SE gates are exactly 0 or 1 (z = +40: exp(-40) < 2^-25 under any expf; z = -100: exp(100) overflows to inf); SG_ASP logits are one winner per
           (segment, channel) more than 104 above every other valid frame (exp(-104) < 2^-150 rounds to 0), with higher logits planted on a frame >= L.
           The expectation is the float32 expression in the kernel's documented order.
  bounded  random operands rounded to the operand type, every element against the float64 reference (tests/spk_ref.py).  Terms, u = 2^-24, gam(n) = n u / (1 - n u):
           f32 accumulation of n products: gam(n) sum |a| |w|; a bf16 store: 2^-8 (|ref| + e) on top of the propagated e; sigmoid / expf / tanhf: the device
           libm constants of profiles/decode_kernels.md (4 x the measured maxima); sqrtf and f32 division are IEEE operations in this build (no fast-math
           flag in csrc/Makefile): u each, taken 4 x like the measured ones.
A launch of k_spk_gemm / k_spk_tile sees segments 1 .. S of buffers that hold S + 2: segment 0 and S + 1 are loud (|x| = 64, lens 160 and 1, gates open)
but finite, since ReLU swallows the NaN of the sentinel.  For the same reason stale rows >= L (Y of SG_RES and of k_spk_tile, the f32 kernels' inputs) are loud,
finite and positive on rows L, L + 2, .. and the sentinel on rows L + 1, L + 3, .. (stale())."""
from __future__ import annotations

import zlib

import numpy as np

from tests import spk_ref as R
from tests.spk_ref import BF16_REL, NMEL, T, TVALID, U24

SENT = 0xFFC5
SENT_F32 = np.array([SENT, SENT], np.uint16).view(np.float32)[0]
SG_DW, SG_Y, SG_RES, SG_ASP = range(4)
ST_DW, ST_STATS = 0, 1
MODE_NAMES = {SG_DW: "SG_DW", SG_Y: "SG_Y", SG_RES: "SG_RES", SG_ASP: "SG_ASP"}
LENS_SET = (1, 2, 9, 10, 11, 19, 20, 21, 39, 40, 41, 79, 80, 81, 149, 150)

SIGM_REL, TANHF_REL, EXPF = 4 * 1.52e-7, 4 * 1.32e-7, 4 * 7.96e-8          # profiles/decode_kernels.md: sigm on [-30, 30], tanhf on [-12, 12], expf on [-80, 0]
SQRT_REL = DIV_REL = 4 * U24


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def gam(n):
    return n * U24 / (1.0 - n * U24)


def lens_for(i, S):
    """lens of launch i: segments 1 .. S from LENS_SET, the loud neighbours 160 and 1"""
    mid = [LENS_SET[(5 * i + 7 * s + 3) % 16] for s in range(S)]
    return np.array([160] + mid + [1], np.int32)


def loud(rng, shape):
    return (64.0 * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def mask_rows(x, lens, fill):
    """rows >= L of x [S][160][..] replaced by `fill`"""
    return np.where(R.mask(lens), x, fill).astype(x.dtype)


def stale(x, lens, value=64.0):
    """rows >= L as a launch may find them: row L, L + 2, .. loud, finite and positive (ReLU swallows a NaN, so a mask that is off by one frame or missing would
    not show on the sentinel), rows L + 1, L + 3, .. the sentinel.  The kernels read them and must mask them."""
    x = np.asarray(x, np.float32)
    t = np.arange(T)[None, :, None] - np.asarray(lens)[:, None, None]
    return np.where(t < 0, x, np.where(t % 2 == 0, np.float32(value), SENT_F32)).astype(np.float32)


# ---- k_spk_gemm ---------------------------------------------------------------------------------------------------------------------------------
# (K, N, S, lda, dw_k of SG_DW, dw_k of SG_RES, lda_out): grids S N / 128 = 1, 3, 8, 9, 10, 3, 8, 10, 3, 16; K / 32 = 1 .. 5 take LOOP 0, 8, 16, 32 LOOP 1
GEMM_SHAPES = [(32, 128, 1, 32, 3, 0, 128), (64, 128, 3, 64, 7, 7, 128), (96, 256, 4, 96, 11, 11, 256), (128, 384, 3, 160, 15, 15, 384), (160, 256, 5, 160, 3, 0, 256),
               (256, 128, 3, 256, 7, 7, 128), (256, 256, 4, 256, 11, 11, 320), (512, 256, 5, 512, 15, 15, 256), (1024, 384, 1, 1024, 3, 0, 384),
               (1024, 1024, 2, 1024, 7, 7, 1024)]
FORCED_LOOP0 = [6, 8]          # shapes run once more in a child process with NASR_SPK_LOOP=0: K = 256 and K = 1024


def gemm_kernel(mode, K, forced0=False):
    return f"k_spk_gemm<{MODE_NAMES[mode]},{0 if forced0 or (K // 32) % 8 else 1}>"


def sparse_taps(rng, k, C):
    """taps [k][C] in {-1, 0, 1} with three nonzero per channel (all of them at k = 3), every tap index nonzero in some channel"""
    w = np.zeros((k, C), np.float32)
    for c in range(C):
        idx = [(c + j * (k // 3 + 1)) % k for j in range(3)] if k > 3 else [0, 1, 2]
        w[idx, c] = rng.choice([-1.0, 1.0], size=3)
    return w


def dwabs(x, w, lens):
    return R.depthwise(np.abs(x), np.abs(w), lens)


def dw_store(v, ev, w, lens):
    """(ref, bound) of the depthwise conv of v (error ev, both already masked) stored as bf16"""
    ref = R.depthwise(v, w, lens)
    e = dwabs(ev, w, lens) + gam(w.shape[0] + 1) * dwabs(v, w, lens)
    return ref, e + BF16_REL * (np.abs(ref) + e)


def stats_bound(o, eo, lens):
    """(mean, std, e_mean, e_std) of the masked statistics of o [S][160][C] computed in f32 from values with error eo"""
    m = R.mask(lens)
    L = np.asarray(lens, np.float64)[:, None]
    mean, std = R.stats(o, lens)
    e_mean = np.where(m, eo, 0.0).sum(1) / L + gam(T + 2) * np.where(m, np.abs(o), 0.0).sum(1) / L
    d = np.where(m, np.abs(o - mean[:, None, :]), 0.0)
    ed = np.where(m, eo + e_mean[:, None, :] + 2 * U24 * d, 0.0)
    var = (d ** 2).sum(1) / L
    e_var = (2 * d * ed + ed ** 2).sum(1) / L + gam(T + 6) * var
    hi, lo = np.sqrt(np.clip(var + e_var, 1e-10, 1e30)), np.sqrt(np.clip(var - e_var, 1e-10, 1e30))
    return mean, std, e_mean, (hi - lo) + SQRT_REL * hi + 1e-10 ** 0.5 * 2 * U24          # the last term: 1e-10f is not 1e-10


def asp_bound(x, wgt, mu, var, sc, bi, el):
    """bound of the pool [S][2 C] of attentive statistics computed in f32 from logits with error el [S][C] (x exact, frames >= L zero with weight 0).
    First order in the weights' relative error, with the second-order term of e_mu kept: a logit error moves exp(l_t - max) by expm1(2 el) relatively."""
    C = x.shape[2]
    d = np.expm1(2 * el) + EXPF + 2 * U24                   # relative error of one exp(l_t - max)
    rel_w = 2 * d + gam(T + 2) + DIV_REL                    # ... of one normalised weight
    wx = (wgt * np.abs(x)).sum(1)
    e_mu = (rel_w + gam(T + 2)) * wx + 2 * U24 * np.abs(mu)
    dx = np.abs(x - mu[:, None, :])
    e_var = (rel_w + gam(T + 4) + DIV_REL) * var + 2 * (wgt * dx).sum(1) * e_mu + e_mu ** 2
    hi, lo = np.sqrt(np.maximum(var + e_var, 1e-10)), np.sqrt(np.maximum(var - e_var, 1e-10))
    e_sig = (hi - lo) + SQRT_REL * hi + 1e-5 * 2 * U24      # the last term: 1e-10f is not 1e-10
    sig = np.sqrt(np.maximum(var, 1e-10))
    return np.concatenate([e_mu * np.abs(sc[:C]) + 2 * U24 * (np.abs(mu * sc[:C]) + np.abs(bi[:C])),
                           e_sig * np.abs(sc[C:]) + 2 * U24 * (np.abs(sig * sc[C:]) + np.abs(bi[C:]))], 1)


def gemm_case(i, mode, kind):
    """operands of launch (shape i, mode, kind) over S + 2 segments and what the launched segments 1 .. S must hold afterwards.
    returns dict: ins (name -> array), dims, exp (name -> (expected f32 / bf16 values over the launched segments, bound or None for ==))"""
    K, N, S, lda, k_dw, k_res, lda_out = GEMM_SHAPES[i]
    rng = rng_of("gemm", i, mode, kind)
    St, KT = S + 2, K // 32
    lens = lens_for(i, S)
    ll = lens[1:-1]
    exact = kind == "exact"
    dw_k = k_dw if mode == SG_DW else k_res if mode == SG_RES else 0
    # A [St][160][lda]: columns K .. lda - 1 are loud and never read
    A = loud(rng, (St, T, lda))
    W = np.zeros((N, K), np.float32)
    win = asp_facts = None
    if exact and mode == SG_Y:
        A[1:-1, :, :K] = rng.integers(-3, 4, (S, T, K))
        W[:] = rng.integers(-2, 3, (N, K))
        bias = rng.integers(-4, 5, N).astype(np.float32)
    elif exact:
        A[1:-1, :, :K] = rng.integers(-2, 3, (S, T, K)) if mode != SG_ASP else rng.integers(-1, 2, (S, T, K))
        n = np.arange(N)
        for c in range(KT):          # one nonzero weight per output channel and 32-deep chunk, at a position of its own
            W[n, c * 32 + (n * 7 + c * 13 + n // 16) % 32] = rng.choice([-1.0, 1.0], size=N)
        bias = rng.integers(-2, 3, N).astype(np.float32)
        if mode == SG_ASP:           # the winner frame of each segment: 128 across chunk 0 against weight +2; a louder row on frame L, which is masked
            W[n, (n * 7 + n // 16) % 32] = 2.0
            win = np.array([int(rng.integers(0, L)) for L in ll])
            for s, L in enumerate(ll):
                A[1 + s, win[s], :32] = 128.0
                if L < T:
                    A[1 + s, L, :32] = 192.0
    else:
        A[1:-1, :, :K] = R.bf16_round(rng.standard_normal((S, T, K)))
        W[:] = R.bf16_round(rng.standard_normal((N, K)) / np.sqrt(K))
        bias = (0.5 * rng.standard_normal(N)).astype(np.float32)
    ins = {"A": R.bf16_bits(A).reshape(St * T, lda), "W": W, "bias": bias, "lens": lens}
    a, exp = A[1:-1, :, :K], {}
    acc = R.pointwise(a, W, bias, ll, masked=False)                 # float64, exact in exact mode
    ey = np.zeros_like(acc) if exact else gam(K + 2) * R.pointwise_abs(a, W, bias)
    m = R.mask(ll)
    if dw_k:
        taps = sparse_taps(rng, dw_k, N) if exact else (0.5 * rng.standard_normal((dw_k, N))).astype(np.float32)
        ins["dw_w"] = taps
    if mode == SG_DW:
        v, ev = np.where(m, np.maximum(acc, 0.0), 0.0), np.where(m, ey, 0.0)
        ref, b = dw_store(v, ev, taps, ll)
        exp["a_out"] = (ref, None if exact else b)
    elif mode == SG_Y:
        y = np.where(m, acc, 0.0)
        L = ll.astype(np.float64)[:, None]
        if exact:
            cm = y.sum(1).astype(np.float32) * (np.float32(1.0) / ll.astype(np.float32))[:, None]      # f32(sum) * f32(1 / L), the kernel's expression
            exp["y_out"], exp["colmean"] = (y, None), (cm, None)
        else:
            exp["y_out"] = (y, np.where(m, ey, 0.0))
            exp["colmean"] = (R.colmean(y, ll), np.where(m, ey, 0.0).sum(1) / L + (gam(T + 2) + DIV_REL) * np.abs(y).sum(1) / L)
    elif mode == SG_RES:
        y_in = np.zeros((St, T, N), np.float32) + 64.0
        z = np.full((St, N), 40.0, np.float32)
        if exact:
            y_in[1:-1] = rng.integers(-8, 9, (S, T, N))
            z[1:-1] = rng.choice([40.0, -100.0], size=(S, N))
        else:
            y_in[1:-1] = rng.standard_normal((S, T, N))
            z[1:-1] = 2.0 * rng.standard_normal((S, N))
        yv = y_in[1:-1].astype(np.float64)
        y_in[1:-1] = stale(y_in[1:-1], ll, 256.0)                   # stale rows >= L, 256 where loud: positive after any gate and any acc + bias of these cases
        ins["y_in"], ins["z"] = y_in.reshape(St * T, N), z
        g = np.where(z[1:-1] > 0, 1.0, 0.0)[:, None, :] if exact else R.sigmoid(z[1:-1])[:, None, :]
        o = np.where(m, np.maximum(yv * g + acc, 0.0), 0.0)
        eo = np.where(m, np.abs(yv) * g * SIGM_REL + ey + 3 * U24 * (np.abs(yv * g) + np.abs(acc)), 0.0) * (0.0 if exact else 1.0)
        exp["x_out"] = (o, None if exact else eo + BF16_REL * (o + eo))
        if dw_k:
            ref, b = dw_store(o, eo, taps, ll)
            exp["a_out"] = (ref, None if exact else b)
    else:
        x_in = np.full((St, T, N), 64.0, np.float32)
        x_in[1:-1] = rng.integers(-8, 9, (S, T, N)) if exact else R.bf16_round(rng.standard_normal((S, T, N)))
        x_in[1:-1] = mask_rows(x_in[1:-1], ll, 0.0)                 # rows >= L are zero, as the producer writes them
        ins["x_in"] = R.bf16_bits(x_in).reshape(St * T, N)
        if exact:
            bn_s = np.concatenate([rng.choice([-2.0, -1.0, 1.0, 2.0], size=N), rng.choice([0.5, 1.0, 2.0, -1.0], size=N)]).astype(np.float32)
            bn_b = np.concatenate([rng.integers(-4, 5, N), np.zeros(N)]).astype(np.float32)
        else:
            bn_s = (1.0 + 0.2 * rng.standard_normal(2 * N)).astype(np.float32)
            bn_b = (0.5 * rng.standard_normal(2 * N)).astype(np.float32)
        ins["bn_s"], ins["bn_b"] = bn_s, bn_b
        x = x_in[1:-1].astype(np.float64)
        pool, (wgt, mu, var) = R.asp(x, acc, ll, bn_s, bn_b)
        if exact:
            lg = np.where(m, acc, -np.inf)
            top = lg.max(1)
            second = np.where(np.arange(T)[None, :, None] == win[:, None, None], -np.inf, lg).max(1)
            margin = float((top - second).min())
            planted = all(L == T or np.all(acc[s, L] > top[s]) for s, L in enumerate(ll))
            mu_x = x[np.arange(S), win]                             # [S][N]
            sig = np.sqrt(np.float32(1e-10))                        # sqrtf(fmaxf(0 / 1, 1e-10f)), correctly rounded
            pool = np.concatenate([mu_x * bn_s[:N] + bn_b[:N], np.broadcast_to((sig * bn_s[N:]).astype(np.float64), (S, N))], 1)
            exp["pool"] = (pool, None)
            asp_facts = (margin, planted, np.array_equal(lg.argmax(1), np.broadcast_to(win[:, None], (S, N))))
        else:
            exp["pool"] = (pool, asp_bound(x, wgt, mu, var, bn_s, bn_b, np.where(m, ey, 0.0).max(1)))
    return {"ins": ins, "exp": exp, "dims": dict(K=K, N=N, S=S, lda=lda, dw_k=dw_k, lda_out=lda_out, mode=mode, St=St), "lens": ll, "asp": asp_facts}


# ---- k_spk_tile ---------------------------------------------------------------------------------------------------------------------------------
# (C, S, mode, dw_k or stat_ld / C)
TILE_CASES = [(64, 1, ST_DW, 3), (128, 3, ST_DW, 7), (192, 1, ST_DW, 11), (64, 3, ST_DW, 15), (192, 3, ST_DW, 3), (128, 1, ST_DW, 15),
              (64, 1, ST_STATS, 1), (128, 3, ST_STATS, 2), (192, 3, ST_STATS, 1), (192, 1, ST_STATS, 2), (64, 3, ST_STATS, 2)]


def tile_case(i, kind):
    C, S, mode, arg = TILE_CASES[i]
    rng = rng_of("tile", i, kind)
    St = S + 2
    lens = lens_for(2 * i + 1, S)
    ll = lens[1:-1]
    exact = kind == "exact"
    y = np.full((St, T, C), 64.0, np.float32)
    z = np.full((St, C), 40.0, np.float32)
    if exact:
        y[1:-1] = rng.integers(-8, 9, (S, T, C))
        z[1:-1] = rng.choice([40.0, -100.0], size=(S, C))
    else:
        y[1:-1] = rng.standard_normal((S, T, C))
        z[1:-1] = 2.0 * rng.standard_normal((S, C))
    yv = y[1:-1].astype(np.float64)
    y[1:-1] = stale(y[1:-1], ll)
    m = R.mask(ll)
    g = np.where(z[1:-1] > 0, 1.0, 0.0)[:, None, :] if exact else R.sigmoid(z[1:-1])[:, None, :]
    o = np.where(m, np.maximum(yv * g, 0.0), 0.0)
    eo = np.zeros_like(o) if exact else np.where(m, np.abs(yv) * g * (SIGM_REL + 2 * U24), 0.0)
    ins = {"y_in": y.reshape(St * T, C), "z": z, "lens": lens}
    exp = {"x_out": (o, None if exact else eo + BF16_REL * (o + eo))}
    dims = dict(C=C, S=S, St=St, mode=mode, dw_k=0, lda_out=0, stat_ld=0)
    if mode == ST_DW:
        taps = sparse_taps(rng, arg, C) if exact else (0.5 * rng.standard_normal((arg, C))).astype(np.float32)
        ins["dw_w"] = taps
        ref, b = dw_store(o, eo, taps, ll)
        exp["a_out"] = (ref, None if exact else b)
        dims.update(dw_k=arg, lda_out=C + (64 if i % 2 else 0))
    else:
        mean, std, e_mean, e_std = stats_bound(o, eo, ll)
        exp["mean"], exp["stdv"] = (mean, e_mean + DIV_REL * np.abs(mean)), (std, e_std)
        if exact:                                                    # f32(sum) * f32(1 / L), the kernel's expression; the std is no integer expression and stays bounded
            exp["mean"] = (o.sum(1).astype(np.float32) * (np.float32(1.0) / ll.astype(np.float32))[:, None], None)
        dims.update(stat_ld=arg * C)
    return {"ins": ins, "exp": exp, "dims": dims, "lens": ll}


# ---- k_spk_front --------------------------------------------------------------------------------------------------------------------------------
FRONT_CASES = [(1, 80, 128, (1,)), (3, 96, 192, (2, 149, 150)), (3, 80, 192, (150, 1, 149)), (1, 96, 128, (2,))]


def front_case(i):
    """log-mel on the grid 2^-10 (every double sum of them is exact), taps multiples of 1/8: the float32 restatement of the kernel's documented order is ==."""
    S, cpitch, lda_out, lens = FRONT_CASES[i]
    rng = rng_of("front", i)
    mel = loud(rng, (S, T, cpitch))
    mel[:, :, :NMEL] = np.round(rng.uniform(-12.0, 2.0, (S, T, NMEL)) * 1024) / 1024
    mel[:, TVALID:, :NMEL] = 0.0                                     # as k_diar_logmel leaves them
    taps = (rng.integers(-16, 17, (3, NMEL)) / 8.0).astype(np.float32)
    x = mel[:, :TVALID, :NMEL]
    mean = (x.astype(np.float64).sum(1) / TVALID).astype(np.float32)               # (float)(sum / 150), the sum exact
    d = (x - mean[:, None, :]).astype(np.float32).astype(np.float64)               # __fsub_rn
    part = np.zeros((S, 6, NMEL))
    for u in range(25):                                                            # six groups of 25 frames, each summed in frame order, then the six in order
        part += d.reshape(S, 6, 25, NMEL)[:, :, u] ** 2
    var = np.zeros((S, NMEL))
    for k in range(6):
        var += part[:, k]
    sd = np.sqrt((var / (TVALID - 1)).astype(np.float32))                          # sqrtf, correctly rounded
    inv = np.float32(1.0) / (sd + np.float32(1e-5))                                # __fadd_rn, IEEE division
    xn = ((x - mean[:, None, :]).astype(np.float32) * inv[:, None, :]).astype(np.float32)
    ll = np.array(lens, np.int32)
    full = np.zeros((S, T, NMEL), np.float32)
    full[:, :TVALID] = xn
    m = R.mask(ll)
    xm = np.pad(np.where(m, full, 0.0).astype(np.float64), ((0, 0), (1, 1), (0, 0)))
    acc = (xm[:, 0:T] * taps[0]).astype(np.float32).astype(np.float64)             # x0 * w0, then two fma: the double sum of a 24-bit and a 30-bit term is exact
    acc = (xm[:, 1:T + 1] * taps[1] + acc).astype(np.float32).astype(np.float64)
    acc = (xm[:, 2:T + 2] * taps[2] + acc).astype(np.float32)
    out = np.zeros((S, T, 128), np.float32)
    out[:, :, :NMEL] = np.where(m, acc, 0.0)
    ref = np.zeros((S, T, 128))
    ref64 = np.zeros((S, T, NMEL))
    ref64[:, :TVALID] = R.featnorm(mel[:, :, :NMEL])
    ref[:, :, :NMEL] = R.depthwise(ref64, taps, ll)
    return {"mel": mel.reshape(S * T, cpitch), "taps": taps, "lens": ll, "bits": R.bf16_bits(out), "ref": ref, "dims": dict(S=S, cpitch=cpitch, lda_out=lda_out)}


# ---- k_spk_fc / k_spk_fc_reduce -------------------------------------------------------------------------------------------------------------------
FC_SITES = [(1024, 128), (128, 1024), (3072, 384), (384, 3072), (6144, 128), (6144, 192)]
FC_M = (1, 5, 63, 64, 65, 96)


def fc_slices(M, K, N):
    """spk_fc_slices (kernels_spk.hip) restated"""
    KG, wgs, Z = K // 16, (N // 16) * ((M + 63) // 64), 1
    if K < 1024:
        return 1
    while Z < 16 and wgs * Z < 256 and KG % (8 * Z) == 0:
        Z *= 2
    return Z


def fc_weights(K, N, kind):
    rng = rng_of("fcw", K, N, kind)
    if kind == "exact":
        return rng.integers(-2, 3, (N, K)).astype(np.float32), rng.integers(-8, 9, N).astype(np.float32)
    return (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), (0.5 * rng.standard_normal(N)).astype(np.float32)


def fc_case(K, N, M, relu, ldx, kind):
    rng = rng_of("fc", K, N, M, relu, ldx, kind)
    W, b = fc_weights(K, N, kind)
    x = loud(rng, (M, ldx))
    x[:, :K] = rng.integers(-2, 3, (M, K)) if kind == "exact" else rng.standard_normal((M, K))
    ref = R.linear(x[:, :K], W, b, relu)
    bound = None if kind == "exact" else gam(K + 4) * (np.abs(x[:, :K].astype(np.float64)) @ np.abs(W.astype(np.float64)).T + np.abs(b))
    return {"x": x, "W": W, "b": b, "ref": ref, "bound": bound}


# ---- k_gather_audio -----------------------------------------------------------------------------------------------------------------------------
GATHER_BYTES = (2, 14, 16, 18, 4096 + 6, 48000)
# (name, [(src offset, dst offset, bytes)], max_bytes): offsets chosen so that src and dst are 16-byte aligned or not, each alone and both
GATHER_CASES = [("aligned", [(0, 0, n) for n in GATHER_BYTES[:1]], 2)] + \
    [(f"aligned_{n}", [(0, 0, n)], n) for n in GATHER_BYTES[1:]] + \
    [(f"src_off_{n}", [(6, 0, n)], n) for n in GATHER_BYTES] + \
    [(f"dst_off_{n}", [(0, 10, n)], n) for n in GATHER_BYTES] + \
    [(f"both_off_{n}", [(2, 18, n)], n) for n in GATHER_BYTES] + \
    [("three_mixed", [(0, 0, 4102), (4128 + 6, 4112, 48000), (53000, 52400 + 16, 18)], 48000),
     ("three_small_max", [(16, 32, 14), (64, 64 + 2, 16), (128 + 8, 256, 4102)], 18),
     ("three_aligned", [(0, 0, 48000), (48000, 48016, 16), (48016, 48048, 2)], 48000)]


def gather_case(i):
    name, desc, max_bytes = GATHER_CASES[i]
    rng = rng_of("gather", i)
    size = max(max(so + n for so, _, n in desc), max(do + n for _, do, n in desc)) + 64
    src = rng.integers(0, 65536, size // 2 + 1, dtype=np.uint16)
    src[src == SENT] = 0
    want = np.full(size // 2 + 1, SENT, np.uint16)
    for so, do, n in desc:
        want[do // 2:(do + n) // 2] = src[so // 2:(so + n) // 2]
    return {"src": src, "desc": np.array(desc, np.int64), "max_bytes": max_bytes, "want": want}


# ---- the f32 engine's layer-by-layer kernels (kernels_diar.hip) ------------------------------------------------------------------------------------
def f32_lens(i, S):
    return np.array([LENS_SET[(3 * i + 5 * s) % 16] for s in range(S)], np.int32)


DEPTHWISE_CASES = [(k, C, Cpad, S) for k, (C, Cpad, S) in zip((1, 3, 7, 11, 15, 1, 3, 7, 11, 15, 15, 3),
                                                              [(80, 128, 1), (64, 64, 3), (320, 320, 1), (80, 128, 3), (64, 64, 1), (320, 320, 3), (80, 128, 3), (64, 64, 1),
                                                               (320, 320, 3), (80, 128, 1), (320, 320, 1), (320, 320, 3)])]


def dw_chain_f32(xv, w, lens):
    """k_spk_depthwise's pinned order in float32: tap 0's product rounded, then one fma per tap, i ascending.  With x of 16 and taps of <= 6 significant bits a
    product has <= 22 bits, so product + acc is exact in float64 and the one rounding to f32 is the fma's."""
    k = w.shape[0]
    pad = (k - 1) // 2
    m = R.mask(lens)
    xp = np.pad(np.where(m, xv, 0.0).astype(np.float64), ((0, 0), (pad, pad), (0, 0)))
    acc = (xp[:, 0:T] * w[0].astype(np.float64)).astype(np.float32)
    for i in range(1, k):
        acc = (xp[:, i:i + T] * w[i].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return np.where(m, acc, np.float32(0.0)).astype(np.float32)


def depthwise_case(i, kind):
    """chain: x of 16 significant bits, taps multiples of 1/8: the chain rounds at every step, and dw_chain_f32 restates it bit for bit (`f32`);
    exact: x on the grid 2^-10, taps multiples of 1/8: every product and every partial sum of the fma chain is a multiple of 2^-13 below 2^11, so the chain
    is exact and equals the float64 reference whatever the order; bounded: random f32 taps"""
    k, C, Cpad, S = DEPTHWISE_CASES[i]
    rng = rng_of("dw", i, kind)
    ll = f32_lens(i, S)
    pitch = C + (16 if i % 3 == 0 else 0)
    x = loud(rng, (S, T, pitch))
    x[:, :, :C] = np.round(rng.standard_normal((S, T, C)) * 1024) / 1024 if kind == "exact" else rng.standard_normal((S, T, C))
    if kind == "chain":
        x[:, :, :C] = (x[:, :, :C].view(np.uint32) & np.uint32(0xFFFFFF00)).view(np.float32)
    w = (rng.integers(-16, 17, (k, C)) / 8.0).astype(np.float32) if kind != "bounded" else (0.5 * rng.standard_normal((k, C))).astype(np.float32)
    xv = x[:, :, :C].astype(np.float64)
    x[:, :, :C] = stale(x[:, :, :C], ll)
    ref = np.zeros((S, T, Cpad))
    ref[:, :, :C] = R.depthwise(xv, w, ll)
    bound = np.zeros_like(ref)
    if kind != "exact":
        bound[:, :, :C] = gam(k + 1) * dwabs(xv, w, ll)
    f32 = None
    if kind == "chain":
        f32 = np.zeros((S, T, Cpad), np.float32)
        f32[:, :, :C] = dw_chain_f32(xv, w, ll)
    return {"x": x.reshape(S * T, pitch), "w": w, "lens": ll, "ref": ref, "bound": None if kind == "exact" else bound, "f32": f32, "dims": dict(k=k, C=C, Cpad=Cpad, S=S, pitch=pitch)}


def colmean_f32(y, lens):
    """k_spk_colmean's order in float32: four partial sums over t = 0, 4, 8 .., the remainder into the first, ((s0 + s1) + (s2 + s3)) * (1 / L)"""
    y = np.asarray(y, np.float32)
    out = np.zeros((y.shape[0], y.shape[2]), np.float32)
    for s, L in enumerate(lens):
        p = np.zeros((4, y.shape[2]), np.float32)
        t = 0
        while t + 4 <= L:
            for j in range(4):
                p[j] += y[s, t + j]
            t += 4
        while t < L:
            p[0] += y[s, t]
            t += 1
        out[s] = ((p[0] + p[1]) + (p[2] + p[3])) * (np.float32(1.0) / np.float32(L))
    return out


def colmean_case(i):
    C, S = [(64, 1), (300, 3), (64, 3), (300, 1), (64, 3), (300, 3)][i]
    rng = rng_of("colmean", i)
    ll = f32_lens(i + (0 if i < 4 else 7), S)
    yv = rng.standard_normal((S, T, C)).astype(np.float32)
    L = ll.astype(np.float64)[:, None]
    return {"y": stale(yv, ll).reshape(S * T, C), "lens": ll, "f32": colmean_f32(yv, ll), "ref": R.colmean(yv, ll),
            "bound": (gam(T + 2) + DIV_REL) * np.where(R.mask(ll), np.abs(yv.astype(np.float64)), 0.0).sum(1) / L, "dims": dict(C=C, S=S)}


def combine_case(i):
    C, S, res = [(96, 3, True), (96, 3, False), (320, 1, True), (64, 1, False)][i]
    rng = rng_of("combine", i)
    ll = f32_lens(i + 2, S)
    yv = rng.standard_normal((S, T, C)).astype(np.float32)
    z = (2.0 * rng.standard_normal((S, C))).astype(np.float32)
    r = rng.standard_normal((S, T, C)).astype(np.float32) if res else None
    ref = R.combine(yv, z, r, ll)
    g = R.sigmoid(z)[:, None, :]
    ym = np.where(R.mask(ll), np.abs(yv.astype(np.float64)), 0.0)
    bound = ym * g * (SIGM_REL + 2 * U24) + 2 * U24 * np.abs(ref)
    return {"y": stale(yv, ll).reshape(S * T, C), "z": z, "r": None if r is None else r.reshape(S * T, C), "lens": ll, "ref": ref, "bound": bound, "dims": dict(C=C, S=S)}


def stats_case(i):
    C, S = [(64, 1), (300, 3), (64, 3)][i]
    rng = rng_of("stats", i)
    ll = f32_lens(2 * i + 1, S)
    xv = (rng.standard_normal((S, T, C)) * (1.0 + np.arange(C) % 3)).astype(np.float32)
    if i == 2:
        xv[:, :, :8] = 0.25                                          # constant channels: the 1e-10 clamp decides
    mean, std, e_mean, e_std = stats_bound(xv.astype(np.float64), np.zeros((S, T, C)), ll)
    return {"x": stale(xv, ll).reshape(S * T, C), "lens": ll, "mean": (mean, e_mean + DIV_REL * np.abs(mean)), "stdv": (std, e_std), "dims": dict(C=C, S=S)}


def att_const_case(i):
    C, A, S = [(64, 128, 1), (320, 128, 3), (64, 6, 3), (320, 6, 1)][i]
    rng = rng_of("att_const", i)
    mean, stdv = rng.standard_normal((S, C)).astype(np.float32), np.abs(rng.standard_normal((S, C))).astype(np.float32)
    w1 = (rng.standard_normal((A, 3 * C)) / np.sqrt(C)).astype(np.float32)
    w1[:, :C] = 64.0                                                 # the x third of the conv is not this kernel's: never read
    b1 = rng.standard_normal(A).astype(np.float32)
    ab = np.abs(mean.astype(np.float64)) @ np.abs(w1[:, C:2 * C].astype(np.float64)).T + np.abs(stdv.astype(np.float64)) @ np.abs(w1[:, 2 * C:].astype(np.float64)).T + np.abs(b1)
    return {"mean": mean, "stdv": stdv, "w1": w1, "b1": b1, "ref": R.att_const(mean, stdv, w1, b1), "bound": gam(2 * C + 8) * ab, "dims": dict(C=C, A=A, S=S)}


def att_post_case(i):
    A, S, bf16 = [(128, 1, 0), (128, 3, 1), (6, 3, 0), (6, 1, 1)][i]
    rng = rng_of("att_post", i)
    g = rng.standard_normal((S, T, A)).astype(np.float32)
    c = rng.standard_normal((S, A)).astype(np.float32)
    sc, bi = (1.0 + 0.3 * rng.standard_normal(A)).astype(np.float32), (0.5 * rng.standard_normal(A)).astype(np.float32)
    ref = R.att_post(g, c, sc, bi)
    pre = np.maximum(g.astype(np.float64) + c[:, None, :], 0.0)
    e = 3 * U24 * (np.abs(pre * sc) + np.abs(bi)) + TANHF_REL * np.abs(ref)          # |tanh'| <= 1
    return {"g": g.reshape(S * T, A), "c": c, "sc": sc, "bi": bi, "ref": ref, "bound": e + (BF16_REL * (np.abs(ref) + e) if bf16 else 0.0), "dims": dict(A=A, S=S, bf16=bf16),
            "pre_max": float(np.abs(pre * sc + bi).max())}


def asp_case(i):
    C, S = [(64, 1), (300, 3), (64, 3)][i]
    rng = rng_of("asp", i)
    ll = f32_lens(3 * i + 2, S)
    xv = rng.standard_normal((S, T, C)).astype(np.float32)
    lg = (2.0 * rng.standard_normal((S, T, C))).astype(np.float32)
    sc, bi = (1.0 + 0.2 * rng.standard_normal(2 * C)).astype(np.float32), (0.5 * rng.standard_normal(2 * C)).astype(np.float32)
    xm = np.where(R.mask(ll), xv.astype(np.float64), 0.0)
    pool, (wgt, mu, var) = R.asp(xm, lg, ll, sc, bi)
    return {"x": stale(xv, ll).reshape(S * T, C), "logits": stale(lg, ll).reshape(S * T, C), "lens": ll, "sc": sc, "bi": bi, "ref": pool,
            "bound": asp_bound(xm, wgt, mu, var, sc, bi, np.zeros((S, C))), "dims": dict(C=C, S=S)}


def mask_cvt_case(i):
    C, S = [(64, 1), (300, 3)][i]
    rng = rng_of("mask_cvt", i)
    ll = f32_lens(i + 5, S)
    xv = rng.standard_normal((S, T, C)).astype(np.float32)
    return {"x": stale(xv, ll).reshape(S * T, C), "lens": ll, "want": mask_rows(xv, ll, 0.0), "dims": dict(C=C, S=S)}
