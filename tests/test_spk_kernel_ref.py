"""tests/spk_ref.py and tests/spk_kernel_cases.py checked without a GPU: the float64 references against direct loops on small shapes, the exactness
preconditions of every exact-mode case of tests/test_gpu_spk_kernels.py, the coverage the case lists claim, the sentinel."""
from __future__ import annotations

import math
from pathlib import Path

import numpy as np
import pytest

from tests import spk_kernel_cases as K
from tests import spk_ref as R
from tests.spk_ref import T, TVALID

RNG = np.random.default_rng(7)
S, C = 2, 3
LENS = np.array([5, 160], np.int32)
X = RNG.standard_normal((S, T, C))


def test_sentinel_is_nan_in_both_widths():
    assert np.isnan(R.bf16_values(np.array([K.SENT], np.uint16))[0]) and np.isnan(K.SENT_F32)
    assert np.isnan(np.array([K.SENT], np.uint16).view(np.float16)[0])


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0, 255.0, 257.0, 0.0], np.float32)          # 1 + 2^-8 ties to even (1.0), 1 + 3 * 2^-8 ties to 1 + 2^-6
    assert R.bf16_round(x).tolist() == [1.0, 1.0, 1.015625, -3.0, 255.0, 256.0, 0.0]
    assert np.isnan(R.bf16_round(np.array([np.nan], np.float32))[0])


def test_depthwise_against_loops():
    for k in (1, 3, 7, 15):
        w = RNG.standard_normal((k, C))
        got = R.depthwise(X, w, LENS)
        pad = (k - 1) // 2
        for s in range(S):
            for t in (0, 1, 3, 4, 5, 80, 159):
                for c in range(C):
                    want = 0.0
                    if t < LENS[s]:
                        for i in range(k):
                            tt = t + i - pad
                            if 0 <= tt < LENS[s]:
                                want += X[s, tt, c] * w[i, c]
                    assert abs(got[s, t, c] - want) < 1e-12


def test_pointwise_colmean_combine_stats_against_loops():
    w, b = RNG.standard_normal((4, C)), RNG.standard_normal(4)
    y = R.pointwise(X, w, b, LENS, relu=True)
    assert abs(y[0, 2, 1] - max(X[0, 2] @ w[1] + b[1], 0.0)) < 1e-12 and np.all(y[0, 5:] == 0) and np.all(R.pointwise(X, w, b, LENS, masked=False)[0, 5:] != 0)
    assert np.allclose(R.pointwise_abs(X, w, b)[1, 7, 2], np.abs(X[1, 7]) @ np.abs(w[2]) + abs(b[2]))
    cm = R.colmean(X, LENS)
    assert np.allclose(cm[0], X[0, :5].mean(0)) and np.allclose(cm[1], X[1].mean(0))
    z, r = RNG.standard_normal((S, C)), RNG.standard_normal((S, T, C))
    o = R.combine(X, z, r, LENS)
    assert abs(o[0, 1, 2] - max(X[0, 1, 2] / (1 + math.exp(-z[0, 2])) + r[0, 1, 2], 0.0)) < 1e-12
    assert np.allclose(o[0, 7], np.maximum(r[0, 7], 0.0)) and np.all(R.combine(X, z, r, LENS, mask_out=True)[0, 5:] == 0) and np.all(R.combine(X, z, None, LENS)[0, 5:] == 0)
    mean, std = R.stats(X, LENS)
    assert np.allclose(mean[0], X[0, :5].mean(0)) and np.allclose(std[0], X[0, :5].std(0)) and np.allclose(std[1], X[1].std(0))
    const = np.ones((1, T, 2))
    assert np.allclose(R.stats(const, [9])[1], 1e-5) and np.allclose(R.stats(const * 1e20, [1])[1], 1e-5)          # the 1e-10 clamp
    swing = (1e20 * (-1.0) ** np.arange(T))[None, :, None]
    assert np.allclose(R.stats(swing, [160])[1], 1e15)                                     # variance 1e40: the 1e30 clamp


def test_featnorm_asp_linears_against_loops():
    mel = RNG.standard_normal((1, T, 80)) * 3 - 5
    fn = R.featnorm(mel)
    col = mel[0, :TVALID, 11]
    assert fn.shape == (1, TVALID, 80) and np.allclose(fn[0, :, 11], (col - col.mean()) / (col.std(ddof=1) + 1e-5))
    lg, sc, bi = RNG.standard_normal((S, T, C)), RNG.standard_normal(2 * C), RNG.standard_normal(2 * C)
    pool, (wgt, mu, var) = R.asp(X, lg, LENS, sc, bi)
    e = np.exp(lg[0, :5, 1])
    wt = e / e.sum()
    m = (wt * X[0, :5, 1]).sum()
    v = (wt * (X[0, :5, 1] - m) ** 2).sum()
    assert np.allclose(pool[0, 1], m * sc[1] + bi[1]) and np.allclose(pool[0, C + 1], math.sqrt(v) * sc[C + 1] + bi[C + 1]) and np.all(wgt[0, 5:] == 0)
    assert np.allclose(R.asp(np.ones((1, T, 1)), lg[:1, :, :1], [7], [1, 1], [0, 0])[0][0, 1], 1e-5)                   # constant x: the 1e-10 clamp
    x, w, b = RNG.standard_normal((3, 8)), RNG.standard_normal((4, 8)), RNG.standard_normal(4)
    assert np.allclose(R.linear(x, w, b, relu=True)[2, 3], max(x[2] @ w[3] + b[3], 0.0))
    mean, stdv, w1, b1 = RNG.standard_normal((S, C)), RNG.standard_normal((S, C)), RNG.standard_normal((4, 3 * C)), RNG.standard_normal(4)
    assert np.allclose(R.att_const(mean, stdv, w1, b1)[1, 2], w1[2, C:2 * C] @ mean[1] + w1[2, 2 * C:] @ stdv[1] + b1[2])
    g, c = RNG.standard_normal((S, T, 4)), RNG.standard_normal((S, 4))
    assert np.allclose(R.att_post(g, c, b1, b)[1, 9, 3], math.tanh(max(g[1, 9, 3] + c[1, 3], 0.0) * b1[3] + b[3]))


def test_gates_of_exact_mode_are_exactly_zero_or_one():
    assert math.exp(-40.0) < 2.0 ** -25 and np.float32(1.0) + np.float32(math.exp(-40.0)) == np.float32(1.0)
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(np.float32(100.0)))
    assert math.exp(-104.0) < 2.0 ** -150          # below half the smallest f32 denormal: the weight of every frame but the winner is 0


def ints_below(x, lim):
    x = np.asarray(x, np.float64)
    return np.all(x == np.round(x)) and np.all(np.abs(x) < lim)


@pytest.mark.parametrize("mode", range(4))
@pytest.mark.parametrize("i", range(len(K.GEMM_SHAPES)))
def test_gemm_exact_cases_meet_their_preconditions(i, mode):
    c = K.gemm_case(i, mode, "exact")
    ins, d = c["ins"], c["dims"]
    A = R.bf16_values(ins["A"]).reshape(d["St"], T, d["lda"])[:, :, :d["K"]]
    assert np.array_equal(R.bf16_round(ins["W"]), ins["W"]) and np.array_equal(R.bf16_bits(R.bf16_values(ins["A"])), ins["A"])
    assert R.pointwise_abs(A[1:-1], ins["W"], ins["bias"]).max() < 2 ** 24 and ints_below(A[1:-1], 2 ** 8) and ints_below(ins["W"], 4) and ints_below(ins["bias"], 16)
    assert np.all(np.abs(A[0]) == 64) and np.all(np.abs(A[-1]) == 64) and ins["lens"][0] == 160 and ins["lens"][-1] == 1
    if d["dw_k"]:
        assert ints_below(ins["dw_w"], 2) and np.all((ins["dw_w"] != 0).sum(0) == 3) and np.all((ins["dw_w"] != 0).sum(1) > 0)          # no tap is zero everywhere
    if mode == K.SG_RES:
        assert set(np.unique(ins["z"]).tolist()) <= {40.0, -100.0}
        y = ins["y_in"].reshape(d["St"], T, d["N"])[1:-1]
        assert all(np.all(y[s, L::2] == 256) and np.all(np.isnan(y[s, L + 1::2])) and ints_below(y[s, :L], 9) for s, L in enumerate(c["lens"]))
        gate_open = np.broadcast_to((ins["z"][1:-1] > 0)[:, None, :], (d["S"], T, d["N"]))
        assert gate_open.any() and np.all((256 + R.pointwise(A[1:-1], ins["W"], ins["bias"], c["lens"], masked=False))[gate_open] > 0)          # unmasked, row L would show in X
    for name, (want, bound) in c["exp"].items():
        assert bound is None
        if name in ("a_out", "x_out"):
            assert ints_below(want, 256) and np.array_equal(R.bf16_round(want.astype(np.float32)), want.astype(np.float32)), name          # <= 8 significant bits
        elif name == "y_out":
            assert ints_below(want, 2 ** 24)
    if mode == K.SG_ASP:
        margin, planted, winner_is_argmax = c["asp"]
        assert margin > 104 and planted and winner_is_argmax
        x = R.bf16_values(ins["x_in"]).reshape(d["St"], T, d["N"])[1:-1]
        assert all(np.all(x[s, L:] == 0) for s, L in enumerate(c["lens"])) and ints_below(c["exp"]["pool"][0][:, :d["N"]], 64)
        assert np.all(np.log2(np.abs(ins["bn_s"][d["N"]:])) % 1 == 0) and np.all(ins["bn_b"][d["N"]:] == 0)          # sigma * 2^k + 0: exact with or without fma


@pytest.mark.parametrize("i", range(len(K.TILE_CASES)))
def test_tile_exact_cases_meet_their_preconditions(i):
    c = K.tile_case(i, "exact")
    assert set(np.unique(c["ins"]["z"]).tolist()) <= {40.0, -100.0} and np.any(c["ins"]["z"][1:-1] > 0)
    d = c["dims"]
    y = c["ins"]["y_in"].reshape(d["St"], T, d["C"])[1:-1]
    assert all(np.all(y[s, L::2] == 64) and np.all(np.isnan(y[s, L + 1::2])) for s, L in enumerate(c["lens"]))          # loud where the gate is open: unmasked, row L would show
    if d["mode"] == K.ST_STATS:
        assert c["exp"]["mean"][1] is None and c["exp"]["stdv"][1] is not None
    for name in ("x_out", "a_out"):
        if name in c["exp"]:
            want, bound = c["exp"][name]
            assert bound is None and ints_below(want, 256)


def test_case_lists_cover_what_they_claim():
    lens, grids, kts = set(), set(), set()
    for i, (Kd, N, S_, lda, k_dw, k_res, lda_out) in enumerate(K.GEMM_SHAPES):
        lens |= set(K.lens_for(i, S_)[1:-1].tolist())
        grids.add(S_ * N // 128)
        kts.add(Kd // 32)
        assert Kd % 32 == 0 and N % 128 == 0 and lda >= Kd and lda % 8 == 0 and lda_out >= N
    assert lens == set(K.LENS_SET) and grids == {1, 3, 8, 9, 10, 16} and kts == {1, 2, 3, 4, 5, 8, 16, 32}
    assert {n for _, n, *_ in K.GEMM_SHAPES} == {128, 256, 384, 1024}
    assert {s[4] for s in K.GEMM_SHAPES} == {3, 7, 11, 15} and {s[5] for s in K.GEMM_SHAPES} == {0, 7, 11, 15}
    assert any(s[3] > s[0] for s in K.GEMM_SHAPES) and any(s[6] > s[1] for s in K.GEMM_SHAPES)
    assert {K.GEMM_SHAPES[i][0] for i in K.FORCED_LOOP0} == {256, 1024}
    assert {g & 7 == 0 for g in grids} == {True, False}                                # the XCD remap remainder both zero and non-zero
    assert {(c, s) for c, s, *_ in K.TILE_CASES} >= {(64, 1), (128, 3), (192, 1), (192, 3)} and {a for _, _, m, a in K.TILE_CASES if m == K.ST_DW} == {3, 7, 11, 15}
    assert {a for _, _, m, a in K.TILE_CASES if m == K.ST_STATS} == {1, 2}
    zs = {K.fc_slices(M, Kd, N) for Kd, N in K.FC_SITES for M in K.FC_M}
    assert 1 in zs and max(zs) > 1
    for Kd, N in K.FC_SITES + [(64, 16)]:
        for M in K.FC_M:
            assert (Kd // 16) % (4 * K.fc_slices(M, Kd, N)) == 0                       # every wave of every slice gets whole 16-deep groups
    kinds = set()
    for _, desc, _ in K.GATHER_CASES:
        for so, do, n in desc:
            kinds.add((so % 16 == 0, do % 16 == 0))
            assert so % 2 == 0 and do % 2 == 0 and n % 2 == 0
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    assert {len(d) for _, d, _ in K.GATHER_CASES} == {1, 3} and {n for _, d, _ in K.GATHER_CASES for *_, n in d} >= set(K.GATHER_BYTES)
    assert {k for k, *_ in K.DEPTHWISE_CASES} == {1, 3, 7, 11, 15} and {(c, p) for _, c, p, _ in K.DEPTHWISE_CASES} == {(80, 128), (64, 64), (320, 320)}
    rem = set()
    for i in range(6):
        rem |= {int(L) % 4 for L in K.colmean_case(i)["lens"]}
    assert rem == {0, 1, 2, 3}


@pytest.mark.parametrize("i", range(len(K.FRONT_CASES)))
def test_front_restatement_follows_the_float64_reference(i):
    c = K.front_case(i)
    got, ref = R.bf16_values(c["bits"]).astype(np.float64), c["ref"]
    assert np.all(np.abs(got - ref) <= 2.0 ** -8 * np.abs(ref) + 1e-5)
    assert np.all(got[:, :, 80:] == 0) and all(np.all(got[s, L:] == 0) for s, L in enumerate(c["lens"]))
    assert np.all(c["mel"].reshape(-1, T, c["dims"]["cpitch"])[:, TVALID:, :80] == 0)


def test_depthwise_chain_restatement_rounds_and_pins_the_order():
    """the `chain` cases: the f32 chain differs from the float64 reference (it really rounds) and from the same chain with the taps taken in descending order"""
    for i in range(len(K.DEPTHWISE_CASES)):
        c = K.depthwise_case(i, "chain")
        d = c["dims"]
        k, Cc = d["k"], d["C"]
        f32, ref = c["f32"][:, :, :Cc], c["ref"][:, :, :Cc]
        assert np.all(np.abs(f32 - ref) <= c["bound"][:, :, :Cc])
        x = c["x"].reshape(d["S"], T, d["pitch"])[:, :, :Cc]
        valid_rows = np.broadcast_to(R.mask(c["lens"]), x.shape)
        assert np.all((np.ascontiguousarray(x).view(np.uint32) & 0xFF)[valid_rows] == 0) and np.array_equal(c["w"] * 8, np.round(c["w"] * 8))
        if k >= 3:
            assert np.sum((f32 != ref.astype(np.float32))[valid_rows]) >= 20          # it rounds: not the correctly rounded exact value everywhere
            xv = np.where(R.mask(c["lens"]), x, 0.0)
            flipped = K.dw_chain_f32(xv[:, ::-1], c["w"][::-1], [T] * d["S"])[:, ::-1]          # same taps on the same frames, accumulated from the last tap down
            assert np.sum((f32 != flipped)[valid_rows]) >= 20                          # and the order shows


def test_exact_depthwise_and_colmean_restatements():
    for i in range(len(K.DEPTHWISE_CASES)):
        c = K.depthwise_case(i, "exact")
        assert np.array_equal(c["ref"].astype(np.float32).astype(np.float64), c["ref"]) and np.all(c["ref"] * 8192 == np.round(c["ref"] * 8192)) and np.abs(c["ref"]).max() < 2048
    for i in range(6):
        c = K.colmean_case(i)
        assert np.all(np.abs(c["f32"] - c["ref"]) <= c["bound"])


def test_fc_slices_matches_the_source():
    src = (Path(__file__).resolve().parent.parent / "nemotron-asr.cpp_amd" / "csrc" / "kernels_spk.hip").read_text()
    assert "if (K < 1024) return 1;" in src and "while (Z < 16 && wgs * Z < 256 && KG % (8 * Z) == 0) Z *= 2;" in src
    assert K.fc_slices(1, 6144, 128) == 16 and K.fc_slices(96, 384, 3072) == 1 and K.fc_slices(5, 1024, 128) == 16 and K.fc_slices(65, 3072, 384) == 8
