"""tests/front_ref.py and tests/front_kernel_cases.py checked without a GPU: the float32 restatements lie inside the bounds of the float64 references, every listed
wrong variant of a kernel leaves its bound or breaks its `==` (so the bounds are neither wrong nor vacuous), the case lists cover what they claim."""
from __future__ import annotations

import numpy as np
import pytest

from tests import front_kernel_cases as K
from tests import front_ref as R
from tests import offline_kernel_ref as OR
from tests.front_ref import F32, HOP, MEL_RING, NFFT


def inside(got, ref, bound):
    return bool(np.all(np.abs(got.astype(np.float64) - ref) <= bound))


def test_sentinel_is_nan_and_tables_are_the_engines():
    assert np.isnan(K.SENT_F32) and np.isnan(K.stale(2, 4)[1, 0]) and K.stale(2, 4)[0, 0] == 64.0
    cos_t, sin_t = R.twiddles()
    assert cos_t.dtype == F32 and cos_t[0] == 1 and sin_t[0] == 0 and abs(float(sin_t[128]) - 1) < 1e-7 and abs(float(cos_t[256]) + 1) < 1e-7
    assert float(np.abs(cos_t - np.cos(2 * np.pi * np.arange(512) / 512)).max()) <= R.TWIDDLE_ABS
    assert float(np.abs(sin_t - np.sin(2 * np.pi * np.arange(512) / 512)).max()) <= R.TWIDDLE_ABS
    w = R.padded_window(np.ones(400, F32))
    assert w[:56].sum() == 0 and w[456:].sum() == 0 and w[56:456].sum() == 400
    assert R.BITREV[1] == 256 and R.BITREV[3] == 384 and sorted(R.BITREV) == list(range(512))
    b = R.bands(np.array([[0, 0, 1, 2, 0], [0, 0, 0, 0, 0], [3, 0, 0, 0, 1]], F32))
    assert b.tolist() == [[2, 4], [0, 0], [0, 5]]


def test_fft_restatement_against_rfft():
    rng = np.random.default_rng(1)
    v = rng.standard_normal((3, NFFT)).astype(F32)
    cos_t, sin_t = R.twiddles()
    p = R.fft_power_f32(v, cos_t, sin_t, True)
    want = np.abs(np.fft.rfft(v.astype(np.float64), axis=1)) ** 2
    assert np.allclose(p, want, rtol=1e-4, atol=1e-3)


@pytest.fixture(scope="module")
def mel():
    case = K.mel_case("exact-max_n")
    return case, K.mel_case_reference(case)


def all_s(case, slot):
    return np.concatenate([p["s"][slot] for p in case["pushes"]])


def test_stream_case_is_what_the_issue_sets(mel):
    case, _ = mel
    p1, p2 = case["pushes"]
    assert p1["desc"][:, 1].tolist() == [2, 0, 3] and p1["desc"][1, 2] == 0 and p1["desc"][1, 5] == 0
    assert p1["desc"][0].tolist()[2:] == [1000, 256, 0, 5, MEL_RING - 2, 800] and p2["desc"][0].tolist()[2:] == [2049, 456, 1, 13, 3, 2080]
    assert (p1["max_n"] + 2047) // 2048 == 1 and (p2["max_n"] + 2047) // 2048 == 2
    up = K.mel_case("graph-upper-bound-tap")["pushes"]
    assert up[0]["max_n"] == 16 * HOP + NFFT > 2049 and up[0]["max_frames"] == 16 and up[1]["tap_cap"] == 3 < 13
    for s in K.MEL_START:
        x = case["pcm_all"][s]
        assert x.min() == -32768 and x.max() == 32767
    assert case["last0"][3] == 0.25 and np.isnan(case["last0"][1]) and np.isnan(case["pushes"][1]["abuf"][1]).all()


def test_stream_mel_restatement_is_inside_the_bound_and_two_pushes_are_one(mel):
    case, ref = mel
    one = K.mel_case("exact-max_n", pushes=(sum(K.MEL_PUSHES),))
    for s in K.MEL_START:
        s2 = all_s(case, s)
        assert s2.shape == (18, 128) and np.array_equal(s2, all_s(one, s))
        want, _ = K.logf_expect(s2)
        r, bound = ref[s]
        assert inside(want, r, bound(0.0))
        b = bound(K.LOGF_REL)          # normwise: loosest on the low filters, which the pre-emphasis attenuates
        assert float(np.median(b)) < 2e-3 and float(b.max()) < 0.5, "a vacuous bound"


WRONG_MEL = {"twiddle index j instead of j * step": dict(twiddle_stride=False), "0.96 instead of 0.97": dict(coeff=F32(0.96)), "band end one short": dict(band_end=-1),
             "re^2 + im^2 without the sqrt round trip": dict(sqrt_trip=False), "8-bit reversal": dict(rev_bits=8)}


@pytest.mark.parametrize("name", list(WRONG_MEL))
def test_wrong_stream_variants_are_seen(mel, name):
    case, ref = mel
    bad = K.mel_case("exact-max_n", **WRONG_MEL[name])
    seen_eq = seen_bound = False
    for s in K.MEL_START:
        good_s, bad_s = all_s(case, s), all_s(bad, s)
        gw, gb = K.logf_expect(good_s)
        bw, _ = K.logf_expect(bad_s)
        seen_eq |= not inside(bw, gw, gb) or not np.array_equal(case["pushes"][1]["abuf"], bad["pushes"][1]["abuf"])
        r, bound = ref[s]
        seen_bound |= not inside(bw, r, bound(K.LOGF_REL))
    assert seen_eq, "the exact-up-to-logf comparison does not see this variant"
    if name != "re^2 + im^2 without the sqrt round trip":          # 3 u of the power: inside any float64 bound, seen by the exact comparison alone
        assert seen_bound, "the float64 bound does not see this variant"


def test_empty_filter_gives_log_of_the_guard():
    case = K.mel_case("empty-filter")
    assert case["tables"][2][5].tolist() == [0, 0]
    s = all_s(case, 2)
    assert np.all(s[:, 5] == 0) and np.all(s[:, 4] > 0)
    want, bound = K.logf_expect(s)
    assert np.all(np.abs(want[:, 5] - np.log(2.0 ** -24)) == 0) and np.all(bound[:, 5] > 0)
    r, b = K.mel_case_reference(case)[2]
    assert inside(want, r, b(0.0))


# ---- convolutions -----------------------------------------------------------------------------------------------------------------------------------------
def test_conv0_cases_cover_the_three_splits_and_the_wrap():
    for Rc, (chunk_mel, H1, H2) in {0: (17, 9, 5), 1: (25, 13, 7)}.items():
        assert K.conv0_dims(Rc) == (chunk_mel, H1, H2)
        assert [K.conv0_fz(H2, B) for B in K.CONV0_B[Rc]] == [11, 3, 3, 1]
        assert [H2 * B <= 64 for B in K.CONV0_B[Rc]][:2] == [True, False] and [H2 * B <= 512 for B in K.CONV0_B[Rc]][2:] == [True, False]
    assert K.conv0_dims("even") == (16, 9, 5) and [K.conv0_fz(5, B) for B in K.CONV0_B["even"]] == [11, 3, 3, 1]
    reach = {Rc: 4 * (K.conv0_dims(Rc)[2] - 1) - K.conv0_dims(Rc)[0] for Rc in K.CONV0_B}          # last mel row a patch reaches, minus chunk_mel
    assert reach == {0: -1, 1: -1, "even": 0}, "only the even chunk reads a row behind the chunk"
    assert any(MEL_RING - 5 <= ms < MEL_RING for _, ms in K.CONV0_COMBOS) and len({s for s, _ in K.CONV0_COMBOS}) == 3
    c = K.conv0_case(1)
    used = np.zeros((3, MEL_RING), int)
    for (slot, ms), mel in zip(K.CONV0_COMBOS, c["chunks"]):
        rows = (ms + np.arange(-2, 27)) % MEL_RING
        used[slot, rows] += 1
        assert np.array_equal(c["ring"][slot, rows[2:-2]], mel)
        assert np.isnan(c["ring"][slot, rows[0], 0]) and c["ring"][slot, rows[1], 0] == 64 and c["ring"][slot, rows[-2], 0] == 64 and np.isnan(c["ring"][slot, rows[-1], 0])
    assert used.max() == 1
    f32, ref, bound = K.conv0_expect(c, 3)
    assert f32.shape == (7, 33, 256) and inside(f32, ref, bound) and float((bound / (np.abs(ref) + 1)).max()) < 1e-4


def test_dw_restatement_bound_and_wrong_variants():
    for Hin, (Bs, Bl) in K.DW_CASES.items():
        Hout = Hin // 2 + 1
        assert Hout * Bs <= 511 and Hout * Bl >= 512 and K.dw_kernel(Hin, Bs, 0) == "k_sub_dw<false>" and K.dw_kernel(Hin, Bl, 1) == "k_sub_dw_row<true>"
    x, wt, bias, w = K.dw_case(5)
    x = x[:4]
    f32 = R.dw_f32(x, wt, bias)
    assert f32.shape == (4, 3, 17, 256) and 17 == 4 * 4 + 1
    ref, bound = K.dw_reference(x, w, bias, range(4))
    assert inside(f32, ref, bound)
    direct = sum(float(w[7, kh, kw]) * float(x[2, 2 * 1 + kh - 2, 2 * 16 + kw - 2, 7]) for kh in range(3) for kw in range(3) if 2 * 16 + kw - 2 < 33) + float(bias[7])
    assert abs(ref[2, 1, 16, 7] - direct) < 1e-9
    swapped = R.dw_f32(x, wt, bias, swap_taps=True)
    assert np.any(swapped != f32) and inside(swapped, ref, bound), "a swapped tap order must break `==` (and only `==`)"
    dropped = np.where(np.isnan(R.dw_f32(x, wt, bias, w_out=16)), K.SENT_F32, f32)
    assert np.isnan(dropped[:, :, 16]).all() and not np.array_equal(dropped, f32, equal_nan=True)
    assert OR.conv3x3_s2(x[0], w, bias, True).shape == (3, 17, 256)


# ---- diarization mel --------------------------------------------------------------------------------------------------------------------------------------
def test_diar_interior_frames_from_the_reference_alone():
    """frame t of the window at 160 i is frame t + 1 of the window at 160 (i - 1) exactly where neither frame touches its window's edges"""
    d = K.DIAR_SHAPES["vad"]
    tables, fb = K.diar_tables("vad")
    x = K.diar_audio("vad", True)
    off = K.diar_offsets()
    same = []
    for t in range(d["t_valid"] - 1):
        a = R.diar_windowed(x[off[1]:], d["n_win"], t, tables[0], True, f64=True)[0]
        b = R.diar_windowed(x[off[0]:], d["n_win"], t + 1, tables[0], True, f64=True)[0]
        if np.array_equal(a, b):
            same.append(t)
    interior = K.diar_interior(d["n_win"], d["t_valid"])
    assert interior == list(range(2, 62)) and same == [t for t in interior if t + 1 in interior] == list(range(2, 61))
    assert [t in interior for t in K.DIAR_FRAME_T] == [False, False, True, False]


@pytest.mark.parametrize("s16", [False, True])
def test_diar_restatement_is_inside_the_bound_and_wrong_variants_are_seen(s16):
    d = K.DIAR_SHAPES["vad"]
    tables, fb = K.diar_tables("vad")
    x = K.diar_audio("vad", s16)
    o = int(K.diar_offsets()[1])
    ts = [0, 1, 2, 30, 61, 62]
    s = R.diar_frames_f32(x[o:], d["n_win"], ts, tables, s16)
    want, lb = K.logf_expect(s)
    ref, bound = K.diar_reference(x[o:], d["n_win"], ts, tables, fb, s16)
    assert inside(want, ref, bound(0.0)) and float(np.median(bound(K.LOGF_REL))) < 2e-3
    before = float(x[o - 1]) / (32768.0 if s16 else 1.0)
    bad = R.diar_frames_f32(x[o:], d["n_win"], ts, tables, s16, before=before)          # the restart at sample 0 dropped
    bw, _ = K.logf_expect(bad)
    assert not inside(bw[:2], want[:2], lb[:2]) and not inside(bw[:2], ref[:2], bound(K.LOGF_REL)[:2]) and np.array_equal(bad[2:], s[2:])


@pytest.mark.parametrize("s16", [False, True])
@pytest.mark.parametrize("shape", list(K.DIAR_SHAPES))
def test_featnorm_bound_makes_a_statement_on_the_product_shapes(shape, s16):
    d = K.DIAR_SHAPES[shape]
    tables, fb = K.diar_tables(shape)
    x = K.diar_audio(shape, s16)
    for o in K.diar_offsets():
        ref, bound = K.diar_reference(x[o:], d["n_win"], range(d["t_valid"]), tables, fb, s16)
        nb = R.featnorm_bound(ref, bound(K.LOGF_REL))
        assert np.isfinite(nb).all() and float(np.median(nb)) < 1e-2, (float(np.median(nb)), float(nb.max()))


def test_featnorm_restatement_bound_and_wrong_denominator():
    rng = np.random.default_rng(5)
    for n in (1, 2, 63, 150):
        x64 = -8 + 3 * rng.standard_normal((n, 80))
        x = x64.astype(F32)
        got = R.featnorm_f32(x)
        e = np.abs(x.astype(np.float64) - x64)
        ref, _, _ = R.featnorm_f64(x64)
        bound = R.featnorm_bound(x64, e)
        assert inside(got, ref, bound), n
        if n == 1:
            assert np.all(got == 0)
        if n >= 2:
            bad = R.featnorm_f32(x, denom_wrong=True)
            assert not inside(bad, ref, bound) and np.any(bad != got), n


# ---- stream state -----------------------------------------------------------------------------------------------------------------------------------------
def test_checksum_is_the_documented_sum():
    def fmix(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)
    words = np.array([0, 1, 0xFFFFFFFF, 0xFFC5FFC5, 12345], np.uint32)
    want = sum(fmix(int(w) ^ (((7 + i) * 0x9E3779B1) & 0xFFFFFFFF)) for i, w in enumerate(words))
    assert R.checksum(words, 7) == want and R.checksum(words, 8) != want
    assert R.checksum(words[:2], 7) + R.checksum(words[2:], 9) == want          # any cut into pieces gives the same value
    assert (R.greedy_start(0, 77, 1), R.greedy_start(1, 77, 1), R.greedy_start(1, 77, 0)) == (0, 77, -1)


def test_piece_plan_covers_the_edges_and_is_disjoint():
    pieces, sb, db = K.piece_plan()
    vec = [p for p in pieces if not K.piece_is_words(p)]
    words = [p for p in pieces if K.piece_is_words(p)]
    assert sorted(int(p[2]) // 16 for p in vec) == sorted(K.VEC_PIECES) and sorted(int(p[2]) for p in words) == [4, 12, 20, 1028]
    assert any(p[0] & 15 for p in words) and any(p[1] & 15 and not p[0] & 15 for p in words) and any(not (p[0] | p[1]) & 15 and p[2] & 15 for p in words)
    assert {v % 1024 for v in K.VEC_PIECES} >= {1, 255, 256, 1023, 0, 3}
    for col in (0, 1):
        spans = sorted((int(p[col]), int(p[col]) + (int(p[2]) + 15) // 16 * 16) for p in pieces)
        assert all(a[1] + 16 <= b[0] for a, b in zip(spans, spans[1:])) and spans[0][0] >= 16 and spans[-1][1] + 16 <= (sb, db)[col]
    src = np.random.default_rng(3).integers(0, 256, sb, dtype=np.uint8)
    img, sums = K.pieces_expect(pieces, src, db, 1)
    back, sums2 = K.pieces_expect(np.stack([pieces[:, 1], pieces[:, 0], pieces[:, 2], pieces[:, 3]], 1), img, sb, 2)
    assert sums == sums2 and all(np.array_equal(back[p[0]:p[0] + p[2]], src[p[0]:p[0] + p[2]]) for p in pieces)
    no_pad = sum(R.checksum(src[p[0]:p[0] + p[2]].view(np.uint32), p[3]) for p in words)
    assert no_pad != sum(s for p, s in zip(pieces, sums) if K.piece_is_words(p)), "the padding words count"


def test_reset_cases_cover_the_options():
    rows = K.reset_window_rows(K.RESET["kv_head"])
    assert len(rows) == 70 and rows.max() == R.KVC - 1 and rows.min() == 0 and len(set(rows.tolist())) == 70
    cs = K.RESET_CASES
    assert {c["esz"] for c in cs} == {2, 4} and {c["keep"] for c in cs} == {0, 1} and {c["aud"] for c in cs} == {True, False} and {c["boost"] for c in cs} == {True, False}
    assert any(c["lm"] is None for c in cs) and {c["lm"][2] for c in cs if c["lm"]} == {0, 1}
