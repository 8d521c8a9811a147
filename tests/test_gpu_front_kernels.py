"""Every kernel of kernels_front.hip, alone, against a float64 reference of the operation (tests/front_ref.py).

tests/helpers/front_harness.hip makes ONE call of a product launcher -- launch_mel, launch_mel_put, launch_mel_zero, launch_stream_reset, launch_stream_fork,
launch_stream_pack, launch_stream_unpack, launch_sub_conv0_dw, launch_sub_dw, launch_diar_logmel, launch_diar_frames -- on buffers [guard | body | guard] whose every
byte that is not an input is the sentinel 0xFFC5 (NaN as f32 and as bf16), and returns every buffer whole.  The buffer plumbing (Dev, GUARD, SENT, check_bounded) is
tests/test_gpu_layer_kernels.py's.  Cases -- operands, expectations, the terms of the bounds -- are numpy only and live in tests/front_kernel_cases.py, where
tests/test_front_kernel_ref.py checks them without a GPU; the two modes (exact `==`, bounded against float64) are described there.

After every launch: every buffer the launch may write is compared WHOLE with its expected image (the uploaded bytes, the sentinel, and the launch's own writes), so
a write outside what the kernel owns -- another slot, another parity, a ring row outside the window, the bytes between two pieces -- fails the test; every read-only
buffer is checked bit for bit on exit (Dev.check_inputs).  Stale rows next to what a kernel reads alternate between a loud finite value and the sentinel.

The one measured constant is LOGF_REL (test_device_logf: the harness's own k_libm against float64).  No tolerance is measured on a kernel under test.  Largest
observed fractions of the bounds, the module's wall time and the mutation table: profiles/front_kernels.md."""
from __future__ import annotations

import ctypes as C
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi
from tests import front_kernel_cases as K
from tests import front_ref as R
from tests import spk_ref as SR
from tests.front_ref import ABUF_CAP, F32, HOP, MEL_RING, NFFT, NMEL, SUBC
from tests.test_gpu_layer_kernels import SENT, Dev, check_bounded

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HELPER = ROOT / "tests" / "helpers" / "libfront_harness.so"
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"
FRACTIONS = {}            # kernel -> largest observed |got - ref| / bound
CLAIMED = {"k_preemph", "k_melframes", "k_abuf_shift", "k_mel_put", "k_mel_zero", "k_stream_reset", "k_stream_fork", "k_stream_pack", "k_stream_unpack",
           "k_diar_logmel", "k_diar_frames", "k_diar_featnorm"}            # the template instantiations: conv0_kernel() and K.dw_kernel() of the runs below
LOGF_HI = 2.0 ** 16       # every case's mel sum lies below (asserted where the sums are compared)


@lru_cache(maxsize=None)
def harness():
    if not HELPER.exists():
        pytest.fail("tests/helpers/libfront_harness.so not built: __graft_entry__.build() warns when the helper fails to compile (a changed MelParams, StreamResetParams, "
                    "DiarMelParams or launcher of kernels_front.hip?); these tests do not skip")
    C.CDLL(str(capi.LIB_PATH), mode=C.RTLD_GLOBAL)          # the helper's undefined nasr:: symbols resolve against the product library
    L = C.CDLL(str(HELPER))
    L.front_harness_error.restype = C.c_char_p
    L.front_harness_alloc.argtypes = [C.c_longlong, C.c_int]
    L.front_harness_total_bytes.restype = C.c_longlong
    L.front_harness_put.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_longlong]
    L.front_harness_get.argtypes = [C.c_int, C.c_void_p]
    L.front_harness_mel.argtypes = [C.c_void_p, C.c_void_p]
    L.front_harness_mel_ring.argtypes = [C.c_int] * 7 + [C.c_void_p]
    L.front_harness_pieces.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_int]
    L.front_harness_reset.argtypes = [C.c_void_p]
    L.front_harness_conv0.argtypes = [C.c_int] * 13 + [C.c_void_p]
    L.front_harness_diar_logmel.argtypes = [C.c_void_p] + [C.c_int] * 8
    L.front_harness_diar_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    assert L.front_harness_sentinel() == SENT == K.SENT
    assert [L.front_harness_constant(i) for i in range(15)] == [NMEL, R.NBINS, NFFT, HOP, MEL_RING, ABUF_CAP, R.KVC, R.LCTX, R.D, R.HID, R.PRE_CACHE, SUBC, R.DIAR_NMEL,
                                                               R.HIST_MAX, R.BLANK]
    assert [L.front_harness_constant(i) for i in range(15, 20)] == [40, 32, 24, 4 * len(R.DECCTRL_FIELDS), 16]
    return L


def device():
    return Dev(harness(), "front_harness")


def ok(dev, rc):
    """a refused case is a failed test; an error of the device itself ends the session: nothing more is started on a GPU that has faulted"""
    if rc != 0 and dev.err().startswith(("hipDeviceSynchronize", "launch:")):
        pytest.exit(f"the device reported an error, no further GPU test is run: {dev.err()}", returncode=3)
    assert rc == 0, dev.err()


def ints(*v):
    return np.ascontiguousarray(np.array(v, np.int32).reshape(-1))


def p(arr):
    return arr.ctypes.data


def is_sent(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint16) == SENT))


def body(dev, h, dtype, n, what):
    """the first n elements of a buffer; everything behind them (and the guards: Dev.get) still the sentinel"""
    b = dev.get(h, dtype)
    assert is_sent(b[n:]), f"{what}: written behind its {n} elements"
    return b[:n]


def same_image(dev, h, want, what):
    """the whole buffer equals the expected image, bit for bit"""
    want = np.ascontiguousarray(want)
    got = body(dev, h, np.uint8, want.nbytes, what)
    bad = np.flatnonzero(got != want.reshape(-1).view(np.uint8))
    assert bad.size == 0, f"{what}: {bad.size} bytes differ from the expected image, first at byte {bad[0]} (element {bad[0] // want.itemsize} of shape {want.shape})"


def compare(kernel, what, got, want, bound, out_rel=0.0):
    assert np.all(np.isfinite(got)), f"{kernel} {what}: not finite where owned"
    if bound is None:
        bad = np.argwhere(got != want.astype(np.float32))
        assert bad.size == 0, f"{kernel} {what}: {len(bad)} elements differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    else:
        ratio = check_bounded(got.astype(np.float64), want, bound, out_rel, f"{kernel} {what}")
        FRACTIONS[kernel] = max(FRACTIONS.get(kernel, 0.0), ratio)


def up_tables(dev, tables):
    return [dev.up(t) for t in tables]


# ---- the one measured constant ----------------------------------------------------------------------------------------------------------------------------
def test_device_logf():
    """logf as the device computes it against float64: 150 000 points log-spaced over [2^-24, 2^16], the range of the cases' mel sums, and 50 001 around 1.  The
    recorded maximum times 4 is LOGF_REL; a device whose logf is worse than that fails here, not in a kernel test."""
    x = np.concatenate([np.exp(np.linspace(np.log(2.0 ** -24), np.log(LOGF_HI), 150000)), np.linspace(0.5, 2.0, 50001)]).astype(F32)
    assert x.size == 200001
    with device() as dev:
        hx, hy = dev.up(x), dev.new(x.nbytes)
        ok(dev, dev.L.front_harness_libm(hx, hy, x.size))
        y = body(dev, hy, F32, x.size, "logf").astype(np.float64)
    ref = np.log(x.astype(np.float64))
    nz = ref != 0
    assert np.all(y[~nz] == 0)
    worst = float((np.abs(y - ref)[nz] / np.abs(ref)[nz]).max())
    print(f"device logf, max relative deviation from float64 over {x.size} points: {worst:.3e}")
    assert worst <= K.LOGF_REL, worst


# ---- launch_mel: k_preemph, k_melframes, k_abuf_shift -------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def mel_case(variant, pushes=K.MEL_PUSHES):
    return K.mel_case(variant, pushes=pushes)


def run_mel(dev, case):
    """every push of the case on one set of buffers -> slot -> the frames the launches wrote [F][128].  After each push: abuf and last_sample are their expected images;
    the ring holds the frames of all pushes so far at their (wrapping) rows and the sentinel everywhere else; the tap holds the first tap_cap frames of each row"""
    L = dev.L
    tabs = up_tables(dev, case["tables"])
    abuf, last = dev.up(case["abuf0"], written=True), dev.up(case["last0"], written=True)
    ring = dev.new(K.MEL_POOL * MEL_RING * NMEL * 4)
    frames = {s: [] for s in K.MEL_START}
    owned = np.zeros((K.MEL_POOL, MEL_RING), bool)
    for push in case["pushes"]:
        desc, B, cap = push["desc"], len(push["desc"]), push["tap_cap"]
        tab, pcm = dev.new(B * 40), dev.up(push["pcm"])
        tap = dev.new(B * cap * NMEL * 4) if cap else -1
        a = ints(tab, pcm, B, push["max_frames"], abuf, last, ring, *tabs, tap, cap, push["max_n"], K.MEL_POOL)
        ok(dev, L.front_harness_mel(p(a), p(desc)))
        same_image(dev, abuf, push["abuf"], "abuf")
        same_image(dev, last, push["last"], "last_sample")
        r = body(dev, ring, F32, K.MEL_POOL * MEL_RING * NMEL, "mel_ring").reshape(K.MEL_POOL, MEL_RING, NMEL)
        t = body(dev, tap, F32, B * cap * NMEL, "tap").reshape(B, cap, NMEL) if cap else None
        for b, d in enumerate(desc):
            slot, nf, wpos = int(d[1]), int(d[5]), int(d[6])
            rows = (wpos + np.arange(nf)) % MEL_RING
            assert not owned[slot, rows].any()
            owned[slot, rows] = True
            if nf:
                got = r[slot, rows]
                s = push["s"][slot]
                assert float(s.max()) < LOGF_HI
                compare("k_melframes", f"slot {slot}: log of the float32 restatement's sum", got, *K.logf_expect(s))
                frames[slot].append(got)
            if cap:
                keep = min(nf, cap)
                assert np.array_equal(t[b, :keep].view(np.uint32), r[slot, rows[:keep]].view(np.uint32)) and is_sent(t[b, keep:]), "tap"
        assert is_sent(r[~owned]), "mel_ring: a row outside the frames of the pushes was written"
    return {s: np.concatenate(f) for s, f in frames.items()}


@pytest.mark.parametrize("variant", list(K.MEL_VARIANTS))
def test_stream_mel(variant):
    case = mel_case(variant)
    with device() as dev:
        got = run_mel(dev, case)
    for slot, (ref, bound) in K.mel_case_reference(case).items():
        compare("k_melframes", f"slot {slot} against float64", got[slot], ref, bound(K.LOGF_REL))
    if K.MEL_VARIANTS[variant]["zero_row"] is not None:
        assert np.all(got[2][:, 5] == F32(np.log(2.0 ** -24)))


def test_two_pushes_have_the_bits_of_one_push():
    two, one = mel_case("exact-max_n"), mel_case("exact-max_n", (sum(K.MEL_PUSHES),))
    with device() as dev:
        a = run_mel(dev, two)
    with device() as dev:
        b = run_mel(dev, one)
    for slot in K.MEL_START:
        assert a[slot].shape == (18, NMEL) and np.array_equal(a[slot].view(np.uint32), b[slot].view(np.uint32))


@pytest.mark.parametrize("which", [0, 1], ids=["k_mel_put", "k_mel_zero"])
def test_mel_put_and_zero(which):
    desc, staged, max_frames, pool = K.mel_ring_case()
    want = K.sent_f32((pool, MEL_RING, NMEL))
    for b, (slot, nf, wpos) in enumerate(desc):
        want[slot, (wpos + np.arange(nf)) % MEL_RING] = staged[b, :nf] if which == 0 else 0
    with device() as dev:
        ring = dev.new(want.nbytes)
        ok(dev, dev.L.front_harness_mel_ring(which, dev.up(staged), dev.new(len(desc) * 40), ring, len(desc), max_frames, pool, p(desc)))
        same_image(dev, ring, want, "mel_ring")


# ---- k_sub_conv0_dw -----------------------------------------------------------------------------------------------------------------------------------------
def conv0_kernel(bf16):
    return f"k_sub_conv0_dw<{'true' if bf16 else 'false'}>"


@lru_cache(maxsize=None)
def conv0_expected(Rc):
    case = K.conv0_case(Rc)
    exp = [K.conv0_expect(case, k) for k in range(len(K.CONV0_COMBOS))]
    return case, tuple(np.stack([e[i] for e in exp]) for i in range(3))


@pytest.mark.parametrize("bf16", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("Rc", list(K.CONV0_B))
def test_sub_conv0_dw(Rc, bf16):
    """the four batch sizes around H2 B = 64 and 512: fz = 11, 3, 3, 1 column splits on the same chunks -- the same bits"""
    case, (f32, ref, bound) = conv0_expected(Rc)
    H2, nk = case["H2"], len(K.CONV0_COMBOS)
    w0, b0, w2, b2 = case["w"]
    first = None
    with device() as dev:
        ring = dev.up(case["ring"])
        hw = [dev.up(a) for a in (K._Chunk.wt(None, w0), b0, K._Chunk.wt(None, w2), b2)]
        for B in K.CONV0_B[Rc]:
            rows = np.array([K.CONV0_COMBOS[b % nk] for b in range(B)], np.int32)
            n = B * H2 * 33 * SUBC
            out = dev.new(n * (2 if bf16 else 4))
            ok(dev, dev.L.front_harness_conv0(dev.new(B * 32), ring, *hw, out, bf16, B, case["chunk_mel"], case["H1"], 65, 3, p(rows)))
            bits = body(dev, out, np.uint16 if bf16 else np.uint32, n, "out").reshape(B, H2, 33, SUBC)
            got = SR.bf16_values(bits) if bf16 else bits.view(F32)
            k = np.arange(B) % nk
            what = f"B = {B} (fz = {K.conv0_fz(H2, B)})"
            if not bf16:
                compare(conv0_kernel(bf16), what + " float32 restatement", got, f32[k], None)
            compare(conv0_kernel(bf16), what, got, ref[k], bound[k], 2.0 ** -8 if bf16 else 0.0)
            if first is None:
                first = bits[:nk].copy()
            assert np.array_equal(bits[:nk], first) and np.array_equal(bits[B - B % nk - nk:B - B % nk], first), what + ": another column split, other bits"


# ---- k_sub_dw / k_sub_dw_row ----------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def dw_expected(Hin):
    x, wt, bias, w = K.dw_case(Hin)
    Bs, Bl = K.DW_CASES[Hin]
    entries = [0, 1, 2, Bs - 1, Bl - 1]
    return x, wt, bias, R.dw_f32(x, wt, bias), entries, K.dw_reference(x, w, bias, entries)


@pytest.mark.parametrize("bf16", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("Hin", list(K.DW_CASES))
def test_sub_dw_and_row_kernel(Hin, bf16):
    """k_sub_dw (Hout B <= 511) and k_sub_dw_row (>= 512) on the same input prefix: the same bits, the float32 restatement's"""
    x, wt, bias, f32, entries, (ref, bound) = dw_expected(Hin)
    Hout, Wout = Hin // 2 + 1, K.DW_WIN // 2 + 1
    bits = {}
    with device() as dev:
        hx, hw, hb = dev.up(x), dev.up(wt), dev.up(bias)
        for B in K.DW_CASES[Hin]:
            n = B * Hout * Wout * SUBC
            out = dev.new(n * (2 if bf16 else 4))
            ok(dev, dev.L.front_harness_dw(hx, hw, hb, out, bf16, B, Hin, K.DW_WIN))
            kernel = K.dw_kernel(Hin, B, bf16)
            CLAIMED.add(kernel)
            bits[B] = body(dev, out, np.uint16 if bf16 else np.uint32, n, "out").reshape(B, Hout, Wout, SUBC)
            got = SR.bf16_values(bits[B]) if bf16 else bits[B].view(F32)
            if bf16:
                assert np.array_equal(bits[B], SR.bf16_bits(f32[:B])), f"{kernel}: not the bf16 rounding of the float32 restatement"
            else:
                compare(kernel, "float32 restatement", got, f32[:B], None)
            e = [i for i, b in enumerate(entries) if b < B]
            compare(kernel, "against float64", got[[entries[i] for i in e]], ref[e], bound[e], 2.0 ** -8 if bf16 else 0.0)
    Bs, Bl = K.DW_CASES[Hin]
    assert np.array_equal(bits[Bs], bits[Bl][:Bs]), "k_sub_dw and k_sub_dw_row differ on the shared batch entries"


# ---- k_diar_logmel, k_diar_featnorm, k_diar_frames ------------------------------------------------------------------------------------------------------------
def diar_args(dev, tables, x, s16):
    return ints(dev.up(x), int(s16), *up_tables(dev, tables))


def run_diar_logmel(dev, a, hoff, W, d, normalize):
    n = W * d["T_pad"] * d["cpitch"]
    mel = dev.new(n * 4 + d["T_pad"] * d["cpitch"] * 4)          # a neighbour window's rows behind: must stay the sentinel
    ok(dev, dev.L.front_harness_diar_logmel(p(a), hoff, mel, W, d["n_win"], d["T_pad"], d["t_valid"], d["cpitch"], normalize))
    got = body(dev, mel, F32, n, "mel").reshape(W, d["T_pad"], d["cpitch"])
    assert np.all(got[:, d["t_valid"]:].view(np.uint32) == 0) and np.all(got[:, :, 80:].view(np.uint32) == 0), "frames >= t_valid and columns >= 80 are exactly 0.0"
    return got[:, :d["t_valid"], :80]


def check_diar(shape, s16, d, W):
    tables, fb = K.diar_tables(shape)
    x, off = K.diar_audio(shape, s16), K.diar_offsets()[:W]
    ts = list(range(d["t_valid"]))
    with device() as dev:
        a, hoff = diar_args(dev, tables, x, s16), dev.up(off)
        plain = run_diar_logmel(dev, a, hoff, W, d, 0)
        normed = run_diar_logmel(dev, a, hoff, W, d, 1)
    for w in range(W):
        xw = x[off[w]:]
        s = R.diar_frames_f32(xw, d["n_win"], ts, tables, s16)
        assert float(s.max()) < LOGF_HI
        compare("k_diar_logmel", f"window {w}: log of the float32 restatement's sum", plain[w], *K.logf_expect(s))
        ref, bound = K.diar_reference(xw, d["n_win"], ts, tables, fb, s16)
        e = bound(K.LOGF_REL)
        compare("k_diar_logmel", f"window {w} against float64", plain[w], ref, e)
        compare("k_diar_featnorm", f"window {w}: float32 restatement on the kernel's own log-mel", normed[w], R.featnorm_f32(plain[w]), None)
        nb = R.featnorm_bound(ref, e)
        assert np.isfinite(nb).all() if d["t_valid"] > 2 else np.isfinite(nb).mean() >= 0.5
        compare("k_diar_featnorm", f"window {w} against float64", normed[w], R.featnorm_f64(ref)[0], nb)


@pytest.mark.parametrize("s16", [False, True], ids=["float", "s16"])
@pytest.mark.parametrize("shape", list(K.DIAR_SHAPES))
def test_diar_logmel_and_featnorm(shape, s16):
    check_diar(shape, s16, K.DIAR_SHAPES[shape], K.DIAR_W)


@pytest.mark.parametrize("t_valid", [1, 2])
def test_diar_featnorm_denominator(t_valid):
    """max(n - 1, 1): one valid frame normalises to exactly 0, two divide by 1"""
    check_diar("vad", True, dict(n_win=10080, T_pad=16, t_valid=t_valid, cpitch=80), 2)


@pytest.mark.parametrize("s16", [False, True], ids=["float", "s16"])
def test_diar_frames_and_the_shared_interior_frame(s16):
    """nasr_diar.hip's shared-frame VAD: interior frame t of the window at 160 i has the bits of frame t + 1 of the window at 160 (i - 1)"""
    d = K.DIAR_SHAPES["vad"]
    tables, fb = K.diar_tables("vad")
    x, off = K.diar_audio("vad", s16), K.diar_offsets()
    interior = K.diar_interior(d["n_win"], d["t_valid"])
    ts = sorted(set(K.DIAR_FRAME_T) | {t + 1 for t in K.DIAR_FRAME_T if t in interior and t + 1 in interior})
    desc = np.array([(off[w], d["n_win"], t) for w in range(K.DIAR_W) for t in ts], np.int64)
    n = len(desc)
    with device() as dev:
        a, out = diar_args(dev, tables, x, s16), dev.new(n * 80 * 4 + 320)
        ok(dev, dev.L.front_harness_diar_frames(p(a), dev.new(n * 16), out, p(desc), n))
        got = body(dev, out, F32, n * 80, "out").reshape(K.DIAR_W, len(ts), 80)
    for w in range(K.DIAR_W):
        xw = x[off[w]:]
        compare("k_diar_frames", f"window {w}: log of the float32 restatement's sum", got[w], *K.logf_expect(R.diar_frames_f32(xw, d["n_win"], ts, tables, s16)))
        ref, bound = K.diar_reference(xw, d["n_win"], ts, tables, fb, s16)
        compare("k_diar_frames", f"window {w} against float64", got[w], ref, bound(K.LOGF_REL))
    shared = [t for t in ts if t in interior and t + 1 in ts and t + 1 in interior]
    assert shared
    for w in range(1, K.DIAR_W):
        for t in shared:
            assert np.array_equal(got[w, ts.index(t)].view(np.uint32), got[w - 1, ts.index(t + 1)].view(np.uint32)), (w, t)
    assert not np.array_equal(got[1, ts.index(0)], got[0, ts.index(1)]), "frame 0 holds the window's left padding: it is not its neighbour's frame 1"


# ---- k_stream_fork, k_stream_pack, k_stream_unpack ------------------------------------------------------------------------------------------------------------
def run_pieces(dev, which, pieces, hs, hd, n_sums=None):
    n = len(pieces) if n_sums is None else n_sums
    tab = dev.new(max(len(pieces), 1) * 24)
    sums = dev.new((len(pieces) + 2) * 8) if which else -1
    ok(dev, dev.L.front_harness_pieces(which, tab, hs, hd, sums, p(np.ascontiguousarray(pieces, np.int64)), n))
    return [int(v) for v in body(dev, sums, np.uint64, n, "sums")] if which else None


def test_stream_fork():
    pieces, sb, db = K.piece_plan()
    src = K.rng_of("fork-src").integers(0, 256, sb, dtype=np.uint8)
    want, _ = K.pieces_expect(pieces, src, db, 0)
    with device() as dev:
        hs, hd = dev.up(src), dev.new(db)
        run_pieces(dev, 0, pieces, hs, hd)
        same_image(dev, hd, want[:db], "the fork's destination")
    with device() as dev:
        hs, hd = dev.up(src), dev.new(db)
        run_pieces(dev, 0, pieces, hs, hd, n_sums=0)
        assert is_sent(dev.get(hd, np.uint8)), "n_pieces = 0 wrote"


def test_stream_pack_and_unpack():
    pieces, sb, db = K.piece_plan()
    src = K.rng_of("pack-src").integers(0, 256, sb, dtype=np.uint8)
    staged, sums = K.pieces_expect(pieces, src, db, 1)
    back = np.stack([pieces[:, 1], pieces[:, 0], pieces[:, 2], pieces[:, 3]], 1)
    slot, sums_back = K.pieces_expect(back, staged, sb, 2)
    assert sums_back == sums
    with device() as dev:
        hs, hd = dev.up(src), dev.new(db)
        assert run_pieces(dev, 1, pieces, hs, hd) == sums
        same_image(dev, hd, staged[:db], "the staging buffer")          # the padding words of a word piece: zero
        dev.frozen[hd] = dev.raw(hd)
        h2 = dev.new(sb)
        assert run_pieces(dev, 2, back, hd, h2) == sums
        same_image(dev, h2, slot[:sb], "the restored slot")              # the padding is not written to the slot
        for so, _, b, _ in pieces:
            assert np.array_equal(slot[so:so + b], src[so:so + b])
        hz = dev.new(db)
        ok(dev, dev.L.front_harness_pieces(1, dev.new(256), hs, hz, dev.new(256), p(np.ascontiguousarray(pieces, np.int64)), 0))
        assert is_sent(dev.get(hz, np.uint8)), "n_pieces = 0 wrote"


# ---- k_stream_reset -------------------------------------------------------------------------------------------------------------------------------------------
def sent_bytes(*shape):
    return np.full(int(np.prod(shape)) // 2, SENT, np.uint16).view(np.uint8).reshape(shape).copy()


@pytest.mark.parametrize("i", range(len(K.RESET_CASES)))
def test_stream_reset(i):
    c, g = K.RESET_CASES[i], K.RESET
    nl, ns, slot, esz, ccf = g["n_layers"], g["n_slots"], g["slot"], c["esz"], g["cc_slot_floats"]
    L = harness()
    gsize, at_attached, at_start = (L.front_harness_constant(k) for k in (20, 21, 22))
    want = dict(kv=sent_bytes(nl, ns, 2, R.KVC, R.D * esz), cc=sent_bytes(nl, ns, ccf * 4), abuf=sent_bytes(ns, 2, ABUF_CAP * 4), last=sent_bytes(ns, 4),
                ring=sent_bytes(ns, MEL_RING, NMEL * 4), dec_h=sent_bytes(ns, 4 * R.HID * 4), dec_c=sent_bytes(ns, 4 * R.HID * 4), ctrl=sent_bytes(ns, 48),
                boost=sent_bytes(ns, 4), lm=sent_bytes(ns, 4), aud=sent_bytes(ns, 2 * R.HIST_MAX * 4))
    want["kv"][:, slot, :, K.reset_window_rows(g["kv_head"]), :] = 0
    want["dec_h"][slot], want["dec_c"][slot], want["ring"][slot, :R.PRE_CACHE] = 0, 0, 0
    if not c["keep"]:
        want["cc"][:, slot], want["abuf"][slot, 0, :4 * NFFT // 2], want["last"][slot] = 0, 0, 0
    want["ctrl"][slot] = np.array([R.DECCTRL_RESET[f] for f in R.DECCTRL_FIELDS], np.int32).view(np.uint8)
    want["aud"][slot] = 0
    want["boost"][slot] = np.array([1], np.int32).view(np.uint8)
    if c["lm"]:
        want["lm"][slot] = np.array([R.greedy_start(*c["lm"])], np.int32).view(np.uint8)
    with device() as dev:
        h = {k: dev.new(v.nbytes) for k, v in want.items() if (k != "aud" or c["aud"]) and (k != "boost" or c["boost"]) and (k != "lm" or c["lm"])}
        blk = -1
        if c["lm"]:
            greedy = np.zeros(gsize, np.uint8)
            greedy[at_attached:at_attached + 4] = np.array([c["lm"][0]], np.int32).view(np.uint8)
            greedy[at_start:at_start + 4] = np.array([c["lm"][1]], np.int32).view(np.uint8)
            blk = dev.up(greedy)
        a = ints(dev.new(2 * nl * 8), h["kv"], h["cc"], esz, g["kv_head"], nl, slot, ns, ccf, c["keep"], h["abuf"], h["last"], h["ring"], h["dec_h"], h["dec_c"], h["ctrl"],
                 h.get("boost", -1), 1, h.get("lm", -1), blk, c["lm"][2] if c["lm"] else 0, h.get("aud", -1))
        ok(dev, L.front_harness_reset(p(a)))
        ctrl = body(dev, h["ctrl"], np.int32, ns * 12, "ctrl").reshape(ns, 12)
        for k, f in enumerate(R.DECCTRL_FIELDS):
            assert ctrl[slot, k] == R.DECCTRL_RESET[f], f
        for k, hk in h.items():
            same_image(dev, hk, want[k], k)


# ---- the harness refuses what the kernels' indexing does not cover ------------------------------------------------------------------------------------------
def test_harness_refuses_cases_the_kernels_do_not_cover():
    case = mel_case("exact-max_n")
    push = case["pushes"][0]
    with device() as dev:
        L = dev.L
        tabs = up_tables(dev, case["tables"])
        abuf, last, ring = dev.up(case["abuf0"], written=True), dev.up(case["last0"], written=True), dev.new(K.MEL_POOL * MEL_RING * NMEL * 4)
        tab, pcm = dev.new(3 * 40), dev.up(push["pcm"])

        def mel(col=None, value=None, **kw):
            d = push["desc"].copy()
            if col is not None:
                d[0, col] = value
            a = dict(max_frames=push["max_frames"], ring=ring, band=tabs[2])
            a.update(kw)
            args = ints(tab, pcm, 3, a["max_frames"], abuf, last, a["ring"], tabs[0], tabs[1], a["band"], tabs[3], tabs[4], -1, 0, push["max_n"], K.MEL_POOL)
            return L.front_harness_mel(p(args), p(d))
        bad_band = case["tables"][2].copy()
        bad_band[7, 1] = 258
        for rc, why in ((lambda: mel(3, ABUF_CAP - 999), "cnt + n > ABUF_CAP"), (lambda: mel(5, 6, max_frames=6), "samples allow"), (lambda: mel(5, 6), "max_frames"), (lambda: mel(7, 801), "consumed"), (lambda: mel(1, 4), "slot"),
                        (lambda: mel(1, 3), "twice"), (lambda: mel(6, MEL_RING), "mel_wpos"), (lambda: mel(ring=dev.new(MEL_RING * NMEL * 4)), "holds"),
                        (lambda: mel(band=dev.up(bad_band)), "fb_band"), (lambda: mel(0, 2100), "leave the pcm buffer")):
            assert rc() == -1 and why in dev.err(), (why, dev.err())
        same_image(dev, abuf, case["abuf0"], "abuf")          # nothing was launched
        small = dev.new(4096)
        pc = np.array([[0, 0, 64, 0], [64, 32, 64, 16]], np.int64)
        assert L.front_harness_pieces(0, dev.new(256), small, dev.new(4096), -1, p(pc), 2) == -1 and "overlap" in dev.err()
        pc = np.array([[4090, 0, 16, 0]], np.int64)
        assert L.front_harness_pieces(0, dev.new(256), small, dev.new(4096), -1, p(pc), 1) == -1 and "multiples of 4" in dev.err()
        pc = np.array([[4064, 0, 64, 0]], np.int64)
        assert L.front_harness_pieces(0, dev.new(256), small, dev.new(4096), -1, p(pc), 1) == -1 and "leaves its buffer" in dev.err()
        pc = np.array([[0, 4092, 4, 0]], np.int64)          # pack pads the word piece to 16 bytes: 4092 + 16 > 4096
        assert L.front_harness_pieces(1, dev.new(256), small, dev.new(4096), dev.new(256), p(pc), 1) == -1 and "leaves its buffer" in dev.err()
        rows = ints(0, 0)
        assert L.front_harness_conv0(dev.new(256), ring, small, small, small, small, small, 0, 1, 17, 9, 64, 4, p(rows)) == -1 and "W1 != 65" in dev.err()
        a = ints(small, 1, tabs[0], dev.new(R.NBINS * 80 * 4), dev.up(np.zeros((80, 2), np.int32)), tabs[3], tabs[4])
        assert L.front_harness_diar_logmel(p(a), small, small, 1, 1000, 64, 65, 80, 0) == -1 and "t_valid > T_pad" in dev.err()
        assert L.front_harness_diar_logmel(p(a), dev.up(np.array([1500], np.int64)), dev.new(64 * 80 * 4), 1, 1000, 64, 63, 80, 0) == -1 and "leaves the audio buffer" in dev.err()


# ---- every kernel in scope is named by a case -----------------------------------------------------------------------------------------------------------------
def test_every_kernel_in_scope_is_named_by_a_case():
    src = (CSRC / "kernels_front.hip").read_text()
    pat = re.compile(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(k_\w+)\s*\(")
    in_scope = set(pat.findall(src))
    assert len(in_scope) == 15, sorted(in_scope)
    claimed = set(CLAIMED) | {conv0_kernel(b) for b in (0, 1)} | {K.dw_kernel(Hin, B, b) for Hin, Bs in K.DW_CASES.items() for B in Bs for b in (0, 1)}
    assert {n.split("<")[0] for n in claimed} == in_scope
    for name in ("k_sub_conv0_dw", "k_sub_dw", "k_sub_dw_row"):
        assert {n for n in claimed if n.split("<")[0] == name} == {f"{name}<false>", f"{name}<true>"}
        assert f"{name}<true>" in src and f"{name}<false>" in src
    assert len(claimed) == 18
    # the launchers' selection rules, restated from the source text: what K.dw_kernel and K.conv0_fz claim
    assert "if ((long)Hout * B >= 512) {" in src and "const int Hout = Hin / 2 + 1, Wout = Win / 2 + 1;" in src
    assert "const int fz = H2 * B <= 64 ? 11 : (H2 * B <= 512 ? 3 : 1);" in src and "const int H2 = H1 / 2 + 1, W2 = W1 / 2 + 1;" in src
    for Rc, Bs in K.CONV0_B.items():
        assert [K.conv0_fz(K.conv0_dims(Rc)[2], B) for B in Bs] == [11, 3, 3, 1]


def test_report_fractions():
    """prints the largest observed fraction of each bound (pytest -s); asserts nothing beyond what the cases asserted"""
    for kernel in sorted(FRACTIONS):
        print(f"{kernel}: largest |got - ref| / bound = {FRACTIONS[kernel]:.4f}")
