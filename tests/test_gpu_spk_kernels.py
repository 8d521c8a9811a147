"""Every TitaNet-L side-car kernel, alone, against a float64 reference of the operation (tests/spk_ref.py).

tests/helpers/spk_harness.hip makes ONE call of a product launcher -- launch_spk_gemm, launch_spk_tile, launch_spk_front, launch_spk_fc, launch_gather_audio
(kernels_spk.hip) and the eight launch_spk_* of kernels_diar.hip -- on buffers [guard | body | guard] whose every byte that is not an input is the sentinel 0xFFC5
(NaN as bf16 and as f32), and returns every buffer whole.  The buffer plumbing (Dev, GUARD, SENT, check_bounded) is tests/test_gpu_layer_kernels.py's.  bf16 weights
go through the product's launch_pack_weight_bf16, f32 MFMA weights through nasr_eng::pack_f32_mfma: packer and kernel are tested as a pair against the row-major
matrix.  Cases -- operands, expectations, the terms of the bounds -- are numpy only and live in tests/spk_kernel_cases.py, where tests/test_spk_kernel_ref.py checks
them without a GPU; the two modes (exact `==`, bounded against float64) and every bound term are described there.

After every launch: outputs finite where owned; every byte the launch does not own still the sentinel (guards, the loud neighbour segments in front of and behind
the launched ones, padding columns of a_out / stat rows, fc_part when Z = 1, the bytes between gather destinations); every read-only buffer bit for bit as uploaded
(Dev.check_inputs on exit).  Stale rows >= L of Y and of the f32 kernels' inputs alternate between a loud, finite, positive value (row L first: ReLU would
swallow a NaN, and with it a mask that is off by one frame) and the sentinel: the kernels read them and must mask them.

k_spk_gemm's LOOP 0 at K = 256 and 1024 needs NASR_SPK_LOOP=0, which the launcher reads once per process: test_gemm_forced_loop0 runs those cases in one child
process with its own timeout.  No tolerance is measured on a kernel under test; no device libm constant is new (sigmoid, expf, tanhf: profiles/decode_kernels.md;
sqrtf and division are IEEE operations in this build).  Largest observed fractions of the bounds and the mutation table: profiles/spk_kernels.md."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi
from tests import spk_kernel_cases as K
from tests import spk_ref as R
from tests.spk_kernel_cases import SG_ASP, SG_DW, SG_RES, SG_Y, ST_DW, ST_STATS
from tests.spk_ref import T
from tests.test_gpu_layer_kernels import SENT, Dev, check_bounded

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HELPER = ROOT / "tests" / "helpers" / "libspk_harness.so"
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"
FRACTIONS = {}            # kernel -> largest observed |got - ref| / bound
KINDS = ("exact", "bounded")


def _ints(*names):
    return [(n, C.c_int) for n in names]


class SgCase(C.Structure):
    _fields_ = _ints("A", "lda", "W", "S", "N", "K", "mode", "bias", "lens", "dw_w", "dw_k", "a_out", "lda_out", "y_out", "colmean", "y_in", "z", "x_out", "x_in",
                     "bn_s", "bn_b", "pool", "seg0", "S_total")


class StCase(C.Structure):
    _fields_ = _ints("y_in", "z", "lens", "S", "C", "mode", "x_out", "dw_w", "dw_k", "a_out", "lda_out", "mean", "stdv", "stat_ld", "seg0", "S_total")


@lru_cache(maxsize=None)
def harness():
    if not HELPER.exists():
        pytest.fail("tests/helpers/libspk_harness.so not built: __graft_entry__.build() warns when the helper fails to compile (a changed SpkGemmParams, SpkTileParams or "
                    "launcher of kernels_spk.hip / kernels_diar.hip?); these tests do not skip")
    C.CDLL(str(capi.LIB_PATH), mode=C.RTLD_GLOBAL)          # the helper's undefined nasr:: symbols resolve against the product library
    L = C.CDLL(str(HELPER))
    L.spk_harness_error.restype = C.c_char_p
    L.spk_harness_alloc.argtypes = [C.c_longlong, C.c_int]
    L.spk_harness_total_bytes.restype = C.c_longlong
    L.spk_harness_put.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_longlong]
    L.spk_harness_get.argtypes = [C.c_int, C.c_void_p]
    L.spk_harness_gather.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_longlong]
    assert [L.spk_harness_struct_bytes(i) for i in range(3)] == [C.sizeof(SgCase), C.sizeof(StCase), 24]
    assert L.spk_harness_sentinel() == SENT == K.SENT
    assert [L.spk_harness_constant(i) for i in range(9)] == [T, R.TVALID, R.NMEL, SG_DW, SG_Y, SG_RES, SG_ASP, ST_DW, ST_STATS]
    return L


def device():
    return Dev(harness(), "spk_harness")


def ok(dev, rc):
    """a refused case is a failed test; an error of the device itself ends the session: nothing more is started on a GPU that has faulted"""
    if rc != 0 and dev.err().startswith(("hipDeviceSynchronize", "launch:")):
        pytest.exit(f"the device reported an error, no further GPU test is run: {dev.err()}", returncode=3)
    assert rc == 0, dev.err()


def is_sent(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint16) == SENT))


def out_buf(dev, n_elems, itemsize):
    return dev.new(max(n_elems * itemsize, 256))


def flat_out(dev, h, dtype, n, what):
    """the first n elements of an output; everything behind them (and the guards: Dev.get) still the sentinel"""
    b = dev.get(h, dtype)
    assert is_sent(b[n:]), f"{what}: written behind its {n} elements"
    return b[:n]


def seg_out(dev, h, dtype, St, rows, ld, ncols, what):
    """an output [St][rows][ld] of which the launch owns columns 0 .. ncols - 1 of segments 1 .. St - 2: those; everything else must still be the sentinel"""
    a = flat_out(dev, h, dtype, St * rows * ld, what).reshape(St, rows, ld)
    assert is_sent(a[0]) and is_sent(a[-1]), f"{what}: a neighbour segment was written"
    assert is_sent(a[1:-1, :, ncols:]), f"{what}: columns >= {ncols} were written"
    got = a[1:-1, :, :ncols]
    return R.bf16_values(got) if dtype == np.uint16 else got


def compare(kernel, what, got, want, bound):
    assert np.all(np.isfinite(got)), f"{kernel} {what}: not finite where owned"
    if bound is None:
        bad = np.argwhere(got != want.astype(np.float32))
        assert bad.size == 0, f"{kernel} {what}: {len(bad)} elements differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    else:
        ratio = check_bounded(got.astype(np.float64), want, bound, 0.0, f"{kernel} {what}")
        FRACTIONS[kernel] = max(FRACTIONS.get(kernel, 0.0), ratio)


def packed_bf16(dev, W):
    N, Kd = W.shape
    src, dst = dev.up(W), dev.new(N * Kd * 2)
    ok(dev, dev.L.spk_harness_pack_bf16(src, dst, N, Kd))
    dev.frozen[dst] = dev.raw(dst)
    return dst


def packed_f32(dev, W):
    N, Kd = W.shape
    src, dst = dev.up(W), dev.new(N * Kd * 4)
    ok(dev, dev.L.spk_harness_pack_f32(src, dst, N, Kd))
    dev.frozen[dst] = dev.raw(dst)
    return dst


# ---- k_spk_gemm -----------------------------------------------------------------------------------------------------------------------------------
def run_gemm(i, mode, kind, forced0=False):
    c = K.gemm_case(i, mode, kind)
    ins, d, exp = c["ins"], c["dims"], c["exp"]
    St, S, N, Kd = d["St"], d["S"], d["N"], d["K"]
    kernel = K.gemm_kernel(mode, Kd, forced0)
    with device() as dev:
        g = SgCase(*([-1] * 24))
        g.A, g.lda, g.W, g.S, g.N, g.K, g.mode = dev.up(ins["A"]), d["lda"], packed_bf16(dev, ins["W"]), S, N, Kd, mode
        g.bias, g.lens, g.dw_k, g.lda_out, g.seg0, g.S_total = dev.up(ins["bias"]), dev.up(ins["lens"]), d["dw_k"], d["lda_out"], 1, St
        for n in ("dw_w", "y_in", "z", "x_in", "bn_s", "bn_b"):
            if n in ins:
                setattr(g, n, dev.up(ins[n]))
        if d["dw_k"]:
            g.a_out = out_buf(dev, St * T * d["lda_out"], 2)
        if mode == SG_Y:
            g.y_out, g.colmean = out_buf(dev, St * T * N, 4), out_buf(dev, St * N, 4)
        if mode == SG_RES:
            g.x_out = out_buf(dev, St * T * N, 2)
        if mode == SG_ASP:
            g.pool = out_buf(dev, St * 2 * N, 4)
        ok(dev, dev.L.spk_harness_gemm(C.byref(g)))
        shapes = {"a_out": (g.a_out, np.uint16, T, d["lda_out"], N), "y_out": (g.y_out, np.float32, T, N, N), "colmean": (g.colmean, np.float32, 1, N, N),
                  "x_out": (g.x_out, np.uint16, T, N, N), "pool": (g.pool, np.float32, 1, 2 * N, 2 * N)}
        for name, (want, bound) in exp.items():
            h, dtype, rows, ld, ncols = shapes[name]
            got = seg_out(dev, h, dtype, St, rows, ld, ncols, f"{kernel} {name}")
            compare(kernel, name, got.reshape(want.shape), want, bound)
    return kernel


GEMM_RUNS = [(i, mode, kind) for i in range(len(K.GEMM_SHAPES)) for mode in (SG_DW, SG_Y, SG_RES, SG_ASP) for kind in KINDS]


def _gemm_id(r):
    Kd, N, S = K.GEMM_SHAPES[r[0]][:3]
    return f"{K.MODE_NAMES[r[1]]}-K{Kd}-N{N}-S{S}-{r[2]}"


@pytest.mark.parametrize("run", GEMM_RUNS, ids=_gemm_id)
def test_gemm(run):
    run_gemm(*run)


def forced_loop0_main():
    """the body of test_gemm_forced_loop0's child process"""
    assert os.environ.get("NASR_SPK_LOOP") == "0"
    n = 0
    try:
        for i in K.FORCED_LOOP0:
            for mode in (SG_DW, SG_Y, SG_RES, SG_ASP):
                for kind in KINDS:
                    run_gemm(i, mode, kind, forced0=True)
                    n += 1
    except pytest.exit.Exception as exc:          # ok(): the device reported an error
        print(exc, file=sys.stderr)
        sys.exit(3)
    print(f"forced LOOP 0: {n} launches ok")


def test_gemm_forced_loop0():
    """LOOP 0 at K = 256 and K = 1024, all four epilogues, both modes: one fresh process (the launcher reads NASR_SPK_LOOP once)"""
    env = dict(os.environ, NASR_SPK_LOOP="0")
    code = "import tests.conftest; from tests.test_gpu_spk_kernels import forced_loop0_main; forced_loop0_main()"
    try:
        r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        pytest.exit("the forced-LOOP-0 child process hung on the GPU, no further GPU test is run", returncode=3)
    if r.returncode not in (0, 1):          # 3: the child's own device error; negative / 134 / 139: abort or fault.  1 is a failed assertion
        pytest.exit(f"the forced-LOOP-0 child process ended with {r.returncode}, no further GPU test is run: {r.stderr[-1500:]}", returncode=3)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "forced LOOP 0: 16 launches ok" in r.stdout


def test_gemm_launcher_takes_loop1_where_the_cases_claim_it():
    """the claim of gemm_kernel() restated from launch_spk_gemm's source: the register-ring loop where K / 32 is a multiple of 8 and NASR_SPK_LOOP is not 0"""
    src = (CSRC / "kernels_spk.hip").read_text()
    assert "const bool regs = !force0 && (p.K / 32) % 8 == 0;" in src and 'getenv("NASR_SPK_LOOP")' in src
    assert os.environ.get("NASR_SPK_LOOP", "1")[:1] != "0", "this module's cases assume the default loop choice"


# ---- k_spk_tile -----------------------------------------------------------------------------------------------------------------------------------
def tile_kernel(mode):
    return f"k_spk_tile<{'ST_DW' if mode == ST_DW else 'ST_STATS'}>"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", range(len(K.TILE_CASES)))
def test_tile(i, kind):
    c = K.tile_case(i, kind)
    ins, d, exp = c["ins"], c["dims"], c["exp"]
    St, S, Cc, mode = d["St"], d["S"], d["C"], d["mode"]
    kernel = tile_kernel(mode)
    with device() as dev:
        g = StCase(*([-1] * 16))
        g.y_in, g.z, g.lens, g.S, g.C, g.mode, g.seg0, g.S_total = dev.up(ins["y_in"]), dev.up(ins["z"]), dev.up(ins["lens"]), S, Cc, mode, 1, St
        g.x_out = out_buf(dev, St * T * Cc, 2)
        g.dw_k, g.lda_out, g.stat_ld = d["dw_k"], d["lda_out"], d["stat_ld"]
        if mode == ST_DW:
            g.dw_w, g.a_out = dev.up(ins["dw_w"]), out_buf(dev, St * T * d["lda_out"], 2)
        elif d["stat_ld"] == 2 * Cc:
            g.mean = g.stdv = out_buf(dev, St * 2 * Cc, 4)          # the halves of one [S][2 C] buffer, as the product's pooling input
        else:
            g.mean, g.stdv = out_buf(dev, St * Cc, 4), out_buf(dev, St * Cc, 4)
        ok(dev, dev.L.spk_harness_tile(C.byref(g)))
        compare(kernel, "x_out", seg_out(dev, g.x_out, np.uint16, St, T, Cc, Cc, "x_out"), *exp["x_out"])
        if mode == ST_DW:
            compare(kernel, "a_out", seg_out(dev, g.a_out, np.uint16, St, T, d["lda_out"], Cc, "a_out"), *exp["a_out"])
        elif d["stat_ld"] == 2 * Cc:
            both = seg_out(dev, g.mean, np.float32, St, 1, 2 * Cc, 2 * Cc, "mean | std")[:, 0]
            compare(kernel, "mean", both[:, :Cc], *exp["mean"])
            compare(kernel, "stdv", both[:, Cc:], *exp["stdv"])
        else:
            compare(kernel, "mean", seg_out(dev, g.mean, np.float32, St, 1, Cc, Cc, "mean")[:, 0], *exp["mean"])
            compare(kernel, "stdv", seg_out(dev, g.stdv, np.float32, St, 1, Cc, Cc, "stdv")[:, 0], *exp["stdv"])


@pytest.mark.parametrize("k", [3, 7, 11, 15])
def test_fused_depthwise_has_the_bits_of_the_f32_kernel(k):
    """kernels_spk.hip: "k_spk_depthwise's order (same bits from the same f32 inputs)".  Gate exactly 1, y >= 0 and bf16-representable, random f32 taps: a_out of
    k_spk_tile<ST_DW> must be, bit for bit, the bf16 rounding of k_spk_depthwise's f32 output on the same y."""
    rng = K.rng_of("identity", k)
    S, Cc = 3, 128
    ll = np.array([10, 81, 150], np.int32)
    y = K.stale(R.bf16_round(np.abs(rng.standard_normal((S, T, Cc)))), ll)
    taps = rng.standard_normal((k, Cc)).astype(np.float32)
    with device() as dev:
        hy, hl, hw = dev.up(y.reshape(S * T, Cc)), dev.up(ll), dev.up(taps)
        g = StCase(*([-1] * 16))
        g.y_in, g.z, g.lens, g.S, g.C, g.mode, g.seg0, g.S_total = hy, dev.up(np.full((S, Cc), 40.0, np.float32)), hl, S, Cc, ST_DW, 0, S
        g.x_out, g.dw_w, g.dw_k, g.a_out, g.lda_out = out_buf(dev, S * T * Cc, 2), hw, k, out_buf(dev, S * T * Cc, 2), Cc
        ok(dev, dev.L.spk_harness_tile(C.byref(g)))
        f32_out = out_buf(dev, S * T * Cc, 4)
        ok(dev, dev.L.spk_harness_depthwise(hy, Cc, hw, k, Cc, Cc, hl, f32_out, S))
        fused = flat_out(dev, g.a_out, np.uint16, S * T * Cc, "a_out")
        plain = flat_out(dev, f32_out, np.float32, S * T * Cc, "k_spk_depthwise")
        assert np.all(np.isfinite(plain)) and np.any(plain != 0)
        assert np.array_equal(fused, R.bf16_bits(plain))
        assert np.array_equal(flat_out(dev, g.x_out, np.uint16, S * T * Cc, "x_out"), R.bf16_bits(K.mask_rows(y.reshape(S, T, Cc), ll, 0.0)).reshape(-1))


# ---- k_spk_front ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(K.FRONT_CASES)))
def test_front(i):
    c = K.front_case(i)
    d = c["dims"]
    S, ld = d["S"], d["lda_out"]
    with device() as dev:
        out = out_buf(dev, S * T * ld, 2)
        ok(dev, dev.L.spk_harness_front(dev.up(c["mel"]), d["cpitch"], dev.up(c["taps"]), dev.up(c["lens"]), out, ld, S))
        a = flat_out(dev, out, np.uint16, S * T * ld, "a_out").reshape(S, T, ld)
        assert is_sent(a[:, :, 128:]), "k_spk_front wrote columns >= 128"
        got, want = R.bf16_values(a[:, :, :128]), R.bf16_values(c["bits"])
        compare("k_spk_front", "a_out", got, want, None)
        assert np.all(got[:, :, 80:] == 0) and all(np.all(got[s, L:] == 0) for s, L in enumerate(c["lens"]))


# ---- k_spk_fc, k_spk_fc_reduce ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("site", K.FC_SITES + [(64, 16)], ids=lambda s: f"K{s[0]}-N{s[1]}")
def test_fc(site, kind):
    Kd, N = site
    W, b = K.fc_weights(Kd, N, kind)
    zs = set()
    with device() as dev:
        hw, hb = packed_f32(dev, W), dev.up(b)
        for j, M in enumerate(K.FC_M if Kd > 64 else (5,)):
            relu, ldx = (j + Kd // 64) % 2, Kd + (8 if M == 5 else 0)
            c = K.fc_case(Kd, N, M, relu, ldx, kind)
            Z = dev.L.spk_harness_fc_slices(M, Kd, N)
            assert Z == K.fc_slices(M, Kd, N)
            zs.add(Z)
            out, part = out_buf(dev, M * N, 4), out_buf(dev, Z * M * N, 4)
            ok(dev, dev.L.spk_harness_fc(dev.up(c["x"]), ldx, hw, hb, out, part, M, Kd, N, relu))
            kernel = "k_spk_fc" if Z == 1 else "k_spk_fc_reduce"
            compare(kernel, f"out M={M} relu={relu}", flat_out(dev, out, np.float32, M * N, "out").reshape(M, N), c["ref"], c["bound"])
            if Z == 1:
                assert is_sent(dev.get(part, np.float32)), "fc_part was written although Z = 1"
            else:
                assert np.all(np.isfinite(flat_out(dev, part, np.float32, Z * M * N, "part")))
    assert zs == {K.fc_slices(M, Kd, N) for M in (K.FC_M if Kd > 64 else (5,))}


# ---- k_gather_audio -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(K.GATHER_CASES)), ids=lambda i: K.GATHER_CASES[i][0])
def test_gather(i):
    c = K.gather_case(i)
    B = len(c["desc"])
    with device() as dev:
        dst, tab = out_buf(dev, c["want"].size, 2), dev.new(B * 24)
        desc = np.ascontiguousarray(c["desc"], np.int64)
        ok(dev, dev.L.spk_harness_gather(dev.up(c["src"]), dst, tab, desc.ctypes.data, B, c["max_bytes"]))
        got = dev.get(dst, np.uint16)
        assert np.array_equal(got[:c["want"].size], c["want"]) and is_sent(got[c["want"].size:])


# ---- the f32 engine's kernels (kernels_diar.hip) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS + ("chain",))
@pytest.mark.parametrize("i", range(len(K.DEPTHWISE_CASES)))
def test_depthwise_f32(i, kind):
    c = K.depthwise_case(i, kind)
    d = c["dims"]
    n = d["S"] * T * d["Cpad"]
    with device() as dev:
        out = out_buf(dev, n, 4)
        ok(dev, dev.L.spk_harness_depthwise(dev.up(c["x"]), d["pitch"], dev.up(c["w"]), d["k"], d["C"], d["Cpad"], dev.up(c["lens"]), out, d["S"]))
        got = flat_out(dev, out, np.float32, n, "a_out").reshape(c["ref"].shape)
        compare("k_spk_depthwise", "a_out", got, c["ref"], c["bound"])
        if kind == "chain":
            compare("k_spk_depthwise", "a_out (float32 restatement: tap 0's product, then one fma per tap, i ascending)", got, c["f32"], None)
        assert np.all(got[:, :, d["C"]:] == 0)


@pytest.mark.parametrize("i", range(6))
def test_colmean_f32(i):
    c = K.colmean_case(i)
    d = c["dims"]
    with device() as dev:
        out = out_buf(dev, d["S"] * d["C"], 4)
        ok(dev, dev.L.spk_harness_colmean(dev.up(c["y"]), d["C"], dev.up(c["lens"]), out, d["S"]))
        got = flat_out(dev, out, np.float32, d["S"] * d["C"], "mean").reshape(d["S"], d["C"])
        compare("k_spk_colmean", "mean (float32 restatement)", got, c["f32"], None)
        compare("k_spk_colmean", "mean", got, c["ref"], c["bound"])


@pytest.mark.parametrize("i", range(4))
def test_combine_f32(i):
    c = K.combine_case(i)
    d = c["dims"]
    n = d["S"] * T * d["C"]
    with device() as dev:
        out = out_buf(dev, n, 4)
        hr = -1 if c["r"] is None else dev.up(c["r"])
        ok(dev, dev.L.spk_harness_combine(dev.up(c["y"]), dev.up(c["z"]), hr, d["C"], dev.up(c["lens"]), out, d["S"]))
        compare("k_spk_combine", "out", flat_out(dev, out, np.float32, n, "out").reshape(c["ref"].shape), c["ref"], c["bound"])


@pytest.mark.parametrize("i", range(2))
def test_mask_cvt_f32(i):
    c = K.mask_cvt_case(i)
    d = c["dims"]
    n = d["S"] * T * d["C"]
    with device() as dev:
        out = out_buf(dev, n, 4)
        ok(dev, dev.L.spk_harness_mask_cvt(dev.up(c["x"]), d["C"], dev.up(c["lens"]), out, d["S"]))
        compare("k_spk_mask_cvt", "a_out", flat_out(dev, out, np.float32, n, "a_out").reshape(c["want"].shape), c["want"], None)


@pytest.mark.parametrize("i", range(3))
def test_stats_f32(i):
    c = K.stats_case(i)
    d = c["dims"]
    n = d["S"] * d["C"]
    with device() as dev:
        hm, hs = out_buf(dev, n, 4), out_buf(dev, n, 4)
        ok(dev, dev.L.spk_harness_stats(dev.up(c["x"]), d["C"], dev.up(c["lens"]), hm, hs, d["S"]))
        compare("k_spk_stats", "mean", flat_out(dev, hm, np.float32, n, "mean").reshape(d["S"], d["C"]), *c["mean"])
        compare("k_spk_stats", "stdv", flat_out(dev, hs, np.float32, n, "stdv").reshape(d["S"], d["C"]), *c["stdv"])


@pytest.mark.parametrize("i", range(4))
def test_att_const_f32(i):
    c = K.att_const_case(i)
    d = c["dims"]
    n = d["S"] * d["A"]
    with device() as dev:
        out = out_buf(dev, n, 4)
        ok(dev, dev.L.spk_harness_att_const(dev.up(c["mean"]), dev.up(c["stdv"]), dev.up(c["w1"]), dev.up(c["b1"]), out, d["C"], d["A"], d["S"]))
        compare("k_spk_att_const", "c", flat_out(dev, out, np.float32, n, "c").reshape(d["S"], d["A"]), c["ref"], c["bound"])


@pytest.mark.parametrize("i", range(4))
def test_att_post_f32(i):
    c = K.att_post_case(i)
    d = c["dims"]
    n = d["S"] * T * d["A"]
    assert c["pre_max"] < 12          # the range tanhf was measured on
    with device() as dev:
        out = out_buf(dev, n, 2 if d["bf16"] else 4)
        ok(dev, dev.L.spk_harness_att_post(dev.up(c["g"]), dev.up(c["c"]), dev.up(c["sc"]), dev.up(c["bi"]), out, d["bf16"], d["A"], d["S"]))
        got = flat_out(dev, out, np.uint16 if d["bf16"] else np.float32, n, "a_out")
        compare("k_spk_att_post", "a_out", (R.bf16_values(got) if d["bf16"] else got).reshape(c["ref"].shape), c["ref"], c["bound"])


@pytest.mark.parametrize("i", range(3))
def test_asp_f32(i):
    c = K.asp_case(i)
    d = c["dims"]
    n = d["S"] * 2 * d["C"]
    with device() as dev:
        out = out_buf(dev, n, 4)
        ok(dev, dev.L.spk_harness_asp(dev.up(c["x"]), dev.up(c["logits"]), d["C"], dev.up(c["lens"]), dev.up(c["sc"]), dev.up(c["bi"]), out, d["S"]))
        compare("k_spk_asp", "pool", flat_out(dev, out, np.float32, n, "pool").reshape(c["ref"].shape), c["ref"], c["bound"])


# ---- the harness refuses what the kernels' indexing does not cover ------------------------------------------------------------------------------------
def test_harness_refuses_cases_the_kernels_do_not_cover():
    c = K.gemm_case(0, SG_DW, "exact")
    ins, d = c["ins"], c["dims"]
    with device() as dev:
        def case(**kw):
            g = SgCase(*([-1] * 24))
            g.A, g.lda, g.W, g.S, g.N, g.K, g.mode = dev.up(ins["A"]), d["lda"], packed_bf16(dev, ins["W"]), d["S"], d["N"], d["K"], SG_DW
            g.bias, g.lens, g.dw_w, g.dw_k, g.lda_out, g.seg0, g.S_total = dev.up(ins["bias"]), dev.up(ins["lens"]), dev.up(ins["dw_w"]), 3, 128, 1, d["St"]
            g.a_out = out_buf(dev, d["St"] * T * 128, 2)
            for k, v in kw.items():
                setattr(g, k, v)
            return g
        bad_lens = ins["lens"].copy()
        bad_lens[1] = 0
        for g, whys in ((case(lens=dev.up(bad_lens)), ("lens",)), (case(K=48), ("holds", "spk_gemm_check")), (case(N=192), ("holds", "spk_gemm_check")),
                        (case(dw_k=1), ("spk_gemm_check",)), (case(S_total=d["St"] + 1), ("holds", "lens")), (case(lda_out=256), ("holds",)), (case(a_out=-1), ("holds",))):
            assert dev.L.spk_harness_gemm(C.byref(g)) == -1 and any(w in dev.err() for w in whys), (whys, dev.err())
        long_lens = np.array([161], np.int32)
        assert dev.L.spk_harness_colmean(dev.new(T * 64 * 4), 64, dev.up(long_lens), dev.new(256), 1) == -1 and "lens" in dev.err()
        assert dev.L.spk_harness_fc(dev.new(64 * 4), 64, dev.new(64 * 16 * 4), dev.new(64), dev.new(64), -1, 1, 96, 16, 0) == -1
        assert dev.L.spk_harness_att_post(dev.new(256), dev.new(256), dev.new(256), dev.new(256), dev.new(256), 0, 129, 1) == -1


# ---- every kernel in scope is named by a case ---------------------------------------------------------------------------------------------------
def claimed_kernels():
    names = {K.gemm_kernel(mode, K.GEMM_SHAPES[i][0]) for i, mode, _ in GEMM_RUNS} | {K.gemm_kernel(mode, K.GEMM_SHAPES[i][0], True) for i in K.FORCED_LOOP0 for mode in range(4)}
    names |= {tile_kernel(m) for _, _, m, _ in K.TILE_CASES}
    names |= {"k_spk_front", "k_spk_fc", "k_spk_fc_reduce", "k_gather_audio", "k_spk_depthwise", "k_spk_mask_cvt", "k_spk_colmean", "k_spk_combine", "k_spk_stats",
              "k_spk_att_const", "k_spk_att_post", "k_spk_asp"}
    return names


def test_every_kernel_in_scope_is_named_by_a_case():
    pat = re.compile(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(k_\w+)\s*\(")
    spk = (CSRC / "kernels_spk.hip").read_text()
    diar = (CSRC / "kernels_diar.hip").read_text()
    banner = "// TitaNet-L speaker embedding"
    assert diar.count(banner) == 1
    diar = diar[diar.index(banner):]                                # the TitaNet part; MarbleNet above the banner is out of scope
    in_scope = set(pat.findall(spk)) | set(pat.findall(diar))
    assert len(in_scope) == 14 and not any(n.startswith("k_vad") for n in in_scope), sorted(in_scope)
    claimed = claimed_kernels()
    assert {n.split("<")[0] for n in claimed} == in_scope
    assert {n for n in claimed if n.startswith("k_spk_gemm")} == {f"k_spk_gemm<{m},{lp}>" for m in K.MODE_NAMES.values() for lp in (0, 1)}
    assert {n for n in claimed if n.startswith("k_spk_tile")} == {"k_spk_tile<ST_DW>", "k_spk_tile<ST_STATS>"}
    assert any(K.fc_slices(M, Kd, N) > 1 for Kd, N in K.FC_SITES for M in K.FC_M) and any(K.fc_slices(M, Kd, N) == 1 for Kd, N in K.FC_SITES for M in K.FC_M)


def test_report_fractions():
    """prints the largest observed fraction of each bound (pytest -s); asserts nothing beyond what the cases asserted"""
    for kernel in sorted(FRACTIONS):
        print(f"{kernel}: largest |got - ref| / bound = {FRACTIONS[kernel]:.4f}")
