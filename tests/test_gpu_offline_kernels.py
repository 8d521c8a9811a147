"""Every kernel of kernels_offline.hip, alone, against a float64 reference of the operation (tests/offline_kernel_ref.py, tests/layer_ref.py).

tests/helpers/offline_harness.hip runs ONE launch through the product's launcher (launch_off_attention, launch_off_dwconv, launch_off_conv0_dw,
launch_off_window, launch_off_dec_reset) on buffers [guard | body | guard] whose every byte that is not an input is the sentinel 0xFFC5 (NaN as bf16
and, doubled, as f32), and returns every buffer whole.  The buffer plumbing (Dev, check_inputs, the sentinel checks) is tests/test_gpu_layer_kernels.py's.
Each case names the kernel its launcher takes (`attention_kernel`, `conv0_kernel`: act_bf16 selects); test_every_offline_kernel_is_reached compares the
names with the __global__ functions of the source.  The cases themselves -- layouts, operands, expectations, references, the terms of the bounds -- are
numpy only and live in tests/offline_kernel_cases.py, where tests/test_offline_kernel_ref.py checks them without a GPU.

Attention layout.  A packed batch of 2 to 4 utterances, qkv [M + SLACK][3072] in the act dtype, rows past M the sentinel (for bf16 the f32 image, sentinel
rows included, is converted by the product's launch_f32_to_bf16, whose NaN rule (u >> 16) | 0x40 keeps 0xFFC5: asserted), the position table whole
([4095][1024]).  The work items are the driver's (nasr_offline.hip: one item (off, T, q0, 0) per off_attn_qb(act) query rows, qb asked from the library).

Selector mode (`==`, both kernels).  q = 0, bias_u = 32 e0 + 32 e2, bias_v = 32 e1 + 32 e3 in every head.  A rank rho = a + 256 b (a < 256, b < 16) is
stored as 64 a in one dimension and 16384 b in the other (both exact in bf16, every f32 sum exact): content run K[j][h, 0], K[j][h, 2] with Pos = 0 and
rho a per-head permutation of the packed rows; position run Pos[r][h, 1], Pos[r][h, 3] with K = 0 and rho a per-head permutation of the 4095 table
rows.  A raw score is 2048 rho: distinct ranks are >= 181 apart after the scale, exp(-181) = 0 in f32, so every softmax is one-hot (alpha is 0 or 1,
l_run = 1) and the context row equals, bit for bit, the V row (small integers naming (utterance, frame, column)) of the highest-ranked key the query may
attend: j < T of its own utterance in the content run, argmax_j rho(j - i + 2047) in the position run.  The expectation is computed from that
definition.  Every utterance of a batch is under test and the ranks of its neighbours' rows compete with its own, so a key read across `off` or
`off + T` wins somewhere.  Besides random seeds, targeted runs put the top ranks on the first row of every utterance (key 0; the next utterance's first
row off + T outranks it and must not win), on the last row of every utterance (key T - 1; row off - 1 outranks it), on key 63 and on key 64 (the last
key of a 64-key block: alpha = 1 in the blocks behind it; the first key of the next: alpha = 0 there), and on the table rows of rel = +(T - 1), 0 and
-(T - 1) of every T of the batch -- rows 0 and 4094 at T = 2048.  The rows 2048 - T (2046 + T) are ranked longest T first: an utterance reaches those of
every T' <= T, so its own is the highest it reaches, and its query T - 1 selects key 0 (its query 0 key T - 1) whatever the other utterances are.

Bounded mode.  The utterance under test lies between two others whose q, K and V are finite and loud (|x| = 64); the table rows no query of T frames
may address are loud too; only the items of the utterance under test are launched, so the neighbours' context rows must stay the sentinel.  Operands
random, rounded to the operand type, per element against offline_kernel_ref.attention with the bound tests/test_gpu_layer_kernels.py states:
  |got - ref| <= (2 Delta_i + omega + EXPF_REL) sum_j w_j |V_jd| + o |ref|, Delta_i = max_j scale (rho + 256 2^-24) (|q + u| . |K_j| + |q + v| . |Pos_r|),
  rho = 2^-9 for k_off_attn_bf16 (q + bias rounded to bf16), 0 for k_off_attn_f32; omega = 2^-8 (the weights rounded to bf16) or 2^-23 T; o = 2^-8 or
  2^-23.  Delta_i <= 0.05 is asserted.  rho = 2^-9 is the allowance stated for the streaming kernels and is kept; it is not the worst case of one
  rounding to bf16 (2^-8 relative just above a power of two), which the 128 roundings of a score do not reach together: the kernel sits at 0.14 of the bound.
A uniform softmax hides an index error, so the operands are not white noise: q, K and Pos carry one direction per head (content on the even
dimensions, position on the odd ones: |a| . |b| = |a . b| there, which is what lets a score be large while Delta_i stays small), a few keys per
utterance are salient and the position term moves a score by a few units.  `bounded_case` asserts that the reference's largest weight per row has a
median >= 0.2 (tests/test_offline_kernel_ref.py runs that on the CPU for every shape).
Shapes: T in {1, 2, 15, 16, 17, 63, 64, 65, 129, 200} for both kernels (every remainder of 64 query rows | 16 per wave | 64 keys), and one utterance
of T = 2048 alone -- the only T at which rbase + 79 passes row 4094 and at which table rows 0 and 4094 are read: selector mode on all rows, bounded mode
on the first and the last query block plus 64 random rows, both kernels.

k_off_dwconv: taps ks u sum_k |z w| through layer_ref.layer_norm_bound, 1.1 x through SiLU, + EXPF_REL |ref|, + 2^-8 |ref| for bf16 (k_dwconv's bound), with
a loud utterance in front of every utterance under test; tpos as the driver builds it.  k_off_conv0_dw: |got - ref| <= sum |w2| e0 + g (sum |w2| a0 + |b2|),
e0 = g (sum |w0 x| + |b0|), g = 10 u / (1 - 10 u) (nine products and a bias each; ReLU is 1-Lipschitz), + 2^-8 |ref| for bf16; the f32 form is also bit for
bit a float32 restatement in the documented order (separate multiply and add: the file is built with -ffp-contract=off).  k_off_window: an exact copy.
k_off_dec_reset: the documented values.  EXPF_REL is tests/test_gpu_gemm_kernels.py's constant.  No tolerance here is measured on a kernel.
After every launch: outputs finite, every byte the launch does not own still the sentinel (context rows outside [off, off + T) of the launched
utterances, rows >= M, output rows past an utterance's H2, windows rows >= n_b, slot B, guards), and every read-only buffer bit for bit as uploaded
(Dev.check_inputs)."""
from __future__ import annotations

import ctypes as C
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi
from tests import layer_ref as LR
from tests import offline_kernel_ref as OR
from tests.test_gpu_gemm_kernels import EXPF_REL
from tests.offline_kernel_cases import (BOUNDED_T, SEEDS, SELECTOR_BATCHES, Packed, SubSetup, attention_bound, bounded_case, conv_front_f32, selector_case,
                                        selector_runs, sub_h2)
from tests.test_gpu_layer_kernels import GUARD, SENT, TINY, U24, Dev, act_bits, act_values, check_bounded, rng_of

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HELPER = ROOT / "tests" / "helpers" / "liboffline_harness.so"
SOURCE = ROOT / "nemotron-asr.cpp_amd" / "csrc" / "kernels_offline.hip"
D, NH, DH, MAX_T, NREL, QKV_LD, MAX_KS, SUBC, NMEL, JNT, HID, BLANK, DEC_WIN = 1024, 8, 128, 2048, 4095, 3072, 32, 256, 128, 640, 640, 1024, 256
SLACK = 5                 # sentinel rows behind the M packed rows of every row buffer (the engine's workspaces are longer than a batch)


# ---- the launchers' rules, restated (kernels_offline.hip: act_bf16 / out_bf16 selects) ----------------------------------------------------------
def attention_kernel(bf16):
    return "k_off_attn_bf16" if bf16 else "k_off_attn_f32"


def conv0_kernel(bf16):
    return f"k_off_conv0_dw<{'true' if bf16 else 'false'}>"


def takes(name, want):
    assert name == want, f"the launcher's rule takes {name}, the case is there for {want}"


# ---- the harness -----------------------------------------------------------------------------------------------------------------------------
def _ints(*names):
    return [(n, C.c_int) for n in names]


class AttnCase(C.Structure):
    _fields_ = _ints("qkv", "pos", "bias_u", "bias_v", "items", "n_items", "ctx", "M", "act_bf16")


class ConvCase(C.Structure):
    _fields_ = _ints("glu", "tpos", "M", "dw", "ks", "ln_w", "ln_b", "out", "act_bf16")


class SubCase(C.Structure):
    _fields_ = _ints("desc", "B", "max_h2", "mel", "mel_rows", "w0t", "b0", "w2t", "b2", "out", "out_rows", "out_bf16")


class WinCase(C.Structure):
    _fields_ = _ints("encproj", "rows", "win", "B", "W", "out")


class ResetCase(C.Structure):
    _fields_ = _ints("B", "h", "c", "ctrl")


DEC_CTRL = ("t", "n_frames", "symbols", "prev_token", "cur", "n_tok", "active", "iterations", "row", "dirty", "frame0", "frame_next")


@lru_cache(maxsize=None)
def harness():
    if not HELPER.exists():
        pytest.fail("tests/helpers/liboffline_harness.so not built: __graft_entry__.build() warns when the helper fails to compile (a changed launcher of "
                    "kernels_offline.hip?); these tests do not skip")
    C.CDLL(str(capi.LIB_PATH), mode=C.RTLD_GLOBAL)          # the helper's undefined nasr:: symbols resolve against the product library
    L = C.CDLL(str(HELPER))
    L.offline_harness_error.restype = C.c_char_p
    L.offline_harness_alloc.argtypes = [C.c_longlong, C.c_int]
    L.offline_harness_total_bytes.restype = C.c_longlong
    L.offline_harness_put.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_longlong]
    L.offline_harness_get.argtypes = [C.c_int, C.c_void_p]
    L.offline_harness_to_bf16.argtypes = [C.c_int, C.c_int, C.c_longlong]
    for i, s in enumerate((AttnCase, ConvCase, SubCase, WinCase, ResetCase)):
        assert L.offline_harness_struct_bytes(i) == C.sizeof(s), s
    assert [L.offline_harness_struct_bytes(i) for i in (5, 6, 7)] == [16, 4 * len(DEC_CTRL), 16]          # OffSubDesc, DecCtrl, int4
    assert L.offline_harness_sentinel() == SENT
    assert [L.offline_harness_constant(i) for i in range(13)] == [D, NH, DH, MAX_T, NREL, QKV_LD, MAX_KS, SUBC, NMEL, JNT, HID, BLANK, DEC_WIN]
    return L


def dev():
    return Dev(harness(), "offline_harness")


def attn_qb(bf16):
    return harness().offline_harness_attn_qb(int(bf16))


def owned_rows_only(bits, owned, what):
    """bits [rows][row elements] of a downloaded body; owned [rows] bool: every other row is still the sentinel"""
    rest = np.ascontiguousarray(bits[~owned]).view(np.uint16).reshape(int((~owned).sum()), -1)
    bad = np.flatnonzero(~owned)[(rest != SENT).any(-1)]
    assert bad.size == 0, f"{what}: {bad.size} rows the launch does not own were written, the first is row {bad[0]}"


# ==== attention =================================================================================================================================
def run_attention(dv: Dev, lay: Packed, bf16, qkv, pos, bu, bv, only=None):
    """one launch -> (context rows [M][1024] as f32 values, finite where launched; NaN elsewhere); ownership checked"""
    esz, M = (2 if bf16 else 4), lay.M
    items = lay.items(attn_qb(bf16), only)
    c = AttnCase()
    if bf16:                                                                 # converted by the product's launch_f32_to_bf16: a NaN becomes (u >> 16) | 0x40, so the slack rows stay 0xFFC5
        c.qkv = dv.bf16_of(qkv, SLACK * QKV_LD * 4)
        assert np.all(dv.frozen[c.qkv][-(GUARD // 2 + SLACK * QKV_LD):] == SENT), "the slack rows of the converted qkv are not the sentinel"
    else:
        c.qkv = dv.up(act_bits(qkv, False), SLACK * QKV_LD * 4)
    c.pos = dv.up(act_bits(pos, bf16))
    c.bias_u, c.bias_v, c.items, c.n_items = dv.up(bu), dv.up(bv), dv.up(items), len(items)
    c.ctx, c.M, c.act_bf16 = dv.new((M + SLACK) * D * esz), M, int(bf16)
    assert dv.L.offline_harness_attention(C.byref(c)) == 0, dv.err()
    out = dv.get(c.ctx, np.uint16 if bf16 else np.uint32)
    out = out[:(len(out) // D) * D].reshape(-1, D)
    owned = np.zeros(len(out), bool)
    owned[:M] = lay.rows_of(only)
    owned_rows_only(out, owned, "ctx")
    got = np.full((M, D), np.nan, np.float32)
    got[owned[:M]] = act_values(out[:M][owned[:M]].reshape(-1), bf16).reshape(-1, D)
    assert np.all(np.isfinite(got[owned[:M]])), "a context element is not finite (unwritten, or poison reached it)"
    return got


ATTN_KERNELS = [("k_off_attn_bf16", True), ("k_off_attn_f32", False)]
SELECTOR_CASES = [(kernel, bf16, Ts) for kernel, bf16 in ATTN_KERNELS for Ts in SELECTOR_BATCHES]
CONV0_KERNELS = [("k_off_conv0_dw<false>", False), ("k_off_conv0_dw<true>", True)]


def _check_selector(bf16, Ts, seeds):
    lay = Packed(Ts)
    for run, seed, target in selector_runs(seeds):
        qkv, pos, bu, bv, exp = selector_case(lay, run, seed, target)
        with dev() as dv:
            got = run_attention(dv, lay, bf16, qkv, pos, bu, bv)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (f"{attention_kernel(bf16)} T {Ts} {run} seed {seed} target {target}: {len(bad)} elements differ, first (row, column) {bad[0]}: "
                               f"got {got[tuple(bad[0])]}, want {exp[tuple(bad[0])]}")


@pytest.mark.parametrize("kernel,bf16,Ts", SELECTOR_CASES, ids=lambda v: str(v))
def test_attention_selector(kernel, bf16, Ts):
    takes(attention_kernel(bf16), kernel)
    _check_selector(bf16, Ts, SEEDS)


@pytest.mark.parametrize("kernel,bf16", ATTN_KERNELS, ids=lambda v: str(v))
def test_attention_selector_2048(kernel, bf16):
    """T = 2048 alone, every row: band row 79 passes the table's end (clamped), table rows 0 and 4094 are read (rel_plus / rel_minus put the top rank there)"""
    takes(attention_kernel(bf16), kernel)
    _check_selector(bf16, (MAX_T,), (0,))


def _check_bounded(T, bf16):
    lay, k, qkv, pos, bu, bv, rows, ref, delta, wabsv = bounded_case(T, bf16)
    bound = attention_bound(ref, delta, wabsv, T, bf16, EXPF_REL)
    with dev() as dv:
        got = run_attention(dv, lay, bf16, qkv, pos, bu, bv, only=[k])
    got = got[lay.offs[k] + rows]
    err = np.abs(got - ref)
    print(f"{attention_kernel(bf16)} T {T}: worst |got - ref| / bound = {(err / bound).max():.3f}")
    assert np.all(err <= bound), f"worst ratio {(err / bound).max()} at {np.unravel_index(np.argmax(err / bound), err.shape)}"


@pytest.mark.parametrize("T", BOUNDED_T + (MAX_T,))
@pytest.mark.parametrize("kernel,bf16", ATTN_KERNELS, ids=lambda v: str(v))
def test_attention_bounded(kernel, bf16, T):
    takes(attention_kernel(bf16), kernel)
    _check_bounded(T, bf16)


# ==== depthwise conv from a zero history ===========================================================================================================
DWCONV_KS = (2, 9, MAX_KS)


def dwconv_lengths(ks):
    return sorted({1, 2, ks - 1, ks, ks + 1, 20} - {0})


class OffConvSetup:
    """[loud | T_0 | loud | T_1 | ...]: a loud utterance of ks frames in front of every utterance under test"""

    def __init__(self, ks, seed=0, scale=1.0):
        rng = rng_of("off-conv", ks, seed)
        self.ks, self.tested = ks, []
        Ts = []
        for T in dwconv_lengths(ks):
            Ts += [ks, T]
            self.tested.append(len(Ts) - 1)
        self.lay = lay = Packed(Ts)
        self.glu = (64.0 * rng.choice([-1.0, 1.0], (lay.M, D))).astype(np.float32)
        for k in self.tested:
            self.glu[lay.offs[k]:lay.offs[k] + lay.Ts[k]] = (scale * rng.standard_normal((lay.Ts[k], D))).astype(np.float32)
        self.dw = (rng.standard_normal((ks, D)) / np.sqrt(ks)).astype(np.float32)
        self.ln_w, self.ln_b = (1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32), (0.2 * rng.standard_normal(D)).astype(np.float32)

    def reference(self):
        """-> per utterance under test (rows, ref [T][1024], bound before the output rounding)"""
        out = []
        for k in self.tested:
            off, T = self.lay.offs[k], self.lay.Ts[k]
            g = self.glu[off:off + T]
            ref, conv = OR.dwconv(g, self.dw, self.ln_w, self.ln_b)
            z = np.abs(np.concatenate([np.zeros((self.ks - 1, D)), g.astype(np.float64)]))
            e_conv = self.ks * U24 * sum(z[kk:kk + T] * np.abs(self.dw[kk].astype(np.float64)) for kk in range(self.ks))
            e_ln = LR.layer_norm_bound(conv, self.ln_w, self.ln_b, dx=e_conv)
            out.append((slice(off, off + T), ref, 1.1 * e_ln + EXPF_REL * np.abs(ref)))
        return out


def run_off_dwconv(dv: Dev, s: OffConvSetup, act_bf16):
    M = s.lay.M
    c = ConvCase()
    c.glu, c.tpos, c.M = dv.up(s.glu, SLACK * D * 4), dv.up(s.lay.frame.astype(np.int32)), M
    c.dw, c.ks, c.ln_w, c.ln_b = dv.up(s.dw), s.ks, dv.up(s.ln_w), dv.up(s.ln_b)
    c.out, c.act_bf16 = dv.new((M + SLACK) * D * (2 if act_bf16 else 4)), int(act_bf16)
    assert dv.L.offline_harness_dwconv(C.byref(c)) == 0, dv.err()
    out = dv.get(c.out, np.uint16 if act_bf16 else np.uint32)
    out = out[:(len(out) // D) * D].reshape(-1, D)
    owned_rows_only(out, np.arange(len(out)) < M, "dwconv out")
    got = act_values(out[:M].reshape(-1), act_bf16).reshape(M, D)
    assert np.all(np.isfinite(got))
    return got


@pytest.mark.parametrize("act_bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("ks", DWCONV_KS)
def test_off_dwconv(ks, act_bf16):
    s = OffConvSetup(ks, seed=int(act_bf16))
    with dev() as dv:
        got = run_off_dwconv(dv, s, act_bf16)
    for rows, ref, bound in s.reference():
        r = check_bounded(got[rows], ref, bound, 2.0 ** -8 if act_bf16 else 2.0 ** -23, f"k_off_dwconv ks {ks} T {rows.stop - rows.start}")
        print(f"k_off_dwconv ks {ks} T {rows.stop - rows.start} bf16 {act_bf16}: worst |got - ref| / bound = {r:.3f}")


def test_off_dwconv_eps_on_rows_of_tiny_variance():
    """rows ~ TINY N(0, 1): the conv's variance is about eps = 1e-5, the bound ~1e-4 of the output, a wrong eps or divisor far outside it"""
    s = OffConvSetup(9, seed=7, scale=TINY)
    with dev() as dv:
        got = run_off_dwconv(dv, s, False)
    for rows, ref, bound in s.reference():
        if rows.stop - rows.start >= 9:                                      # rows with a full history: the conv of 9 N(0, 1 / 9) taps has the input's variance
            var = OR.dwconv(s.glu[rows], s.dw, s.ln_w, s.ln_b)[1].var(-1)[8:]
            assert 0.3e-5 < float(var.min()) and float(var.max()) < 3e-5
            assert float(np.median(bound[8:] / np.abs(ref[8:]))) < 1e-3, "the bound is tight here"
        print(f"tiny variance k_off_dwconv T {rows.stop - rows.start}: {check_bounded(got[rows], ref, bound, 2.0 ** -23, 'k_off_dwconv'):.3f}")


# ==== conv0 + ReLU + depthwise 3x3 =================================================================================================================
@pytest.mark.parametrize("kernel,out_bf16", CONV0_KERNELS, ids=lambda v: str(v))
def test_off_conv0_dw(kernel, out_bf16):
    takes(conv0_kernel(out_bf16), kernel)
    s = SubSetup(seed=int(out_bf16))
    assert s.h2[s.tested[0]] == 0 and s.max_h2 == sub_h2(33) == 9 and min(s.h2[k] for k in s.tested[1:]) == 1      # grid rows t2 >= H2 in every shorter utterance
    row = 33 * SUBC
    with dev() as dv:
        c = SubCase()
        c.desc, c.B, c.max_h2, c.mel, c.mel_rows = dv.up(s.desc), s.B, s.max_h2, dv.up(s.mel, SLACK * NMEL * 4), len(s.mel)
        c.w0t, c.b0, c.w2t, c.b2 = dv.up(s.wt(s.w0)), dv.up(s.b0), dv.up(s.wt(s.w2)), dv.up(s.b2)
        c.out, c.out_rows, c.out_bf16 = dv.new(s.out_rows * row * (2 if out_bf16 else 4)), s.out_rows, int(out_bf16)
        assert dv.L.offline_harness_conv0_dw(C.byref(c)) == 0, dv.err()
        out = dv.get(c.out, np.uint16 if out_bf16 else np.uint32)
    out = out[:(len(out) // row) * row].reshape(-1, row)
    owned = np.zeros(len(out), bool)
    for k in range(s.B):
        owned[s.out_row[k]:s.out_row[k] + s.h2[k]] = True
    owned_rows_only(out, owned, "conv0_dw out")                              # the row behind every utterance, every row of n_mel = 0, the rows behind the batch
    got = np.full((len(out), row), np.nan, np.float32)
    got[owned] = act_values(out[owned].reshape(-1), out_bf16).reshape(-1, row)
    assert np.all(np.isfinite(got[owned]))
    for k in s.tested:
        g = got[s.out_row[k]:s.out_row[k] + s.h2[k]].reshape(s.h2[k], 33, SUBC)
        ref, bound = s.reference(k)
        assert ref.shape == g.shape
        if s.h2[k] == 0:
            continue
        r = check_bounded(g, ref, bound, 2.0 ** -8 if out_bf16 else 0.0, f"{conv0_kernel(out_bf16)} n_mel {s.n_mel[k]}")       # every column, 0 and 32 included
        print(f"{conv0_kernel(out_bf16)} n_mel {s.n_mel[k]}: worst |got - ref| / bound = {r:.3f}")
        if not out_bf16:
            want = conv_front_f32(s.utterance(k), s.wt(s.w0), s.b0, s.wt(s.w2), s.b2)
            assert np.array_equal(g, want), f"n_mel {s.n_mel[k]}: not the bits of the documented operation order"


# ==== decode window, decoder reset ===================================================================================================================
def test_off_window():
    n_b, first = (0, 1, 255, 256), (3, 7, 261, 530)                         # wd.x: a multiple of nothing
    B, W, rows = len(n_b), DEC_WIN, 530 + 256
    rng = rng_of("off-window")
    src = rng.standard_normal((rows, JNT)).astype(np.float32)
    win = np.array([(first[b], n_b[b], 0, 0) for b in range(B)], np.int32)
    with dev() as dv:
        c = WinCase()
        c.encproj, c.rows, c.win, c.B, c.W = dv.up(src, SLACK * JNT * 4), rows, dv.up(win), B, W      # frozen: the source is untouched
        c.out = dv.new((B + 1) * W * JNT * 4)
        assert dv.L.offline_harness_window(C.byref(c)) == 0, dv.err()
        out = dv.get(c.out, np.uint32)
    out = out[:(B + 1) * W * JNT].reshape(B + 1, W, JNT)
    for b in range(B):
        assert np.array_equal(out[b, :n_b[b]], src[first[b]:first[b] + n_b[b]].view(np.uint32)), f"window {b}: not a copy of rows {first[b]} .. + {n_b[b]}"
        assert np.all(out[b, n_b[b]:] == SENT * 0x10001), f"window {b}: rows >= n_b = {n_b[b]} were written"
    assert np.all(out[B] == SENT * 0x10001), "a window behind the batch was written"


def test_off_dec_reset():
    B = 3
    with dev() as dv:
        c = ResetCase()
        c.B, c.h, c.c, c.ctrl = B, dv.new((B + 1) * 4 * HID * 4), dv.new((B + 1) * 4 * HID * 4), dv.new((B + 1) * 4 * len(DEC_CTRL))
        assert dv.L.offline_harness_dec_reset(C.byref(c)) == 0, dv.err()
        h, cc, ctrl = dv.get(c.h, np.uint32), dv.get(c.c, np.uint32), dv.get(c.ctrl, np.uint32)
    for name, state in (("h", h), ("c", cc)):
        assert not state[:B * 4 * HID].any(), f"{name}: not zero in the B slots"
        assert np.all(state[B * 4 * HID:] == SENT * 0x10001), f"{name}: slot B was written"
    want = dict.fromkeys(DEC_CTRL, 0)
    want.update(prev_token=BLANK, dirty=1)                                   # k_stream_reset's values: blank start, no committed candidate
    got = ctrl[:B * len(DEC_CTRL)].view(np.int32).reshape(B, len(DEC_CTRL))
    for b in range(B):
        assert dict(zip(DEC_CTRL, (int(x) for x in got[b]))) == want, f"slot {b}"
    assert np.all(ctrl[B * len(DEC_CTRL):] == SENT * 0x10001), "ctrl: slot B was written"


# ==== the harness refuses, the list of kernels ==========================================================================================================
def test_harness_refuses_what_the_kernels_do_not_index():
    """a case outside the kernels' indexing is an error string of the harness, never a launch"""
    with dev() as dv:
        L = dv.L
        a = AttnCase()
        M = MAX_T + 1
        a.qkv, a.pos, a.bias_u, a.bias_v = dv.new(M * QKV_LD * 2), dv.new(NREL * D * 2), dv.new(D * 4), dv.new(D * 4)
        a.ctx, a.M, a.act_bf16, a.n_items = dv.new(M * D * 2), M, 1, 1
        for item, why in (((0, M, 0, 0), "T outside"), ((M - 4, 5, 0, 0), "off + T"), ((0, 0, 0, 0), "T outside"), ((0, 8, 8, 0), "first query row"), ((0, 80, 16, 0), "first query row"),
                          ((-1, 4, 0, 0), "off + T")):
            a.items = dv.up(np.array([item], np.int32))
            assert L.offline_harness_attention(C.byref(a)) == -1 and why in dv.err(), dv.err()
        a.act_bf16 = 0                                                       # the same buffers hold half as many f32 rows
        assert L.offline_harness_attention(C.byref(a)) == -1 and "qkv" in dv.err()
        cv = ConvCase()
        cv.glu, cv.dw, cv.ln_w, cv.ln_b, cv.out, cv.M, cv.act_bf16 = dv.new(4 * D * 4), dv.new(MAX_KS * D * 4), dv.new(D * 4), dv.new(D * 4), dv.new(4 * D * 4), 4, 0
        cv.tpos, cv.ks = dv.up(np.array([0, 1, 2, 3], np.int32)), MAX_KS + 1
        assert L.offline_harness_dwconv(C.byref(cv)) == -1 and "ks" in dv.err()
        cv.tpos, cv.ks = dv.up(np.array([0, 2, 0, 1], np.int32)), 9                         # frame 2 at row 1: two rows in front of the buffer's first
        assert L.offline_harness_dwconv(C.byref(cv)) == -1 and "tpos" in dv.err()
        sc = SubCase()
        sc.w0t, sc.b0, sc.w2t, sc.b2 = dv.new(9 * SUBC * 4), dv.new(SUBC * 4), dv.new(9 * SUBC * 4), dv.new(SUBC * 4)
        sc.mel, sc.mel_rows, sc.out, sc.out_rows, sc.B, sc.max_h2 = dv.new(8 * NMEL * 4), 8, dv.new(2 * 33 * SUBC * 4), 2, 1, 3
        for d, why in (((1, 8, 0, 0), "mel rows"), ((0, 8, 0, 0), "output rows"), ((0, 3, 1, 0), "output rows")):
            sc.desc = dv.up(np.array([d], np.int32))
            assert L.offline_harness_conv0_dw(C.byref(sc)) == -1 and why in dv.err(), dv.err()
        w = WinCase()
        w.encproj, w.rows, w.B, w.W, w.out = dv.new(10 * JNT * 4), 10, 1, 4, dv.new(4 * JNT * 4)
        w.win = dv.up(np.array([(8, 3, 0, 0)], np.int32))
        assert L.offline_harness_window(C.byref(w)) == -1 and "source rows" in dv.err()
        r = ResetCase()
        r.B, r.h, r.c, r.ctrl = 2, dv.new(2 * 4 * HID * 4), dv.new(4 * HID * 4), dv.new(2 * 4 * len(DEC_CTRL))
        assert L.offline_harness_dec_reset(C.byref(r)) == -1 and "buffer c" in dv.err()


def planned_kernels():
    """the kernel every case of this file is there for, by the launchers' rules applied to the cases' parameters"""
    out = {attention_kernel(bf16) for _, bf16, _ in SELECTOR_CASES} | {attention_kernel(bf16) for _, bf16 in ATTN_KERNELS}
    out |= {conv0_kernel(b) for _, b in CONV0_KERNELS}
    return out | {"k_off_dwconv", "k_off_window", "k_off_dec_reset"}          # launchers with one kernel each


def source_kernels():
    """the __global__ functions of kernels_offline.hip; a template <bool> kernel counts as its two instances.  Every `__global__` of the file must be one the
    pattern understands, so that a kernel declared in another form cannot go unnoticed"""
    names = set()
    src = SOURCE.read_text()
    found = list(re.finditer(r"(?:template\s*<([^>]*)>\s*)?(?:static\s+)?__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(k_\w+)\s*\(", src))
    assert len(found) == src.count("__global__"), "a __global__ of kernels_offline.hip is declared in a form this test does not read"
    for m in found:
        if m.group(1) is None:
            names.add(m.group(2))
        else:
            assert re.fullmatch(r"bool\s+\w+", m.group(1).strip()), f"{m.group(2)}: template parameters this test cannot enumerate: <{m.group(1)}>"
            names |= {f"{m.group(2)}<true>", f"{m.group(2)}<false>"}
    return names


def test_every_offline_kernel_is_reached():
    assert source_kernels() == planned_kernels(), (sorted(source_kernels() - planned_kernels()), sorted(planned_kernels() - source_kernels()))
