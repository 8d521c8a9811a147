"""Every kernel of kernels_layer.hip and kernels_fused.hip, alone, against a float64 reference of the operation (tests/layer_ref.py, tests/gemm_ref.py).

tests/helpers/layer_harness.hip runs ONE launch through the product's launcher (launch_post, launch_attention, launch_dwconv, launch_fused_skinny,
launch_fused_skinny_group) on buffers [guard | body | guard] whose every byte that is not an input is the sentinel 0xFFC5 (NaN as bf16 and, doubled,
as f32), and returns every buffer whole.  Each case states the kernel the launcher's rule takes, restated here (`attention_kernel`, `dwconv_kernel`,
`fused_kernel`: the launchers have no plan object); test_every_kernel_is_reached checks the list.  k_attention<true> is unreached: launch_attention takes
k_attention_mfma for every bf16 T <= 16 and TMAX is 14.

Poison.  K / V pool: one slot more than the case uses, all sentinel; in a used slot every ring row outside [kv_head, kv_head + 70 + TS) mod KVC is
sentinel in both halves; the masked ring rows (offset < 70 - valid_len) are finite -- the kernels add -1e9 to a score they still compute -- and loud
(|K|, |V| = 64 in bounded mode).  posproj has exactly 70 + 2 T - 1 rows.  Conv-cache pool: one unused slot, and the parity buffer being written starts
as sentinel.  q / GLU / A / x rows at index >= M are NaN (the slack rows of the engine's workspaces).

Selector mode (`==`).  q = 0, bias_u = 32 e0, bias_v = 32 e1 in every head; content run: K[ring row][head, 0] = 64 rank, P = 0; position run:
P[r][head, 1] = 64 rank(r), K = 0; rank = a per-head random permutation onto bf16-exact integers.  A score is 2048 rank / sqrt(128): neighbours are
>= 181 apart, exp(-181) = 0 in f32, so every softmax is one-hot and the context row equals, bit for bit, the V row (small integers naming (stream, row,
column)) of the highest-ranked key the query may attend -- inside its own 70 + T window, unmasked, through the rel-shift.  The expectation is computed
from that definition.  Besides random seeds, targeted runs lift the top rank onto the first unmasked key, the last masked key, window key 0, key
70 + T - 1 and the ring rows on either side of the wrap.

Bounded mode.  Operands random, rounded to the operand type, per element against layer_ref:
  attention   |got - ref| <= (2 Delta_i + omega + EXPF_REL) sum_j w_j |V_jd| + o |ref|, Delta_i = max over unmasked j of
              scale (rho + 256 2^-24) (|q + u| . |K_j| + |q + v| . |P_r|): a score off by delta changes a softmax weight by at most a factor e^(2 delta).
              rho = 2^-9 where q + bias is rounded to bf16 (mfma, row1, fused), 0 for k_attention<false>; omega = 2^-8 where the weights are rounded to bf16
              (mfma), else 2^-23 KV; o = 2^-8 for bf16 outputs, else 2^-23.  The operands are scaled so that Delta_i <= 0.05 (asserted).
  LayerNorm   layer_ref.layer_norm_bound, the first-order forward error of the two-pass f32 LayerNorm over n = 1024 terms with u = 2^-24:
                mean      (n + 1) u mean|x|                      an n-term sum in any order ((n - 1) u sum|x|) and one multiply
                d = x - mean:  e_d = e_mean + u |d|
                variance  mean(2 |d| e_d) + (n + 3) u var        perturbed squares, the n-term sum, one square and one multiply each
                1 / sqrt  (e_var / (2 (var + eps)) + 4 u) / sd   derivative of v^-1/2; add, sqrt, divide
                y = d inv:  e_d / sd + |d| e_inv + u |y|;  out = y w + b:  e_y |w| + 2 u (|y w| + |out|)
              an input known only to dx (the residual sum, the conv taps, a first LayerNorm) adds mean(dx) to the mean and dx to d.
  dwconv      taps: ks u sum_k |z w|; that through the LayerNorm bound, through SiLU (|silu'| <= 1.1), plus EXPF_REL |ref|.
  bf16 outputs add 2^-8 |ref|.
EXPF_REL is tests/test_gpu_gemm_kernels.py's constant.  No tolerance here is measured on a kernel.
Both modes: outputs finite, and every byte the launch does not own still the sentinel (rows >= M, guards, unused slots, other streams' slots); every
read-only buffer of a launch (operands, K / V pool, posproj, weights, descriptors, with their poison and guards) is downloaded after it and must be bit for bit
what was uploaded (Dev.check_inputs).  test_layer_norm_eps_on_rows_of_tiny_variance runs every LayerNorm body on rows of variance ~ eps, where the analytic
bound is ~1e-4 of the output and a wrong eps or divisor is far outside it (on N(0, 1) rows the f32 kernels sit 200 to 500 times under the bound)."""
from __future__ import annotations

import ctypes as C
import zlib
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi
from tests import gemm_ref as R
from tests import layer_ref as LR
from tests.test_gpu_gemm_kernels import EXPF_REL

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HELPER = ROOT / "tests" / "helpers" / "liblayer_harness.so"
GUARD = 256 * 1024
SENT = 0xFFC5
D, NH, DH, LCTX, KVC, TMAX, MAXNEW = 1024, 8, 128, 70, 326, 14, 256
PRO_LN, PRO_PLAIN, PRO_ATTN, PRO_DWCONV = range(4)
PRO_NAMES = ["PRO_LN", "PRO_PLAIN", "PRO_ATTN", "PRO_DWCONV"]
U24 = 2.0 ** -24
UNREACHED = {"k_attention<true>": "launch_attention takes k_attention_mfma for every bf16 T <= 16 and TMAX is 14"}
KERNELS = ["k_post", "k_attention<false>", "k_attention_mfma", "k_attention_row1", "k_dwconv", "k_dwconv_stream<7>"] + \
          [f"k_fused_skinny<{p},{m}>" for p in PRO_NAMES for m in (1, 2, 16) if not (p == "PRO_ATTN" and m == 16)] + \
          [f"k_fused_skinny_grp<{p},{m}>" for p in ("PRO_LN", "PRO_ATTN", "PRO_DWCONV") for m in (1, 2)]


# ---- the launchers' rules, restated -------------------------------------------------------------------------------------------------------
def attention_kernel(bf16, T, TS):
    if bf16 and T == 1 and TS == 1:
        return "k_attention_row1"
    if bf16 and T <= 16:
        return "k_attention_mfma"
    return "k_attention<true>" if bf16 else "k_attention<false>"


def dwconv_kernel(stream_form, ks, T, B):
    return "k_dwconv_stream<7>" if stream_form and ks == 9 and T >= 7 and T % 7 == 0 and B >= 256 else "k_dwconv"


def fused_kernel(pro, M, K, splits, grouped=False):
    fits_u2 = pro != PRO_DWCONV or (K // 32 // splits + 3) // 4 <= 2
    mmax = 1 if M == 1 and fits_u2 else 2 if (M <= 2 or grouped) else 16
    return f"k_fused_skinny{'_grp' if grouped else ''}<{PRO_NAMES[pro]},{mmax}>"


def takes(name, want):
    assert name == want, f"the launcher's rule takes {name}, the case is there for {want}"


# ---- the harness -----------------------------------------------------------------------------------------------------------------------------
def _ints(*names):
    return [(n, C.c_int) for n in names]


class PostCase(C.Structure):
    _fields_ = _ints("x", "M", "part", "splits") + [("scale", C.c_float)] + _ints("ln1_w", "ln1_b", "ln_out", "ln2_w", "ln2_b", "a_out", "act_bf16", "copy_out")


class AttnCase(C.Structure):
    _fields_ = _ints("q", "kv_pool", "n_slots", "act_bf16", "posproj", "bias_u", "bias_v", "rows", "B", "T", "TS", "ctx_out")


class ConvCase(C.Structure):
    _fields_ = _ints("glu", "cc_pool", "n_slots", "dw", "ln_w", "ln_b", "rows", "B", "T", "ks", "c_out", "act_bf16", "stream_form")


class FusedCase(C.Structure):
    _fields_ = _ints("pro", "M", "N", "K", "splits", "epi", "ldo", "ldo_act", "T", "A", "lda", "W", "out_f32", "out_act", "q_out", "kv_pool", "n_slots", "rows",
                     "x_in", "x_out", "part", "part_splits") + [("scale", C.c_float)] + _ints("lno_w", "lno_b", "ln_w", "ln_b") + [("at", AttnCase), ("cv", ConvCase)]


def _no_handles(s):
    for name, typ in s._fields_:
        if typ is C.c_int and name in ("x", "part", "ln1_w", "ln1_b", "ln2_w", "ln2_b", "a_out", "copy_out", "q", "kv_pool", "posproj", "bias_u", "bias_v", "rows", "ctx_out",
                                       "glu", "cc_pool", "dw", "ln_w", "ln_b", "c_out", "A", "W", "out_f32", "out_act", "q_out", "x_in", "x_out", "lno_w", "lno_b"):
            setattr(s, name, -1)
        elif typ in (AttnCase, ConvCase):
            _no_handles(getattr(s, name))
    return s


@lru_cache(maxsize=None)
def harness():
    if not HELPER.exists():
        pytest.fail("tests/helpers/liblayer_harness.so not built: __graft_entry__.build() warns when the helper fails to compile (a changed FusedParams, AttnParams "
                    "or ConvParams?); these tests do not skip")
    C.CDLL(str(capi.LIB_PATH), mode=C.RTLD_GLOBAL)          # the helper's undefined nasr:: symbols resolve against the product library
    L = C.CDLL(str(HELPER))
    L.layer_harness_error.restype = C.c_char_p
    L.layer_harness_alloc.argtypes = [C.c_longlong, C.c_int]
    L.layer_harness_total_bytes.restype = C.c_longlong
    L.layer_harness_put.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_longlong]
    L.layer_harness_get.argtypes = [C.c_int, C.c_void_p]
    L.layer_harness_to_bf16.argtypes = [C.c_int, C.c_int, C.c_longlong]
    for i, s in enumerate((PostCase, AttnCase, ConvCase, FusedCase)):
        assert L.layer_harness_struct_bytes(i) == C.sizeof(s), s
    assert L.layer_harness_struct_bytes(4) == 32 and L.layer_harness_sentinel() == SENT
    assert [L.layer_harness_constant(i) for i in range(7)] == [D, NH, DH, LCTX, TMAX, MAXNEW, KVC]
    return L


class Dev:
    """device buffers of one launch (or of the launches that are compared with each other); everything is freed on exit"""

    def __init__(self, lib=None, prefix="layer_harness"):
        """lib, prefix: another harness with the same buffer entries (<prefix>_alloc, _put, _get, ...), as tests/test_gpu_offline_kernels.py passes"""
        self.L = lib if lib is not None else harness()
        self.prefix = prefix
        self.frozen = {}          # handle -> the whole buffer, guards included, as a launch must leave it: every input that no launch may write
        assert self.fn("init")(0) == 0, self.err()

    def fn(self, name):
        return getattr(self.L, f"{self.prefix}_{name}")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.check_inputs()
        finally:
            self.fn("free_all")()

    def check_inputs(self):
        """every read-only buffer -- operands, pools with their unused slots and poisoned rows, slack rows, weights, descriptors -- and its guards: bit for bit as uploaded"""
        for h, want in self.frozen.items():
            assert np.array_equal(self.raw(h), want), f"a launch wrote into read-only buffer {h} ({want.size * 2} bytes with guards)"

    def err(self):
        return self.fn("error")().decode()

    def new(self, nbytes):
        h = self.fn("alloc")(int(nbytes), GUARD)
        assert h >= 0, self.err()
        return h

    def up(self, arr, slack_bytes=0, written=False):
        """a buffer that holds arr, `slack_bytes` of sentinel behind it; written: a launch may write it (it is then not checked as an input)"""
        arr = np.ascontiguousarray(arr)
        h = self.new(arr.nbytes + slack_bytes)
        assert self.fn("put")(h, 0, arr.ctypes.data, arr.nbytes) == 0, self.err()
        if not written:
            want = np.full(self.fn("total_bytes")(h) // 2, SENT, np.uint16)
            want[GUARD // 2:GUARD // 2 + arr.nbytes // 2] = arr.reshape(-1).view(np.uint16)
            self.frozen[h] = want
        return h

    def get(self, h, dtype):
        """the body as `dtype`; the guards in front of and behind it must still be sentinel"""
        n = self.fn("total_bytes")(h)
        raw = np.empty(n // 2, np.uint16)
        assert self.fn("get")(h, raw.ctypes.data) == 0, self.err()
        g = GUARD // 2
        assert np.all(raw[:g] == SENT), "the launch wrote in front of a buffer"
        assert np.all(raw[-g:] == SENT), "the launch wrote behind a buffer"
        return raw[g:-g].view(dtype)

    def raw(self, h):
        n = self.fn("total_bytes")(h)
        raw = np.empty(n // 2, np.uint16)
        assert self.fn("get")(h, raw.ctypes.data) == 0, self.err()
        return raw

    def bf16_of(self, arr_f32, slack_bytes=0):
        """arr (f32, + sentinel slack) converted on the device by the product's launch_f32_to_bf16: the sentinel stays the sentinel"""
        src = self.up(np.asarray(arr_f32, np.float32), slack_bytes)
        n = (np.asarray(arr_f32).size * 4 + slack_bytes) // 4
        dst = self.new(n * 2)
        assert self.fn("to_bf16")(src, dst, n) == 0, self.err()
        self.frozen[dst] = self.raw(dst)
        return dst

    def packed(self, W):
        N, K = W.shape
        src, dst = self.up(np.asarray(W, np.float32)), self.new(N * K * 2)
        assert self.fn("pack_weight")(src, dst, N, K) == 0, self.err()
        self.frozen[dst] = self.raw(dst)
        return dst


def rest_is_sentinel(body, owned_elems, what):
    """everything behind the first owned_elems elements of a downloaded body"""
    tail = body[owned_elems:].view(np.uint16)
    assert np.all(tail == SENT), f"{what}: written behind its {owned_elems} elements"


def slack_rows(M):
    """rows of the engine workspace a step of M rows runs in, minus M (gemm_harness_workspace_rows)"""
    return max((M + TMAX - 1) // TMAX * TMAX, MAXNEW) - M


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def row_descs(slots, valid=None, head=None, par=None):
    B = len(slots)
    rd = np.zeros((B, 8), np.int32)
    rd[:, 0] = slots
    rd[:, 1] = valid if valid is not None else 0
    rd[:, 2] = head if head is not None else 0
    rd[:, 4] = par if par is not None else 0
    rd[:, 6] = -1
    return rd


def act_bits(x, bf16):
    """values -> the bits the kernel reads: bf16 (uint16) or f32 (uint32); NaN entries become the sentinel"""
    x = np.asarray(x, np.float32)
    if bf16:
        return np.where(np.isnan(x), np.uint16(SENT), R.bf16_bits(np.nan_to_num(x))).astype(np.uint16)
    return np.where(np.isnan(x), np.uint32(SENT * 0x10001), np.nan_to_num(x).view(np.uint32)).astype(np.uint32)


def act_values(bits, bf16):
    return R.bf16_to_f32(bits) if bf16 else np.ascontiguousarray(bits).view(np.float32)


IDENT = np.eye(D, dtype=np.float32)


# ==== attention =================================================================================================================================
# bf16-exact non-negative integers in rising order: the rank values of selector mode (at most 70 + 252 + 2 of them are needed)
EXACT_INTS = np.array(list(range(256)) + list(range(256, 512, 2)), np.float64)


class AttnSetup:
    """the streams of one attention case: slots permuted in a pool of B + 1, per-stream valid_len and kv_head (rotated by `rot`)"""

    def __init__(self, B, T, TS, rot=0):
        self.B, self.T, self.TS, self.G = B, T, TS, TS // T
        assert TS % T == 0 and TS <= MAXNEW and 1 <= T <= TMAX
        G = self.G
        cross = 63 if G == 1 else max(1, LCTX - T * max(1, G // 2))          # valid_len + g T passes 70 inside the launch
        valid = [0, LCTX, cross]
        head = [0, KVC - 1, KVC - LCTX - TS // 2]
        self.n_slots = B + 1
        self.slots = [2, 0, 3][:B] if B == 3 else list(range(B, 0, -1))
        self.valid = [valid[(b + rot) % 3] for b in range(B)] if B > 1 else [valid[rot % 3]]
        self.head = [head[(b + 2 * rot) % 3] for b in range(B)] if B > 1 else [head[(1 + rot) % 3]]
        self.n_off = LCTX + TS                                              # ring rows of a stream the launch may read
        self.n_rel = LCTX + 2 * T - 1

    def rows(self):
        return row_descs(self.slots, self.valid, self.head)

    def pool(self, Kv, Vv, bf16):
        """Kv, Vv [B][n_off][1024] values by ring offset -> the pool's bits [n_slots][2][KVC][1024], sentinel wherever the launch must not read"""
        pool = np.full((self.n_slots, 2, KVC, D), np.nan, np.float32)
        for b in range(self.B):
            ring = (self.head[b] + np.arange(self.n_off)) % KVC
            pool[self.slots[b], 0, ring] = Kv[b]
            pool[self.slots[b], 1, ring] = Vv[b]
        return act_bits(pool, bf16)

    def chunks(self):
        """(b, g, validity of chunk g, ring offsets of its 70 + T keys, unmasked)"""
        T = self.T
        for b in range(self.B):
            for g in range(self.G):
                v = min(self.valid[b] + g * T, LCTX)
                j = np.arange(LCTX + T)
                yield b, g, v, g * T + j, j >= LCTX - v


def v_marks(s: AttnSetup):
    """V[b][offset][column]: small integers (exact in bf16) that name (stream, ring offset, column)"""
    b, o, d = np.arange(s.B)[:, None, None], np.arange(s.n_off)[None, :, None], np.arange(D)[None, None, :]
    return ((o * 37 + d * 11 + b * 101) % 255 - 127).astype(np.float32)


def selector_ranks(s: AttnSetup, run, seed, target):
    """content: [B][8][n_off] rank of every ring offset; position: [8][n_rel] rank of every position row.  target lifts the top rank of every
    (stream, head) onto one key of a middle chunk (content) / one position row (position)"""
    rng = rng_of("ranks", s.B, s.T, s.TS, run, seed)
    T, g = s.T, s.G // 2
    if run == "content":
        rank = np.stack([np.stack([rng.permutation(s.n_off) for _ in range(NH)]) for _ in range(s.B)])
        for b in range(s.B):
            v = min(s.valid[b] + g * T, LCTX)
            wrap = KVC - s.head[b]                                           # ring offset of ring row 0
            o = {None: None, "first_unmasked": g * T + LCTX - v, "last_masked": g * T + LCTX - v - 1 if v < LCTX else None,
                 "key0": g * T if v == LCTX else None, "last_key": g * T + LCTX + T - 1,
                 "wrap_lo": wrap - 1 if 0 < wrap <= s.n_off else None, "wrap_hi": wrap if 0 <= wrap < s.n_off else None}[target]
            if o is not None:
                for h in range(NH):
                    top = int(np.argmax(rank[b, h]))
                    rank[b, h, [o, top]] = rank[b, h, [top, o]]
        return rank
    rank = np.stack([rng.permutation(s.n_rel) for _ in range(NH)])
    vc = min(s.valid[-1] + g * T, LCTX)
    r = {None: None, "first_unmasked": LCTX - vc + T - 1, "last_masked": LCTX - vc - 1 + T - 1 if vc < LCTX else None, "key0": T - 1, "last_key": LCTX + 2 * T - 2,
         "wrap_lo": 0, "wrap_hi": LCTX + T - 1}[target]                      # position rows have no wrap: the two ends of the table of frame T - 1 / frame 0
    if r is not None:
        for h in range(NH):
            top = int(np.argmax(rank[h]))
            rank[h, [r, top]] = rank[h, [top, r]]
    return rank


def selector_case(s: AttnSetup, run, seed, target=None):
    """-> (q, K values, V values, P values, bias_u, bias_v, expected ctx [B TS][1024])"""
    rank = selector_ranks(s, run, seed, target)
    T = s.T
    Kv, P = np.zeros((s.B, s.n_off, D), np.float32), np.zeros((s.n_rel, D), np.float32)
    if run == "content":
        for h in range(NH):
            Kv[:, :, h * DH] = 64.0 * EXACT_INTS[rank[:, h]]
    else:
        for h in range(NH):
            P[:, h * DH + 1] = 64.0 * EXACT_INTS[rank[h]]
    Vv = v_marks(s)
    bu, bv = np.zeros(D, np.float32), np.zeros(D, np.float32)
    bu[0::DH], bv[1::DH] = 32.0, 32.0
    exp = np.zeros((s.B * s.TS, D), np.float32)
    for b, g, v, offs, unm in s.chunks():
        for h in range(NH):
            # scores [T][70 + T]: content (q + u) . K_j is the key's rank for every query; position (q + v) . P_r for every position row r, then the
            # reference's pad-and-reshape rel-shift (layer_ref.rel_shift: the definition, not the kernels' index form)
            scores = np.tile(rank[b, h, offs], (T, 1)) if run == "content" else LR.rel_shift(np.tile(rank[h], (T, 1)), LCTX + T)
            for i in range(T):
                win = int(np.argmax(np.where(unm, scores[i], -1)))
                exp[b * s.TS + g * T + i, h * DH:(h + 1) * DH] = Vv[b, offs[win], h * DH:(h + 1) * DH]
    return np.zeros((s.B * s.TS, D), np.float32), Kv, Vv, P, bu, bv, exp


def bounded_case(s: AttnSetup, bf16, kind):
    """random operands -> (q, K, V, P, bias_u, bias_v, ref ctx, bound); kind: "f32", "mfma", "row1" (also the fused prologue)"""
    rng = rng_of("attn-bounded", s.B, s.T, s.TS, bf16)
    rnd = R.bf16_round if bf16 else (lambda x: x)
    q = (0.7 * rng.standard_normal((s.B * s.TS, D))).astype(np.float32)
    Kv = rnd((0.7 * rng.standard_normal((s.B, s.n_off, D))).astype(np.float32))
    Vv = rnd(rng.standard_normal((s.B, s.n_off, D)).astype(np.float32))
    P = rnd((0.7 * rng.standard_normal((s.n_rel, D))).astype(np.float32))
    bu, bv = (0.5 * rng.standard_normal(D)).astype(np.float32), (0.5 * rng.standard_normal(D)).astype(np.float32)
    for b in range(s.B):                                                     # the masked ring rows: loud
        n = LCTX - min(s.valid[b], LCTX)
        Kv[b, :n] = 64.0 * rng.choice([-1.0, 1.0], (n, D))
        Vv[b, :n] = 64.0 * rng.choice([-1.0, 1.0], (n, D))
    rho = 0.0 if kind == "f32" else 2.0 ** -9
    omega = 2.0 ** -8 if kind == "mfma" else 2.0 ** -23 * (LCTX + s.T)
    o_rel = 2.0 ** -8 if bf16 else 2.0 ** -23
    T, scale = s.T, 1.0 / np.sqrt(float(DH))
    ref, bound = np.zeros((s.B * s.TS, D)), np.zeros((s.B * s.TS, D))
    worst_delta = 0.0
    for b, g, v, offs, unm in s.chunks():
        rows = slice(b * s.TS + g * T, b * s.TS + (g + 1) * T)
        w, unmasked, (qu, qv) = LR.attention_weights(q[rows], Kv[b, offs], P, bu, bv, v)
        assert np.array_equal(unmasked, unm)
        Va = np.abs(Vv[b, offs].astype(np.float64))
        for h in range(NH):
            sl = slice(h * DH, (h + 1) * DH)
            a1 = np.abs(qu[:, sl]) @ np.abs(Kv[b, offs][:, sl].astype(np.float64)).T                   # [T][KV]
            a2 = LR.rel_shift(np.abs(qv[:, sl]) @ np.abs(P[:, sl].astype(np.float64)).T, LCTX + T)
            delta = (scale * (rho + 256 * U24) * (a1 + a2))[:, unm].max(-1)                             # [T]
            worst_delta = max(worst_delta, float(delta.max()))
            ref[rows, sl] = w[h] @ Vv[b, offs][:, sl].astype(np.float64)
            bound[rows, sl] = (2 * delta + omega + EXPF_REL)[:, None] * (w[h] @ Va[:, sl])
    assert worst_delta <= 0.05, worst_delta
    return q, Kv, Vv, P, bu, bv, ref, bound + o_rel * np.abs(ref)


def run_attention(dev: Dev, s: AttnSetup, bf16, q, Kv, Vv, P, bu, bv):
    """-> the context rows [B TS][1024] as f32 values; rows >= M and the guards checked"""
    M = s.B * s.TS
    c = _no_handles(AttnCase())
    c.q = dev.up(q, slack_rows(M) * D * 4)
    c.kv_pool, c.n_slots, c.act_bf16 = dev.up(s.pool(Kv, Vv, bf16)), s.n_slots, int(bf16)
    c.posproj = dev.up(act_bits(P, bf16))
    c.bias_u, c.bias_v, c.rows = dev.up(bu), dev.up(bv), dev.up(s.rows())
    c.B, c.T, c.TS = s.B, s.T, s.TS
    c.ctx_out = dev.new((M + slack_rows(M)) * D * (2 if bf16 else 4))
    assert dev.L.layer_harness_attention(C.byref(c)) == 0, dev.err()
    out = dev.get(c.ctx_out, np.uint16 if bf16 else np.uint32)
    rest_is_sentinel(out, M * D, "ctx_out")
    got = act_values(out[:M * D], bf16).reshape(M, D)
    assert np.all(np.isfinite(got)), "a context element is not finite (unwritten, or poison reached it)"
    return got


ATTN_CASES = [("k_attention_row1", True, B, 1, 1) for B in (1, 3)] + \
             [("k_attention_mfma", True, 3, 1, TS) for TS in (2, 16, 18, 33)] + [("k_attention_mfma", True, 3, 2, TS) for TS in (2, 16, 22)] + \
             [("k_attention_mfma", True, 3, 7, TS) for TS in (7, 21)] + [("k_attention_mfma", True, 3, 14, TS) for TS in (14, 28, 252)] + \
             [("k_attention<false>", False, 3, T, TS) for (T, TS) in ((1, 1), (1, 3), (2, 4), (7, 7), (7, 14), (14, 14), (14, 42))]
TARGETS = ("first_unmasked", "last_masked", "key0", "last_key", "wrap_lo", "wrap_hi")
SEEDS = (0, 1, 2, 3)


def _attn_id(c):
    return f"{c[0]}-B{c[2]}-T{c[3]}-TS{c[4]}"


def _selector_runs():
    return [(run, seed, None) for run in ("content", "position") for seed in SEEDS] + [(run, 9, t) for run in ("content", "position") for t in TARGETS]


@pytest.mark.parametrize("case", ATTN_CASES, ids=_attn_id)
def test_attention_selector(case):
    kernel, bf16, B, T, TS = case
    takes(attention_kernel(bf16, T, TS), kernel)
    for run, seed, target in _selector_runs():
        s = AttnSetup(B, T, TS, rot=seed)
        q, Kv, Vv, P, bu, bv, exp = selector_case(s, run, seed, target)
        with Dev() as dev:
            got = run_attention(dev, s, bf16, q, Kv, Vv, P, bu, bv)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, f"{run} seed {seed} target {target}: {len(bad)} elements differ, first (row, column) {bad[0]}: got {got[tuple(bad[0])]}, want {exp[tuple(bad[0])]}"


@pytest.mark.parametrize("case", ATTN_CASES, ids=_attn_id)
def test_attention_bounded(case):
    kernel, bf16, B, T, TS = case
    takes(attention_kernel(bf16, T, TS), kernel)
    s = AttnSetup(B, T, TS)
    kind = "f32" if not bf16 else "row1" if kernel == "k_attention_row1" else "mfma"
    q, Kv, Vv, P, bu, bv, ref, bound = bounded_case(s, bf16, kind)
    with Dev() as dev:
        got = run_attention(dev, s, bf16, q, Kv, Vv, P, bu, bv)
    err = np.abs(got - ref)
    print(f"{_attn_id(case)}: worst |got - ref| / bound = {(err / bound).max():.3f}")
    assert np.all(err <= bound), f"worst ratio {(err / bound).max()} at {np.unravel_index(np.argmax(err / bound), err.shape)}"
    if T == 1:                                                               # valid_len = 0: the new row is the only unmasked key
        for b in range(B):
            if s.valid[b] == 0:
                assert np.array_equal(got[b * TS], Vv[b, LCTX]), "one unmasked key: the context is that V row"


# ---- attention through the fused prologue -----------------------------------------------------------------------------------------------------
def fused_attn_problem(dev: Dev, s: AttnSetup, q, Kv, Vv, P, bu, bv):
    """PRO_ATTN, W = identity, N = K = 1024, 8 heads = 8 K slices -> (FusedCase, output handle)"""
    M = s.B * s.TS
    c = _no_handles(FusedCase())
    c.pro, c.M, c.N, c.K, c.splits, c.epi, c.ldo, c.T = PRO_ATTN, M, D, D, NH, R.EPI_PART_F32, D, 1
    c.W = dev.packed(IDENT)
    c.out_f32 = dev.new(NH * M * D * 4)
    a = c.at
    a.q = dev.up(q, slack_rows(M) * D * 4)
    a.kv_pool, a.n_slots, a.act_bf16 = dev.up(s.pool(Kv, Vv, True)), s.n_slots, 1
    a.posproj = dev.up(act_bits(P, True))
    a.bias_u, a.bias_v, a.rows = dev.up(bu), dev.up(bv), dev.up(s.rows())
    a.B, a.T, a.TS = s.B, s.T, s.TS
    return c, c.out_f32


def fused_attn_panel(dev, h_out, M):
    """partial h holds head h's 128 context columns (the bf16 panel, exactly) and exact zeros elsewhere -> ctx [M][1024]"""
    out = dev.get(h_out, np.float32)
    rest_is_sentinel(out, NH * M * D, "out_f32")
    part = out[:NH * M * D].reshape(NH, M, D)
    assert np.all(np.isfinite(part))
    ctx = np.zeros((M, D), np.float32)
    for h in range(NH):
        sl = slice(h * DH, (h + 1) * DH)
        ctx[:, sl] = part[h][:, sl]
        rest = part[h].copy()
        rest[:, sl] = 0
        assert not rest.any(), f"partial {h} is not zero outside its head's columns"
    assert np.array_equal(R.bf16_round(ctx), ctx), "the panel is bf16"
    return ctx


FUSED_ATTN = [(1, 1, 1, "k_fused_skinny<PRO_ATTN,1>"), (2, 1, 1, "k_fused_skinny<PRO_ATTN,2>"), (1, 1, 2, "k_fused_skinny<PRO_ATTN,2>"), (1, 2, 1, "k_fused_skinny<PRO_ATTN,2>")]


def run_fused(dev, c, n=1, grouped=0):
    arr = (FusedCase * n)(*c) if n > 1 or grouped else (FusedCase * 1)(c)
    assert dev.L.layer_harness_fused(arr, n, grouped) == 0, dev.err()


@pytest.mark.parametrize("B,T,G,kernel", FUSED_ATTN, ids=lambda v: str(v))
def test_fused_attention(B, T, G, kernel):
    TS, M = T * G, B * T * G
    takes(fused_kernel(PRO_ATTN, M, D, NH), kernel)
    for run, seed, target in _selector_runs():
        s = AttnSetup(B, T, TS, rot=seed)
        q, Kv, Vv, P, bu, bv, exp = selector_case(s, run, seed, target)
        with Dev() as dev:
            c, h = fused_attn_problem(dev, s, q, Kv, Vv, P, bu, bv)
            run_fused(dev, c)
            got = fused_attn_panel(dev, h, M)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, f"{run} seed {seed} target {target}: {len(bad)} elements differ, first (row, column) {bad[0]}"
    for rot in (0, 1, 2):
        s = AttnSetup(B, T, TS, rot=rot)
        q, Kv, Vv, P, bu, bv, ref, bound = bounded_case(s, True, "row1")
        with Dev() as dev:
            c, h = fused_attn_problem(dev, s, q, Kv, Vv, P, bu, bv)
            run_fused(dev, c)
            got = fused_attn_panel(dev, h, M)
            err = np.abs(got - ref)
            print(f"fused attention B{B} T{T} G{G} rot {rot}: worst |got - ref| / bound = {(err / bound).max():.3f}")
            assert np.all(err <= bound), (err / bound).max()
            if T == 1 and G == 1:                                            # "operation for operation": the same bits as k_attention_row1
                takes(attention_kernel(True, 1, 1), "k_attention_row1")
                alone = run_attention(dev, s, True, q, Kv, Vv, P, bu, bv)
                assert np.array_equal(alone, got), "k_attention_row1 and the fused one-row prologue differ"


# ==== depthwise conv ==============================================================================================================================
class ConvSetup:
    def __init__(self, B, T, ks, seed=0, scale=1.0):
        rng = rng_of("conv", B, T, ks, seed)
        self.B, self.T, self.ks = B, T, ks
        self.n_slots = B + 1
        perm = rng.permutation(self.n_slots)
        self.slots = [int(x) for x in perm[:B]]
        self.par = [int((b + seed) & 1) for b in range(B)] if B > 1 else [1 - (seed & 1)]
        self.cache = (scale * rng.standard_normal((B, ks - 1, D))).astype(np.float32)      # scale: the size of the conv's inputs (tiny: eps dominates its LayerNorm)
        self.glu = (scale * rng.standard_normal((B * T, D))).astype(np.float32)
        self.dw = (rng.standard_normal((ks, D)) / np.sqrt(ks)).astype(np.float32)
        self.ln_w, self.ln_b = (1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32), (0.2 * rng.standard_normal(D)).astype(np.float32)

    def pool(self):
        pool = np.full((self.n_slots, 2, self.ks - 1, D), SENT * 0x10001, np.uint32)
        for b in range(self.B):
            pool[self.slots[b], self.par[b]] = self.cache[b].view(np.uint32)
        return pool

    def reference(self):
        """-> (ref [M][1024], bound before the output rounding, new caches [B][ks - 1][1024])"""
        T, ref, bound, caches = self.T, [], [], []
        for b in range(self.B):
            g = self.glu[b * T:(b + 1) * T]
            conv, new = LR.dwconv_taps(self.cache[b], g, self.dw)
            z = np.abs(np.concatenate([self.cache[b], g]).astype(np.float64))
            e_conv = self.ks * U24 * sum(z[k:k + T] * np.abs(self.dw[k].astype(np.float64)) for k in range(self.ks))
            ln = LR.layer_norm(conv, self.ln_w, self.ln_b)
            e_ln = LR.layer_norm_bound(conv, self.ln_w, self.ln_b, dx=e_conv)
            ref.append(R.silu(ln))
            bound.append(1.1 * e_ln + EXPF_REL * np.abs(ref[-1]))
            caches.append(new)
        return np.concatenate(ref), np.concatenate(bound), np.stack(caches)

    def fill(self, dev, cv, act_bf16, stream_form=0, with_out=True):
        M = self.B * self.T
        cv.glu = dev.up(self.glu, slack_rows(M) * D * 4)
        cv.cc_pool, cv.n_slots = dev.up(self.pool(), written=True), self.n_slots
        cv.dw, cv.ln_w, cv.ln_b = dev.up(self.dw), dev.up(self.ln_w), dev.up(self.ln_b)
        cv.rows = dev.up(row_descs(self.slots, par=self.par))
        cv.B, cv.T, cv.ks, cv.act_bf16, cv.stream_form = self.B, self.T, self.ks, int(act_bf16), stream_form
        if with_out:
            cv.c_out = dev.new((M + slack_rows(M)) * D * (2 if act_bf16 else 4))

    def check_pool(self, dev, h_pool, new_caches, writers=None):
        """the written parity == the last ks - 1 rows of [cache ; GLU] (streams in `writers`: all by default), the parity read unchanged, everything else sentinel"""
        pool = dev.get(h_pool, np.uint32)
        n = self.n_slots * 2 * (self.ks - 1) * D
        rest_is_sentinel(pool, n, "cc_pool")
        want = self.pool()
        for b in (range(self.B) if writers is None else writers):
            want[self.slots[b], self.par[b] ^ 1] = np.ascontiguousarray(new_caches[b], np.float32).view(np.uint32)
        assert np.array_equal(pool[:n].reshape(want.shape), want), "conv-cache pool: a written parity differs from the last ks - 1 rows, or something else was written"


def run_dwconv(dev, s: ConvSetup, act_bf16, stream_form=0):
    M = s.B * s.T
    c = _no_handles(ConvCase())
    s.fill(dev, c, act_bf16, stream_form)
    assert dev.L.layer_harness_dwconv(C.byref(c)) == 0, dev.err()
    out = dev.get(c.c_out, np.uint16 if act_bf16 else np.uint32)
    rest_is_sentinel(out, M * D, "c_out")
    got = act_values(out[:M * D], act_bf16).reshape(M, D)
    assert np.all(np.isfinite(got))
    return got, c.cc_pool


@pytest.mark.parametrize("ks", [9, 5, 32])
@pytest.mark.parametrize("T", [1, 2, 7, 14, 28])
def test_dwconv(ks, T):
    takes(dwconv_kernel(0, ks, T, 3), "k_dwconv")
    for act_bf16 in (True, False):
        s = ConvSetup(3, T, ks, seed=int(act_bf16))
        ref, bound, caches = s.reference()
        with Dev() as dev:
            got, h_pool = run_dwconv(dev, s, act_bf16)
            s.check_pool(dev, h_pool, caches)
        bound = bound + (2.0 ** -8 if act_bf16 else 2.0 ** -23) * np.abs(ref)
        err = np.abs(got - ref)
        print(f"k_dwconv ks {ks} T {T} bf16 {act_bf16}: worst |got - ref| / bound = {(err / bound).max():.3f}")
        assert np.all(err <= bound), (err / bound).max()


@pytest.mark.parametrize("T", [7, 14, 21])
def test_dwconv_stream(T):
    B = 256
    takes(dwconv_kernel(1, 9, T, B), "k_dwconv_stream<7>")
    takes(dwconv_kernel(0, 9, T, B), "k_dwconv")
    s = ConvSetup(B, T, 9, seed=T)
    ref, bound, caches = s.reference()
    bound = bound + 2.0 ** -8 * np.abs(ref)
    outs = []
    for stream_form in (1, 0):
        with Dev() as dev:
            got, h_pool = run_dwconv(dev, s, True, stream_form)
            s.check_pool(dev, h_pool, caches)
            outs.append(got)
    err = np.abs(outs[0] - ref)
    print(f"k_dwconv_stream<7> T {T}: worst |got - ref| / bound = {(err / bound).max():.3f}")
    assert np.all(err <= bound), (err / bound).max()
    assert np.array_equal(outs[0], outs[1]), "k_dwconv_stream<7> and k_dwconv differ"


def fused_conv_problem(dev, s: ConvSetup, splits):
    M = s.B * s.T
    c = _no_handles(FusedCase())
    c.pro, c.M, c.N, c.K, c.splits, c.epi, c.ldo, c.T = PRO_DWCONV, M, D, D, splits, R.EPI_PART_F32, D, 1
    c.W = dev.packed(IDENT)
    c.out_f32 = dev.new(splits * M * D * 4)
    s.fill(dev, c.cv, act_bf16=True, with_out=False)
    return c


def fused_panel(dev, h_out, M, splits):
    """identity W: partial s holds columns [s 1024 / splits, (s + 1) 1024 / splits) of the bf16 A panel and exact zeros elsewhere -> the panel [M][1024]"""
    out = dev.get(h_out, np.float32)
    rest_is_sentinel(out, splits * M * D, "out_f32")
    part = out[:splits * M * D].reshape(splits, M, D)
    assert np.all(np.isfinite(part))
    w = D // splits
    panel = np.concatenate([part[k][:, k * w:(k + 1) * w] for k in range(splits)], axis=1)
    assert np.array_equal(part.sum(0), panel), "a partial is not zero outside its K slice"
    assert np.array_equal(R.bf16_round(panel), panel), "the panel is bf16"
    return panel


FUSED_CONV = [(1, 1, 4, 1), (1, 1, 2, 2), (2, 1, 4, 2), (1, 2, 4, 2), (3, 1, 4, 16), (1, 7, 4, 16), (1, 14, 4, 16), (8, 2, 4, 16), (16, 1, 4, 16)]


@pytest.mark.parametrize("ks", [9, 5])
@pytest.mark.parametrize("B,T,splits,mmax", FUSED_CONV)
def test_fused_dwconv(B, T, splits, mmax, ks):
    M = B * T
    takes(fused_kernel(PRO_DWCONV, M, D, splits), f"k_fused_skinny<PRO_DWCONV,{mmax}>")
    s = ConvSetup(B, T, ks, seed=splits)
    ref, bound, caches = s.reference()
    bound = bound + 2.0 ** -8 * np.abs(ref)
    with Dev() as dev:
        c = fused_conv_problem(dev, s, splits)
        run_fused(dev, c)
        got = fused_panel(dev, c.out_f32, M, splits)
        s.check_pool(dev, c.cv.cc_pool, caches)          # block (0, 0) alone writes the caches: once, every stream's
    err = np.abs(got - ref)
    print(f"fused dwconv B{B} T{T} splits {splits} ks {ks}: worst |got - ref| / bound = {(err / bound).max():.3f}")
    assert np.all(err <= bound), (err / bound).max()


# ==== residual + LayerNorm =======================================================================================================================
class PostSetup:
    def __init__(self, M, splits, seed=0, scale=1.0):
        rng = rng_of("post", M, splits, seed)
        self.M, self.splits = M, splits
        self.x = (scale * rng.standard_normal((M, D))).astype(np.float32)
        self.part = (0.5 * rng.standard_normal((splits, M, D))).astype(np.float32)
        self.scale = 0.5
        self.ln = [((1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32), (0.2 * rng.standard_normal(D)).astype(np.float32)) for _ in range(2)]

    def reference(self, ln_first, ln_second):
        """-> (x', bound of x', a, bound of a) in float64"""
        x1, _ = LR.post(self.x, self.part, self.scale)
        e = (self.splits + 2) * U24 * (np.abs(self.x.astype(np.float64)) + self.scale * np.abs(self.part.astype(np.float64)).sum(0)) if self.splits else np.zeros_like(x1)
        if ln_first:
            x2, e2 = LR.layer_norm(x1, *self.ln[0]), LR.layer_norm_bound(x1, *self.ln[0], dx=e)
        else:
            x2, e2 = x1, e
        if not ln_second:
            return x2, e2, None, None
        return x2, e2, LR.layer_norm(x2, *self.ln[1]), LR.layer_norm_bound(x2, *self.ln[1], dx=e2)


def check_bounded(got, ref, bound, out_rel, what):
    bound = bound + out_rel * np.abs(ref)
    err = np.abs(got - ref)
    assert np.all(np.isfinite(got)), what
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    assert np.all(err <= bound), f"{what}: worst |got - ref| / bound = {ratio}"
    return ratio


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("splits", [0, 1, 4, 8])
def test_post(M, splits):
    takes("k_post", "k_post")
    worst = 0.0
    for ln_out in (0, 1):
        for act in (None, "bf16", "f32"):
            for copy in (0, 1):
                s = PostSetup(M, splits, seed=ln_out)
                x_ref, e_x, a_ref, e_a = s.reference(ln_out, act is not None)
                with Dev() as dev:
                    c = _no_handles(PostCase())
                    c.x, c.M, c.splits, c.scale, c.ln_out = dev.up(s.x, slack_rows(M) * D * 4, written=bool(splits or ln_out)), M, splits, s.scale, ln_out
                    if splits:
                        c.part = dev.up(s.part)
                    if ln_out:
                        c.ln1_w, c.ln1_b = dev.up(s.ln[0][0]), dev.up(s.ln[0][1])
                    if act:
                        c.ln2_w, c.ln2_b, c.act_bf16 = dev.up(s.ln[1][0]), dev.up(s.ln[1][1]), int(act == "bf16")
                        c.a_out = dev.new((M + slack_rows(M)) * D * (2 if act == "bf16" else 4))
                    if copy:
                        c.copy_out = dev.new((M + slack_rows(M)) * D * 4)
                    assert dev.L.layer_harness_post(C.byref(c)) == 0, dev.err()
                    x = dev.get(c.x, np.float32)
                    rest_is_sentinel(x, M * D, "x")
                    x = x[:M * D].reshape(M, D)
                    if splits or ln_out:
                        worst = max(worst, check_bounded(x, x_ref, e_x, 2.0 ** -23, "x"))
                    else:
                        assert np.array_equal(x, s.x), "x was written without a residual update or a LayerNorm to write"
                    if copy:
                        cp = dev.get(c.copy_out, np.float32)
                        rest_is_sentinel(cp, M * D, "copy_out")
                        assert np.array_equal(cp[:M * D].reshape(M, D), x), "copy_out is not the final x"
                    if act:
                        a = dev.get(c.a_out, np.uint16 if act == "bf16" else np.uint32)
                        rest_is_sentinel(a, M * D, "a_out")
                        worst = max(worst, check_bounded(act_values(a[:M * D], act == "bf16").reshape(M, D), a_ref, e_a, 2.0 ** -8 if act == "bf16" else 2.0 ** -23, "a_out"))
    print(f"k_post M {M} splits {splits}: worst |got - ref| / bound = {worst:.3f}")


def test_post_constant_row_gives_the_bias():
    """a constant row has variance 0: its LayerNorm is the bias, exactly"""
    takes("k_post", "k_post")
    s = PostSetup(3, 0)
    x = s.x.copy()
    x[1] = 3.0
    with Dev() as dev:
        c = _no_handles(PostCase())
        c.x, c.M, c.splits, c.ln_out = dev.up(x), 3, 0, 0
        c.ln2_w, c.ln2_b, c.act_bf16, c.a_out = dev.up(s.ln[1][0]), dev.up(s.ln[1][1]), 0, dev.new(3 * D * 4)
        assert dev.L.layer_harness_post(C.byref(c)) == 0, dev.err()
        a = dev.get(c.a_out, np.float32)[:3 * D].reshape(3, D)
    assert np.array_equal(a[1], s.ln[1][1])


# ---- PRO_LN --------------------------------------------------------------------------------------------------------------------------------------
def ln_weight(N):
    """W[n][k] = (k == n % 1024): output column n is panel column n % 1024, exactly"""
    W = np.zeros((N, D), np.float32)
    W[np.arange(N), np.arange(N) % D] = 1.0
    return W


class LnSetup:
    def __init__(self, M, part_splits, lno, epi, seed=0, scale=1.0):
        self.post = PostSetup(M, part_splits, seed=seed * 7 + lno * 3 + epi, scale=scale)
        self.M, self.part_splits, self.lno, self.epi = M, part_splits, lno, epi
        self.N = {R.EPI_SILU_ACT: 4096, R.EPI_GLU: 2048, R.EPI_QKV: 3072}[epi]
        # EPI_QKV: rows m -> stream m / T; two streams where M allows, one of them wrapping inside its chunk
        self.T = M // 2 if (epi == R.EPI_QKV and M % 2 == 0) else M
        nb = M // self.T
        self.slots, self.n_slots = [2, 0][:nb], 3
        self.head = [KVC - LCTX - self.T // 2, 17][:nb]                     # kv_head + 70 + row passes KVC inside the first stream's rows

    def problem(self, dev):
        p, M = self.post, self.M
        c = _no_handles(FusedCase())
        c.pro, c.M, c.N, c.K, c.splits, c.epi, c.T = PRO_LN, M, self.N, D, 1, self.epi, self.T
        c.W = dev.packed(ln_weight(self.N))
        c.x_in, c.x_out = dev.up(p.x, slack_rows(M) * D * 4), dev.new((M + slack_rows(M)) * D * 4)
        if self.part_splits:
            c.part, c.part_splits, c.scale = dev.up(p.part), self.part_splits, p.scale
        if self.lno:
            c.lno_w, c.lno_b = dev.up(p.ln[0][0]), dev.up(p.ln[0][1])
        c.ln_w, c.ln_b = dev.up(p.ln[1][0]), dev.up(p.ln[1][1])
        if self.epi == R.EPI_SILU_ACT:
            c.ldo_act, c.out_act = self.N, dev.new(M * self.N * 2)
        elif self.epi == R.EPI_GLU:
            c.ldo, c.out_f32 = self.N // 2, dev.new(M * self.N // 2 * 4)
        else:
            c.q_out, c.kv_pool, c.n_slots = dev.new((M + slack_rows(M)) * D * 4), dev.new(self.n_slots * 2 * KVC * D * 2), self.n_slots
            c.rows = dev.up(row_descs(self.slots, head=self.head))
        return c

    def outputs(self, c):
        return [h for h in (c.x_out, c.out_act, c.out_f32, c.q_out, c.kv_pool) if h >= 0]

    def check(self, dev, c):
        p, M, N = self.post, self.M, self.N
        x_ref, e_x, a_ref, e_a = p.reference(self.lno, True)
        x = dev.get(c.x_out, np.float32)
        rest_is_sentinel(x, M * D, "x_out")
        worst = check_bounded(x[:M * D].reshape(M, D), x_ref, e_x, 2.0 ** -23, "x_out")
        e_panel = e_a + 2.0 ** -8 * np.abs(a_ref)                                        # the bf16 panel
        col = np.arange(N) % D
        if self.epi == R.EPI_SILU_ACT:
            out = dev.get(c.out_act, np.uint16)
            rest_is_sentinel(out, M * N, "out_act")
            ref = R.silu(a_ref)[:, col]
            worst = max(worst, check_bounded(R.bf16_to_f32(out[:M * N]).reshape(M, N), ref, (1.1 * e_panel)[:, col] + EXPF_REL * np.abs(ref), 2.0 ** -8, "silu"))
        elif self.epi == R.EPI_GLU:
            out = dev.get(c.out_f32, np.float32)
            rest_is_sentinel(out, M * N // 2, "out_f32")
            acc = a_ref[:, col]
            ref = R.glu(acc)
            worst = max(worst, check_bounded(out[:M * N // 2].reshape(M, N // 2), ref, R.epilogue_bound(R.EPI_GLU, acc, e_panel[:, col]) + EXPF_REL * np.abs(ref), 2.0 ** -23, "glu"))
        else:
            q = dev.get(c.q_out, np.float32)
            rest_is_sentinel(q, M * D, "q_out")
            q = q[:M * D].reshape(M, D)
            worst = max(worst, check_bounded(q, a_ref, e_panel, 0.0, "q"))
            assert np.array_equal(R.bf16_round(q), q)
            pool = dev.get(c.kv_pool, np.uint16)
            n = self.n_slots * 2 * KVC * D
            rest_is_sentinel(pool, n, "kv_pool")
            want = np.full((self.n_slots, 2, KVC, D), SENT, np.uint16)
            slot, ring = R.kv_index(M, self.T, self.slots, self.head)                    # ring row kv_head + 70 + frame, mod KVC
            if self.T >= 2 and M // self.T == 2:
                assert ring[:self.T].min() == 0 and ring[:self.T].max() == KVC - 1, "the first stream's rows wrap"
            for m in range(M):
                want[slot[m], 0, ring[m]] = want[slot[m], 1, ring[m]] = R.bf16_bits(q[m])
            assert np.array_equal(pool[:n].reshape(want.shape), want), "K / V ring rows: not the normalised rows at kv_head + 70 + row, or something else was written"
        return worst


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 16])
@pytest.mark.parametrize("epi", [R.EPI_SILU_ACT, R.EPI_GLU, R.EPI_QKV], ids=["SILU", "GLU", "QKV"])
def test_fused_ln(M, epi):
    mmax = 1 if M == 1 else 2 if M == 2 else 16
    takes(fused_kernel(PRO_LN, M, D, 1), f"k_fused_skinny<PRO_LN,{mmax}>")
    worst = 0.0
    for part_splits in (0, 4, 8):
        for lno in (0, 1):
            s = LnSetup(M, part_splits, lno, epi)
            with Dev() as dev:
                c = s.problem(dev)
                run_fused(dev, c)
                worst = max(worst, s.check(dev, c))
    print(f"fused PRO_LN M {M} epi {R.EPI_NAMES[epi]}: worst |got - ref| / bound = {worst:.3f}")


# ---- rows of tiny variance: eps decides the output --------------------------------------------------------------------------------------------------
TINY = 10.0 ** -2.5          # rows ~ TINY N(0, 1): variance 1e-5 = eps, so 1 / sqrt(var + eps) is 0.71 / sd and any other eps (1e-6: 0.95 / sd) is far outside the bound


def test_layer_norm_eps_on_rows_of_tiny_variance():
    """every LayerNorm body -- ln4 (k_post, k_dwconv), k_dwconv_stream's own, block_ln and wave_ln (the fused prologues at M <= 2 and above) -- on rows whose
    variance is about eps = 1e-5, against the same analytic bound as everywhere else (f32 outputs where the kernel has them: the bound is then ~1e-4 of the output)"""
    takes("k_post", "k_post")
    s = PostSetup(3, 0, seed=5, scale=TINY)
    assert 0.5e-5 < float(s.x.astype(np.float64).var(-1).min()) and float(s.x.astype(np.float64).var(-1).max()) < 2e-5
    _, _, a_ref, e_a = s.reference(0, True)
    with Dev() as dev:
        c = _no_handles(PostCase())
        c.x, c.M, c.splits, c.ln_out = dev.up(s.x), 3, 0, 0
        c.ln2_w, c.ln2_b, c.act_bf16, c.a_out = dev.up(s.ln[1][0]), dev.up(s.ln[1][1]), 0, dev.new(3 * D * 4)
        assert dev.L.layer_harness_post(C.byref(c)) == 0, dev.err()
        a = dev.get(c.a_out, np.float32)[:3 * D].reshape(3, D)
    assert float(np.median(e_a / np.abs(a_ref))) < 1e-3, "the bound is tight here"
    print(f"tiny variance k_post: {check_bounded(a, a_ref, e_a, 2.0 ** -23, 'k_post'):.3f}")
    for B, T, stream_form, kernel in ((3, 7, 0, "k_dwconv"), (256, 7, 1, "k_dwconv_stream<7>")):
        takes(dwconv_kernel(stream_form, 9, T, B), kernel)
        cs = ConvSetup(B, T, 9, seed=11, scale=TINY)
        ref, bound, caches = cs.reference()
        with Dev() as dev:
            got, h_pool = run_dwconv(dev, cs, False, stream_form)
            cs.check_pool(dev, h_pool, caches)
        print(f"tiny variance {kernel}: {check_bounded(got, ref, bound, 2.0 ** -23, kernel):.3f}")
    for M, mmax in ((1, 1), (2, 2), (3, 16)):
        takes(fused_kernel(PRO_LN, M, D, 1), f"k_fused_skinny<PRO_LN,{mmax}>")
        for lno in (0, 1):                                                   # lno: the first LayerNorm sees the tiny rows, the second its output
            ls = LnSetup(M, 0, lno, R.EPI_QKV, seed=3, scale=TINY)
            with Dev() as dev:
                c = ls.problem(dev)
                run_fused(dev, c)
                print(f"tiny variance fused PRO_LN M {M} lno {lno}: {ls.check(dev, c):.3f}")
        takes(fused_kernel(PRO_DWCONV, M, D, 4), f"k_fused_skinny<PRO_DWCONV,{mmax}>")
        cs = ConvSetup(M, 1, 9, seed=13, scale=TINY)
        ref, bound, caches = cs.reference()
        with Dev() as dev:
            c = fused_conv_problem(dev, cs, 4)
            run_fused(dev, c)
            got = fused_panel(dev, c.out_f32, M, 4)
            cs.check_pool(dev, c.cv.cc_pool, caches)
        print(f"tiny variance fused PRO_DWCONV M {M}: {check_bounded(got, ref, bound, 2.0 ** -8, 'fused dwconv'):.3f}")


# ==== the fused GEMM body: PRO_PLAIN, exact integers ================================================================================================
@pytest.mark.parametrize("N,K,splits", [(1024, 4096, 4), (1024, 1024, 4), (128, 1024, 1)])
@pytest.mark.parametrize("M", [1, 2, 3, 15, 16])
def test_fused_plain_exact(M, N, K, splits):
    mmax = 1 if M == 1 else 2 if M == 2 else 16
    takes(fused_kernel(PRO_PLAIN, M, K, splits), f"k_fused_skinny<PRO_PLAIN,{mmax}>")
    assert K // splits <= 1024
    rng = rng_of("plain", M, N, K, splits)
    A, W = rng.integers(-3, 4, (M, K)).astype(np.float32), rng.integers(-3, 4, (N, K)).astype(np.float32)
    want = R.product_slices(A, W, R.k_slice_bounds(K, splits, 32)).astype(np.float32)          # integers below 9 x 4096 < 2^24: exact in any order
    with Dev() as dev:
        c = _no_handles(FusedCase())
        c.pro, c.M, c.N, c.K, c.splits, c.epi, c.ldo, c.lda, c.T = PRO_PLAIN, M, N, K, splits, R.EPI_PART_F32, N, K, 1
        c.A, c.W = dev.bf16_of(A, slack_rows(M) * K * 4), dev.packed(W)
        c.out_f32 = dev.new(splits * M * N * 4)
        run_fused(dev, c)
        out = dev.get(c.out_f32, np.float32)
    rest_is_sentinel(out, splits * M * N, "out_f32")
    assert np.array_equal(out[:splits * M * N].reshape(splits, M, N), want)


# ==== grouped launches ===============================================================================================================================
def _group_problem(kind, M, seed, dev):
    """-> (FusedCase, output handles); M = 1: one stream, M = 2: two streams of one row"""
    if kind == PRO_LN:
        s = LnSetup(M, 4, 1, R.EPI_QKV, seed=seed)
        c = s.problem(dev)
        return c, s.outputs(c)
    if kind == PRO_ATTN:
        s = AttnSetup(M, 1, 1, rot=seed)
        q, Kv, Vv, P, bu, bv, _, _ = bounded_case(s, True, "row1")
        c, h = fused_attn_problem(dev, s, q + np.float32(0.01 * seed), Kv, Vv, P, bu, bv)
        return c, [h]
    s = ConvSetup(M, 1, 9, seed=seed)
    c = fused_conv_problem(dev, s, 4)
    return c, [c.out_f32, c.cv.cc_pool]


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("kind", [PRO_LN, PRO_ATTN, PRO_DWCONV], ids=["PRO_LN", "PRO_ATTN", "PRO_DWCONV"])
def test_fused_group(kind, M):
    splits = {PRO_LN: 1, PRO_ATTN: NH, PRO_DWCONV: 4}[kind]
    takes(fused_kernel(kind, M, D, splits, grouped=True), f"k_fused_skinny_grp<{PRO_NAMES[kind]},{M}>")
    with Dev() as dev:
        single = []
        for seed in (0, 2):
            c, outs = _group_problem(kind, M, seed, dev)
            run_fused(dev, c)
            single.append([dev.raw(h) for h in outs])
        cases, outs = zip(*[_group_problem(kind, M, seed, dev) for seed in (0, 1, 2)])
        cases[1].M = 0                                                       # a stage of the pipeline that holds no step
        run_fused(dev, list(cases), n=3, grouped=1)
        for i, want in ((0, single[0]), (2, single[1])):
            for h, w in zip(outs[i], want):
                assert np.array_equal(dev.raw(h), w), f"problem {i}: the grouped launch and the single launch differ"
        for h in outs[1]:
            raw = dev.raw(h)
            if kind == PRO_DWCONV and h == cases[1].cv.cc_pool:               # its conv-cache pool: the inputs, nothing written
                fresh = dev.raw(_group_problem(kind, M, 1, dev)[1][1])
                assert np.array_equal(raw, fresh), "the skipped problem's conv cache was written"
            else:
                assert np.all(raw == SENT), "the skipped problem's outputs were written"


def test_harness_refuses_shapes_the_kernels_do_not_cover():
    """a shape outside the kernels' indexing is an error of the harness, never a launch"""
    with Dev() as dev:
        a = _no_handles(AttnCase())
        for T, TS in ((15, 15), (14, 266), (2, 3)):
            a.B, a.T, a.TS, a.ctx_out = 1, T, TS, dev.new(256)
            assert dev.L.layer_harness_attention(C.byref(a)) == -1 and "attention" in dev.err()
        cv = _no_handles(ConvCase())
        for ks, T in ((33, 1), (1, 1), (9, 257)):
            cv.B, cv.T, cv.ks, cv.c_out = 1, T, ks, dev.new(256)
            assert dev.L.layer_harness_dwconv(C.byref(cv)) == -1 and "dwconv" in dev.err()
        for M, N, K, splits in ((17, 1024, 1024, 4), (1, 1000, 1024, 4), (1, 1024, 4096, 2), (1, 1024, 1024, 3)):
            f = _no_handles(FusedCase())
            f.pro, f.M, f.N, f.K, f.splits, f.epi, f.ldo, f.lda = PRO_PLAIN, M, N, K, splits, R.EPI_PART_F32, N, K
            assert dev.L.layer_harness_fused(C.byref(f), 1, 0) == -1 and "fused" in dev.err()
        f = _no_handles(FusedCase())                                         # buffers too small for the shape
        f.pro, f.M, f.N, f.K, f.splits, f.epi, f.ldo, f.lda = PRO_PLAIN, 2, 1024, 1024, 4, R.EPI_PART_F32, 1024, 1024
        f.W, f.A, f.out_f32 = dev.new(1024 * 1024 * 2), dev.new(2 * 1024 * 2), dev.new(4 * 1024 * 4)
        assert dev.L.layer_harness_fused(C.byref(f), 1, 0) == -1 and "out_f32" in dev.err()


def planned_kernels():
    """the kernel every case of this file is there for, by the launchers' rules"""
    out = {"k_post"}
    out |= {attention_kernel(bf16, T, TS) for _, bf16, _, T, TS in ATTN_CASES}
    out |= {fused_kernel(PRO_ATTN, B * T * G, D, NH) for B, T, G, _ in FUSED_ATTN}
    out |= {dwconv_kernel(0, ks, T, 3) for ks in (9, 5, 32) for T in (1, 2, 7, 14, 28)} | {dwconv_kernel(1, 9, T, 256) for T in (7, 14, 21)}
    out |= {fused_kernel(PRO_DWCONV, B * T, D, splits) for B, T, splits, _ in FUSED_CONV}
    out |= {fused_kernel(PRO_LN, M, D, 1) for M in (1, 2, 3, 4, 5, 16)} | {fused_kernel(PRO_PLAIN, M, K, s) for M in (1, 2, 3, 15, 16) for K, s in ((4096, 4), (1024, 4), (1024, 1))}
    out |= {fused_kernel(kind, M, D, s, grouped=True) for kind, s in ((PRO_LN, 1), (PRO_ATTN, NH), (PRO_DWCONV, 4)) for M in (1, 2)}
    return out


def test_every_kernel_is_reached():
    """every kernel of KERNELS is the one some case above asserts as taken; k_attention<true> is unreached (UNREACHED says why)"""
    planned = planned_kernels()
    assert sorted(planned) == sorted(KERNELS), (sorted(set(KERNELS) - planned), sorted(planned - set(KERNELS)))
    assert not set(UNREACHED) & planned
