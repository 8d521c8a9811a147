"""Every kernel of kernels_decode.hip, alone, against a float64 reference of the operation (tests/decode_ref.py).

tests/helpers/decode_harness.hip makes ONE call of a product launcher (launch_encproj, launch_decode_begin, launch_decode_candidates, launch_decode_iter,
launch_decode_rows, launch_decode_rows_boost, launch_lm_rows) on buffers [guard | body | guard] whose every byte that is not an input is the sentinel
0xFFC5 (NaN as f32), and returns every buffer whole.  The buffer plumbing (Dev, check_inputs, GUARD, SENT) is tests/test_gpu_layer_kernels.py's.  Weights go
through the product's own packer nasr_eng::pack_f32_mfma, resolved from the product library: packer and kernel are tested as a pair against the plain
row-major matrix.  The cases -- layouts, operands, poison, expectations, the terms of the bounds -- are numpy only and live in tests/decode_kernel_cases.py,
where tests/test_decode_kernel_ref.py checks them without a GPU.

One kernel at a time.  Every decode kernel exits on an empty work list, so planting the three device counters runs each alone through the launchers:
  launch_decode_candidates, dlist and n_dirty planted             k_dec_lstm<0>, k_dec_lstm<1>, k_dec_pred<false> only
  launch_decode_iter, n_dirty = 0, n_active = 0, n_rows = nr      the joint alone: k_dec_commit returns at *n_active == 0, so key and every scratch survive
  launch_decode_iter, n_dirty = 0, n_rows = 0, n_active = B       the commit alone, on keys, parts and lists the test planted
  launch_decode_iter, n_dirty = nd, n_rows = 0, n_active = 0      with lm_row: the candidates and the bias-row refresh (k_dec_pred<true> / k_dec_lmrows)
and the tests assert it: in a joint-alone call h, c, predg, ctrl, the lists and the rings come back bit for bit, likewise for the other kinds.
(In a commit-alone call n_rows = 0 also skips the FB variant's fb_row pass, so fb_row is planted there; the chained cases run that pass.)

Poison is values, never indices: every slot, prev_token, cur, automaton / LM state, dlist and rowmap entry a kernel may read is in range, the entries only
the clamped lanes read included (the harness refuses anything else before it launches).  The slot pool is larger than B, rows[b].slot a permutation into it,
unused slots hold the sentinel; dlist is a permutation; encproj rows of frames >= n_dec are the sentinel; every scratch starts as the sentinel and rows that
are not in rowmap must stay it.  After every call: every byte the call does not own is bit for bit what was uploaded, read-only buffers and guards included.

Exact mode (`==`).  Joint: encproj and predg small integers (e + g negative on half the k), out_w in {-2..2}, out_b integer: every partial sum is an
integer below 2^24 in any order, each logit ONE integer, each row and each slot's g with a pattern of its own.  Bit for bit: key = pack_key(max, first index
of the max), every part's m, every ALT list, boost_raw, raw_logits with its padding (columns 1025 .. 1039 = out_b[0]: the packed rows past the vocabulary
are 0).  Ten selector columns plant ties of the row maximum (decode_kernel_cases.TIES: one lane, xor-16, xor-32, two tiles / waves, two workgroups of the
tiled kernel, the borders 15|16, 63|64, 1023|1024, token 0 against blank, blank alone): the smaller index must win; bonus states 2 and 3 and every other LM
row turn the ties over.  LSTM: one-hot embed / h rows and weights in 512 Z make every pre-activation 0 (gate g), >= +32 (sigm is exactly 1) or <= -128
(expf overflows: exactly 0); c carries tags +-4 (2048 + index of (slot, version, layer, unit)), so c' in {c, c +- 1, 0, +-1} and h' in {0, +-1} are exact.
Three gates vary per (unit, k read) and one is held fixed, in turn (LSTM_CONFIGS), so that c' = +-1 never meets an open o gate.
The part's s and the entropy terms are sums of one sign of <= 64 terms through <= 6 exps and merges: relative S_REL = 6 EXPF + 80 u, ENT_REL = 8 EXPF + 90 u.

Bounded mode.  Operands random, rounded to f32, per element against decode_ref with u = 2^-24 (decode_kernel_cases: gate_bound, cell_bound, candidate_bounds,
logit_bound, encproj_case):
  gate sums (1280 + 8) u (|W_ih| |x| + |W_hh| |h| + |b_ih| + |b_hh|); through sigm: / 4 + SIGM_REL; through tanhf: x 1 + TANHF_REL; c', h' first order;
  layer 1 adds |W_ih1| e(h0'); predg (640 + 4) u (|W| |h1'| + |b|) + |W| e(h1'); encproj (K + 4) u (|W| |x| + |b|);
  logits (640 + 4) u (|W_out| x + |b|) + |W_out| (u |e + g|).
Every row has a planted winner whose float64 margin is >= 4 x the logit bound (asserted for every row on the CPU); lse of a part within delta + S_REL.
SIGM_REL, TANHF_REL, EXPF are not derived: test_device_libm measures 1 / (1 + expf(-x)), tanhf, expf on the device (the harness's k_libm) against float64 on a
grid over the range the cases reach; the constants are 4 x the recorded maxima (compilers differ by an ulp or two):
  sigm on [-30, 30]: 1.52e-7; tanhf on [-12, 12]: 1.32e-7; expf on [-80, 0]: 7.96e-8, 200001 points each    (MEASURED_* below, profiles/decode_kernels.md)
EXPF_REL of tests/test_gpu_gemm_kernels.py is __expf's, the fast form the GEMM epilogues call, and does not apply to expf.  No tolerance is measured on a
decode kernel.  Values derived from PLANTED parts (commit alone) are held to the bounds the header tests state: 5e-6 (test_logprob_math, test_topk_math),
2e-6 (test_entropy_math, test_frame_blank_math).

k_dec_joint at 64 rows and T = 14 does not exist (B T <= 64 gives at most 56 rows): 64 runs as B = 64, T = 1 and as B = 4, T = 16."""
from __future__ import annotations

import ctypes as C
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi
from tests import decode_kernel_cases as K
from tests import decode_ref as DR
from tests.decode_kernel_cases import PLAIN, RICH, RICH_LMF, U24, form_id, rng_of, sent
from tests.decode_ref import BLANK, COLS, CT, DEC_CTRL, HID, JNT, VOCAB
from tests.test_gpu_layer_kernels import GUARD, SENT, Dev

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HELPER = ROOT / "tests" / "helpers" / "libdecode_harness.so"
SOURCE = ROOT / "nemotron-asr.cpp_amd" / "csrc" / "kernels_decode.hip"
CALL_BEGIN, CALL_CANDIDATES, CALL_ITER, CALL_ROWS, CALL_ROWS_BOOST = range(5)

MEASURED_SIGM, MEASURED_TANHF, MEASURED_EXPF = 1.52e-7, 1.32e-7, 7.96e-8      # max relative deviation of the device libm from float64 (test_device_libm)
SIGM_REL, TANHF_REL, EXPF = 4 * MEASURED_SIGM, 4 * MEASURED_TANHF, 4 * MEASURED_EXPF
S_REL, ENT_REL = 6 * EXPF + 80 * U24, 8 * EXPF + 90 * U24
LP_BOUND, ENT_BOUND, FB_BOUND = 5e-6, 2e-6, 2e-6

FRACTIONS = {}            # kernel -> largest observed |got - ref| / bound


# ---- the harness -----------------------------------------------------------------------------------------------------------------------------
HANDLES = ("rows", "ctrl", "h", "c", "encproj", "embed", "w_ih0", "w_ih1", "w_hh0", "w_hh1", "b_ih0", "b_ih1", "b_hh0", "b_hh1", "pred_w", "pred_b", "out_w", "out_b",
           "predg", "key", "counters", "dlist", "rowmap", "tok_ring", "tok_frame", "lp_part", "tok_logprob", "boost_bonus", "boost_next", "boost_state", "boost_raw",
           "raw_logits", "alt_key", "alt_id", "alt_lp", "fb_row", "frame_blank", "lm_blk", "lm_state", "lm_row", "lm_next", "ent_part", "tok_entropy")
READ_ONLY = ("rows", "encproj", "boost_bonus", "boost_next", "lm_blk")
WEIGHTS = ("embed", "w_ih0", "w_ih1", "w_hh0", "w_hh1", "b_ih0", "b_ih1", "b_hh0", "b_hh1", "pred_w", "pred_b", "out_w", "out_b")


def _ints(*names):
    return [(n, C.c_int) for n in names]


class DecCase(C.Structure):
    _fields_ = _ints("rows", "B", "T", "n_slots", "ctrl", "h", "c", "encproj", "embed", "w_ih0", "w_ih1", "w_hh0", "w_hh1", "b_ih0", "b_ih1", "b_hh0", "b_hh1",
                     "pred_w", "pred_b", "out_w", "out_b", "predg", "key", "counters", "dlist", "rowmap", "tok_ring", "tok_frame", "lp_part", "tok_logprob",
                     "boost_bonus", "boost_next", "boost_state", "n_states", "boost_raw", "raw_logits", "alt_key", "alt_id", "alt_lp", "alt_k", "fb_row", "frame_blank",
                     "lm_blk", "lm_state", "lm_row", "lm_next", "lm_fold", "lm_relook", "lm_states", "ent_part", "tok_entropy") + [("ent_alpha", C.c_float)]


class LmCase(C.Structure):
    _fields_ = _ints("blk", "states", "uni", "arcs", "n_arcs", "n_states", "order", "max_probe", "start", "attached") + [("weight", C.c_float), ("token_bonus", C.c_float)]


@lru_cache(maxsize=None)
def harness():
    if not HELPER.exists():
        pytest.fail("tests/helpers/libdecode_harness.so not built: __graft_entry__.build() warns when the helper fails to compile (a changed DecParams or launcher of "
                    "kernels_decode.hip?); these tests do not skip")
    C.CDLL(str(capi.LIB_PATH), mode=C.RTLD_GLOBAL)          # the helper's undefined nasr:: symbols resolve against the product library
    L = C.CDLL(str(HELPER))
    L.decode_harness_error.restype = C.c_char_p
    L.decode_harness_alloc.argtypes = [C.c_longlong, C.c_int]
    L.decode_harness_total_bytes.restype = C.c_longlong
    L.decode_harness_put.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_longlong]
    L.decode_harness_get.argtypes = [C.c_int, C.c_void_p]
    assert [L.decode_harness_struct_bytes(i) for i in range(9)] == [C.sizeof(DecCase), C.sizeof(LmCase), 4 * len(DEC_CTRL), 32, 8, 72, 8, 8, 16]
    assert L.decode_harness_sentinel() == SENT
    assert [L.decode_harness_constant(i) for i in range(14)] == [1024, HID, JNT, VOCAB, BLANK, DR.TOK_CAP, DR.FRAME_CAP, DR.MAX_SYMBOLS, DR.SMALL_ROWS, DR.TILE_PARTS,
                                                                  DR.WG_PARTS, COLS, COLS, 8]
    return L


class Session:
    """one Dev for the module: the weight sets stay on the device, what a test allocates is freed when its scope ends"""

    def __init__(self):
        self.d = Dev(harness(), "decode_harness")
        self.L = self.d.L
        self.wsets = {}

    def close(self):
        self.d.fn("free_all")()

    def weights(self, name):
        """the handles of a weight set, matrices packed by the product's packer from their row-major upload"""
        if name not in self.wsets:
            w = K.bounded_weights() if name == "bounded" else K.chain_weights(CHAIN_SEED) if name == "chain" else K.exact_weights(name)
            hs = {}
            for n in WEIGHTS:
                if w[n].ndim == 1 or n == "embed":
                    hs[n] = self.d.up(w[n])
                    continue
                N, Kd = w[n].shape
                src = self.d.up(w[n])
                dst = self.d.new((N + 15) // 16 * 16 * Kd * 4)
                assert self.L.decode_harness_pack(src, dst, N, Kd, int(n.startswith("w_"))) == 0, self.d.err()
                self.d.frozen[dst] = self.d.raw(dst)
                hs[n] = dst
            self.wsets[name] = (w, hs)
        return self.wsets[name]

    def scope(self, wname=None):
        return Scope(self, wname)


class Scope:
    def __init__(self, s, wname):
        self.s, self.d, self.L = s, s.d, s.L
        self.w, self.wh = s.weights(wname) if wname else ({}, {})

    def __enter__(self):
        self.mark = self.L.decode_harness_count()
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:                                  # every read-only buffer of the call, the weights included: bit for bit as uploaded
                for h, want in self.d.frozen.items():
                    if h >= self.mark or h in self.wh.values():
                        assert np.array_equal(self.d.raw(h), want), f"a launch wrote into read-only buffer {h}"
        finally:
            for h in [h for h in self.d.frozen if h >= self.mark]:
                del self.d.frozen[h]
            self.L.decode_harness_free_from(self.mark)

    def call(self, st, call, alt_k=0, alpha=0.0, lm_fold=0, n_states=0, lm_states=0):
        """upload the arrays of st that are buffers of the call, make the call, return every writable buffer as it came back"""
        c = DecCase()
        hs = {}
        for n in HANDLES:
            if n in self.wh:
                hs[n] = self.wh[n]
            elif n in st and isinstance(st[n], int):
                hs[n] = st[n]                                   # a handle made by the test (lm_blk)
            elif n in st:
                hs[n] = self.d.up(st[n], slack_bytes=512, written=n not in READ_ONLY)
            else:
                hs[n] = -1
            setattr(c, n, hs[n])
        c.B, c.T, c.n_slots, c.alt_k, c.ent_alpha, c.lm_fold, c.lm_relook = st["B"], st["T"], st["pool"], alt_k, alpha, lm_fold, 0
        c.n_states, c.lm_states = n_states, lm_states
        self.ok(self.L.decode_harness_call(C.byref(c), call))
        return self.fetch(st, hs)

    def ok(self, rc):
        """a refused case is a failed test; an error of the device itself ends the session: nothing more is started on a GPU that has faulted"""
        if rc != 0 and self.d.err().startswith(("hipDeviceSynchronize", "launch")):
            pytest.exit(f"the device reported an error, no further GPU test is run: {self.d.err()}", returncode=3)
        assert rc == 0, self.d.err()

    def fetch(self, st, hs):
        out = {}
        for n in HANDLES:
            if n in st and not isinstance(st[n], int) and n not in READ_ONLY and n not in self.wh:
                body = self.d.get(hs[n], np.uint8)
                assert np.all(body[st[n].nbytes:].view(np.uint16) == SENT), f"{n}: written behind its {st[n].nbytes} bytes"
                out[n] = body[:st[n].nbytes].view(st[n].dtype).reshape(st[n].shape).copy()
        return out

    def lm_block(self, attached=0, states=None, uni=None, weight=0.0, token_bonus=0.0):
        states = states if states is not None else np.zeros((1, 2), np.int32)
        uni = uni if uni is not None else np.zeros((1027, 2), np.int32)
        arcs = np.zeros(4, np.uint32)
        arcs[:2] = 0xffffffff                                   # one arc, EMPTY: every probe ends at once
        lc = LmCase(self.d.new(72), self.d.up(states), self.d.up(uni), self.d.up(arcs), 1, len(states), 1 if attached else 0, 1, 0, attached, weight, token_bonus)
        assert self.L.decode_harness_lm_block(C.byref(lc)) == 0, self.d.err()
        self.d.frozen[lc.blk] = self.d.raw(lc.blk)
        return lc.blk


@pytest.fixture(scope="module")
def sess():
    s = Session()
    yield s
    s.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def nz(a):
    """-0.0 -> +0.0 (0 x a negative number is -0.0 on either side; the sign of a zero is not what these tests are about); NaN payloads stay"""
    a = np.array(a, copy=True)
    if a.dtype.kind == "f":
        a[a == 0] = 0
    return a


def same(out, st, names, what):
    for n in names:
        if n in out:
            assert np.array_equal(bits(out[n]), bits(st[n])), f"{what}: {n} changed"


def within(got, ref, bound, kernel, what):
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), f"{what}: not finite"
    err = np.abs(got - ref)
    frac = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    FRACTIONS[kernel] = max(FRACTIONS.get(kernel, 0.0), frac)
    print(f"{what}: largest |got - ref| / bound = {frac:.3f}")
    assert frac <= 1.0, f"{what}: {frac:.3f} of the bound at {np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)}"


ALL_STATE = ("ctrl", "h", "c", "predg", "key", "counters", "dlist", "rowmap", "tok_ring", "tok_frame", "lp_part", "tok_logprob", "boost_state", "boost_raw", "raw_logits",
             "alt_key", "alt_id", "alt_lp", "fb_row", "frame_blank", "lm_state", "lm_row", "lm_next", "ent_part", "tok_entropy")


def but(*names):
    return [n for n in ALL_STATE if n not in names]


# ---- the device libm ---------------------------------------------------------------------------------------------------------------------------
def test_device_libm(sess):
    """1 / (1 + expf(-x)), tanhf(x), expf(x) as the device computes them, against float64, on the ranges the cases reach.  The recorded maxima
    (MEASURED_*) times 4 are the constants of the bounds; a device whose libm is worse than that fails here, not in a kernel test."""
    grids = (np.linspace(-30, 30, 200001), np.linspace(-12, 12, 200001), np.linspace(-80, 0, 200001))
    refs = (DR.sigm, np.tanh, np.exp)
    got = []
    with sess.scope() as sc:
        for which, (x, f) in enumerate(zip(grids, refs)):
            x32 = x.astype(np.float32)
            hx, hy = sc.d.up(x32), sc.d.new(x32.nbytes)
            sc.ok(sc.L.decode_harness_libm(hx, hy, x32.size, which))
            y = sc.d.get(hy, np.float32)[:x32.size].astype(np.float64)
            ref = f(x32.astype(np.float64))
            nz = ref != 0
            got.append(float((np.abs(y - ref)[nz] / np.abs(ref)[nz]).max()))
    print(f"device libm, max relative deviation from float64: sigm {got[0]:.3e}, tanhf {got[1]:.3e}, expf {got[2]:.3e}")
    assert got[0] <= SIGM_REL and got[1] <= TANHF_REL and got[2] <= EXPF, got


# ---- k_encproj -----------------------------------------------------------------------------------------------------------------------------------
ENCPROJ_CASES = [(M, 1024, 640) for M in K.ENCPROJ_M] + [(3, k, n) for k, n in K.ENCPROJ_SITES if (k, n) != (1024, 640)]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bounded"])
@pytest.mark.parametrize("M,Kd,N", ENCPROJ_CASES)
def test_encproj(sess, M, Kd, N, exact):
    x, W, b, ref, bound = K.encproj_case(M, Kd, N, exact)
    with sess.scope() as sc:
        d = sc.d
        src, dst = d.up(W), d.new(N * Kd * 4)
        assert sc.L.decode_harness_pack(src, dst, N, Kd, 0) == 0, d.err()
        d.frozen[dst] = d.raw(dst)
        hx, hb, ho = d.up(x, slack_bytes=4 * Kd * 4), d.up(b), d.new(M * N * 4 + 1024)      # four sentinel rows behind x: the clamped lanes read row M - 1, never these
        sc.ok(sc.L.decode_harness_encproj(hx, dst, hb, ho, M, Kd, N))
        body = d.get(ho, np.float32)
        assert np.all(body[M * N:].view(np.uint16) == SENT), "written behind the M rows"
        got = body[:M * N].reshape(M, N)
        if exact:
            assert np.array_equal(got, ref.astype(np.float32))
        else:
            within(got, ref, bound, "k_encproj", f"encproj M={M} K={Kd} N={N}")


# ---- candidates: k_dec_lstm<0>, k_dec_lstm<1>, k_dec_pred<false> ------------------------------------------------------------------------------------
def check_candidates(out, st, w, exact, what):
    s, cur, x0, h, c = K.candidate_inputs(st, w)
    want = {n: st[n].copy() for n in ("h", "c", "predg")}
    if exact:
        h2, c2, g, ok, _ = K.exact_candidates(w, x0, h, c)
        assert ok
        want["h"][s, cur ^ 1], want["c"][s, cur ^ 1], want["predg"][s] = h2, c2, g
        for n in ("c", "h", "predg"):
            ok = bits(nz(want[n])) == bits(nz(out[n]))
            assert ok.all(), f"{what}: {n} differs at flat bytes {np.flatnonzero(~ok)[:4].tolist()} ..."
    else:
        (rh, rc, rg), (eh, ec, eg) = K.candidate_bounds(w, x0, h, c, SIGM_REL, TANHF_REL)
        within(out["c"][s, cur ^ 1], rc, ec, "k_dec_lstm", what + " c'")
        within(out["h"][s, cur ^ 1], rh, eh, "k_dec_lstm", what + " h'")
        within(out["predg"][s], rg, eg, "k_dec_pred", what + " predg")
        for n, v in (("h", out["h"][s, cur ^ 1]), ("c", out["c"][s, cur ^ 1])):        # everything but the owned elements: bit for bit
            want[n][s, cur ^ 1] = v
        want["predg"][s] = out["predg"][s]
        same(out, want, ("h", "c", "predg"), what)
    same(out, st, but("h", "c", "predg"), what)


@pytest.mark.parametrize("mode", ["exact", "bounded"])
@pytest.mark.parametrize("nd", K.ND_SWEEP)
def test_candidates(sess, nd, mode):
    exact = mode == "exact"
    st = K.candidate_case(nd, exact)
    with sess.scope("g" if exact else "bounded") as sc:
        out = sc.call(st, CALL_CANDIDATES)
        check_candidates(out, st, sc.w, exact, f"candidates nd={nd}")


@pytest.mark.parametrize("cfg", [c for c in K.LSTM_CONFIGS if c != "g"])
def test_candidates_gate_roles(sess, cfg):
    """the fixed gate moves over i, f, g, o: with i closed and f open c' is c's tag, with o closed h' is 0, and a gate / accumulator-register mix-up cannot pass"""
    st = K.candidate_case(97, True, seed=cfg)
    with sess.scope(cfg) as sc:
        out = sc.call(st, CALL_CANDIDATES)
        check_candidates(out, st, sc.w, True, f"candidates, gate {cfg} fixed")


# ---- the joint kernels ----------------------------------------------------------------------------------------------------------------------------------
def add_options(st, form, parts, alt_k=8, beam=False):
    """the option buffers of a form, every scratch and ring the sentinel"""
    BT, pool = st["B"] * st["T"], st["pool"]
    st = dict(st)
    if not form.get("BOOST") or form.get("LMF"):
        for n in ("boost_bonus", "boost_next", "boost_state"):
            st.pop(n, None)
    if not form.get("LMF"):
        st.pop("lm_row", None)
    else:
        st["lm_state"] = np.zeros(pool, np.int32)
        st["lm_next"] = np.zeros((pool, COLS), np.int32)
    if beam:
        st.pop("boost_next", None)
    if form.get("LP"):
        st["lp_part"], st["tok_logprob"] = sent((BT, parts, 2)), sent((pool, DR.TOK_CAP))
        if form.get("BOOST") and not form.get("BEAMB"):
            st["boost_raw"] = sent((BT, parts))
    if form.get("BEAMB"):
        st["raw_logits"] = sent((BT, COLS))
    if form.get("ALT"):
        st["alt_key"] = sent((BT, parts, alt_k, 2)).view(np.uint64).reshape(BT, parts, alt_k)
        st["alt_id"], st["alt_lp"] = sent((pool, DR.TOK_CAP, alt_k), np.int32), sent((pool, DR.TOK_CAP, alt_k))
    if form.get("ENT"):
        st["ent_part"], st["tok_entropy"] = sent((BT, parts)), sent((pool, DR.TOK_CAP))
    if form.get("FB"):
        st["fb_row"], st["frame_blank"] = sent(BT), sent((pool, DR.FRAME_CAP))
    return st


def check_joint(out, st, w, form, parts, exact, alt_k, alpha, kernel, what, win=None):
    ki, n = st["ki"], st["n_rows"]
    L = K.joint_logits(st, w)
    bias = K.joint_bias(st, form)
    V = L if bias is None else L + bias
    rest = np.ones(st["B"] * st["T"], bool)
    rest[ki] = False
    want_key = st["key"].copy()
    slice_of = np.minimum(np.arange(VOCAB) // DR.part_width(parts), parts - 1)
    if exact:
        assert np.array_equal(L, np.round(L)) and np.abs(V).max() < 2 ** 24
        want_key[ki] = DR.pack_key(V.max(-1).astype(np.float32), DR.first_argmax(V))
        bad = np.flatnonzero(want_key != out["key"])
        assert bad.size == 0, f"{what}: key of rows {bad[:6].tolist()}: got index {DR.key_index(out['key'][bad[:6]]).tolist()}, want {DR.key_index(want_key[bad[:6]]).tolist()}"
        delta = np.zeros_like(L)
    else:
        delta = K.logit_bound(st, w) + (0 if bias is None else U24 * np.abs(V))
        got_idx = DR.key_index(out["key"][ki])
        assert np.array_equal(got_idx, win), f"{what}: arg-max of rows {np.flatnonzero(got_idx != win)[:6].tolist()}"
        within(DR.key_logit(out["key"][ki]), V[np.arange(n), win], delta[np.arange(n), win], kernel, what + " winning logit")
        assert np.array_equal(out["key"][rest], st["key"][rest]), f"{what}: keys of rows that are not in rowmap changed"
    dmax = delta.max(-1)
    if form.get("LP"):
        lp = out["lp_part"]
        assert np.all(lp[rest].view(np.uint16) == SENT), f"{what}: lp_part of rows that are not in rowmap written"
        m, s = DR.parts_of(L, parts)
        if exact:
            assert np.array_equal(lp[ki][..., 0], m.astype(np.float32)), f"{what}: a part's m"
        else:
            within(lp[ki][..., 0], m, np.repeat(dmax[:, None], parts, 1), kernel, what + " parts' m")
        assert np.all(lp[ki][..., 1] > 0)
        within(lp[ki][..., 0].astype(np.float64) + np.log(lp[ki][..., 1].astype(np.float64)), m + np.log(s), dmax[:, None] + S_REL + 0 * m, kernel, what + " parts' lse")
    if form.get("LP") and form.get("BOOST") and not form.get("BEAMB"):
        br = out["boost_raw"]
        assert np.all(br[rest].view(np.uint16) == SENT), f"{what}: boost_raw of rows that are not in rowmap written"
        for p in range(parts):
            cols = np.flatnonzero(slice_of == p)
            if exact:
                j = cols[DR.first_argmax(V[:, cols])]
                assert np.array_equal(br[ki, p], L[np.arange(n), j].astype(np.float32)), f"{what}: boost_raw of part {p}"
            else:                                               # the raw logit of an entry that wins the part by boosted key, up to the bound
                near = V[:, cols] >= V[:, cols].max(-1, keepdims=True) - 2 * dmax[:, None]
                hit = np.abs(br[ki, p][:, None].astype(np.float64) - L[:, cols]) <= delta[:, cols]
                assert np.all((near & hit).any(-1)), f"{what}: boost_raw of part {p}"
    if form.get("BEAMB"):
        rl = out["raw_logits"]
        assert np.all(rl[rest].view(np.uint16) == SENT), f"{what}: raw_logits of rows that are not in rowmap written"
        assert np.array_equal(rl[ki][:, VOCAB:], np.full((n, COLS - VOCAB), w["out_b"][0], np.float32)), f"{what}: the padding columns of raw_logits"
        if exact:
            assert np.array_equal(rl[ki][:, :VOCAB], L.astype(np.float32)), f"{what}: raw_logits"
        else:
            within(rl[ki][:, :VOCAB], L, K.logit_bound(st, w), kernel, what + " raw_logits")
    if form.get("ALT"):
        ak = out["alt_key"]
        assert np.all(ak[rest].view(np.uint16) == SENT), f"{what}: alt_key of rows that are not in rowmap written"
        src = V if form.get("BEAMB") else L
        if exact:
            assert np.array_equal(ak[ki], DR.top_keys(src.astype(np.float32), parts, alt_k)), f"{what}: the alternatives' lists"
        else:
            idx, val = DR.key_index(ak[ki]), DR.key_logit(ak[ki]).astype(np.float64)
            live = ak[ki] != 0
            ref_keys = DR.top_keys(src.astype(np.float32), parts, alt_k)
            assert np.array_equal(live, ref_keys != 0), f"{what}: a list's length"
            assert np.all((ak[ki][..., :-1] > ak[ki][..., 1:]) | ~live[..., 1:]), f"{what}: a list is not descending"
            rows = np.arange(n)[:, None, None]
            idc = np.where(live, idx, 0)
            assert np.all(~live | (slice_of[idc] == np.arange(parts)[None, :, None])), f"{what}: an alternative outside its slice"
            assert np.all(~live | (np.abs(val - src[rows, idc]) <= (delta + U24 * np.abs(src))[rows, idc])), f"{what}: an alternative's logit"
            ref = DR.key_logit(ref_keys).astype(np.float64)
            assert np.all(~live | (val >= ref - 2 * dmax[:, None, None] - 1e-6)), f"{what}: a list misses a larger entry"
    if form.get("ENT"):
        ep = out["ent_part"]
        assert np.all(ep[rest].view(np.uint16) == SENT), f"{what}: ent_part of rows that are not in rowmap written"
        ref = DR.ent_terms(L, parts, alpha)
        pd = DR.padded(L)[:, :parts * DR.part_width(parts)].reshape(n, parts, -1)
        d = np.where(np.isfinite(pd), pd - pd.max(-1, keepdims=True), -np.inf)
        with np.errstate(invalid="ignore"):
            e = np.where(np.isfinite(d), np.exp(d), 0.0)
            dz = np.where(np.isfinite(d), d, 0.0)
            mag, slope = ((e * np.abs(dz)).sum(-1), (e * (np.abs(1 + dz) + 0)).sum(-1)) if alpha == 1.0 else ((e ** alpha).sum(-1), alpha * (e ** alpha).sum(-1))
        within(ep[ki], ref, ENT_REL * mag + 2 * dmax[:, None] * slope + 1e-30, kernel, what + " entropy terms")
    same(out, st, but("key", "lp_part", "boost_raw", "raw_logits", "alt_key", "ent_part"), what)


def run_joint(sess, B, T, n_rows, form, exact, ragged=False, call=CALL_ITER, alt_k=8, alpha=1.0, seed=0):
    beam = call != CALL_ITER
    parts = DR.WG_PARTS if beam else DR.n_parts(B * T)
    kernel = K.joint_kernel(B * T, beam=beam, **{k: v for k, v in form.items() if k != "FB"})
    with sess.scope("g" if exact else "bounded") as sc:
        st = K.joint_case(B, T, n_rows, exact, seed=seed, ragged=ragged)
        win = None
        if not exact:
            win = K.plant_winners(st, sc.w, seed)
            L = K.joint_logits(st, sc.w)
            bias = K.joint_bias(st, form)
            V = L if bias is None else L + bias
            assert np.array_equal(DR.first_argmax(V), win) and np.all(K.margins(V) >= 4 * (K.logit_bound(st, sc.w).max(-1) + U24 * np.abs(V).max(-1)))
        full = add_options(st, form, parts, alt_k, beam)
        if form.get("LMF"):
            full["lm_blk"] = sc.lm_block()
        out = sc.call(full, call, alt_k=alt_k if form.get("ALT") else 0, alpha=alpha if form.get("ENT") else 0.0, n_states=4, lm_states=1)
        check_joint(out, full, sc.w, form, parts, exact, alt_k, alpha, kernel, f"{kernel} B={B} T={T} rows={n_rows}", win)
    return kernel


def small_layouts(n):
    out = [(n, 1, False)]
    if n <= 56:
        out.append((4 if n > 42 else 3 if n > 28 else 2 if n > 14 else 1 + (n < 14), 14, True))
    else:
        out.append((4, 16, False))
    return out


SWEEP_FORMS = [PLAIN, RICH, RICH_LMF]


@pytest.mark.parametrize("mode", ["exact", "bounded"])
@pytest.mark.parametrize("form", SWEEP_FORMS, ids=form_id)
@pytest.mark.parametrize("n_rows", K.SMALL_ROWS_SWEEP)
def test_joint_small_sweep(sess, n_rows, form, mode):
    for B, T, ragged in small_layouts(n_rows):
        assert B * T <= 64
        run_joint(sess, B, T, n_rows, form, mode == "exact", ragged=ragged, alt_k=1 if n_rows % 2 else 8, alpha=1.0 if n_rows % 3 else 2.0)


@pytest.mark.parametrize("mode", ["exact", "bounded"])
@pytest.mark.parametrize("form", SWEEP_FORMS, ids=form_id)
@pytest.mark.parametrize("n_rows", K.TILED_ROWS_SWEEP)
def test_joint_tiled_sweep(sess, n_rows, form, mode):
    run_joint(sess, 15, 14, n_rows, form, mode == "exact", ragged=True, alt_k=1 if n_rows % 2 else 8, alpha=1.0 if n_rows % 3 else 0.5)


@pytest.mark.parametrize("form", K.joint_forms(), ids=form_id)
@pytest.mark.parametrize("B,T,n_rows", [(5, 4, 17), (22, 4, 81)])
def test_joint_every_form_exact(sess, B, T, n_rows, form):
    REACHED.add(run_joint(sess, B, T, n_rows, form, True, alt_k=8, alpha=1.0))


@pytest.mark.parametrize("mode", ["exact", "bounded"])
@pytest.mark.parametrize("B,T,n_rows", [(5, 4, 17), (22, 4, 81)])
@pytest.mark.parametrize("boost", [False, True], ids=["rows", "rows_boost"])
def test_joint_beam_calls(sess, boost, B, T, n_rows, mode):
    """launch_decode_rows / launch_decode_rows_boost with n_dirty = 0: the tiled joint whatever the row count, 17 parts, no commit"""
    form = dict(LP=True, BOOST=boost, ALT=True, BEAMB=boost)
    REACHED.add(run_joint(sess, B, T, n_rows, form, mode == "exact", call=CALL_ROWS_BOOST if boost else CALL_ROWS, alt_k=8))


# ---- k_dec_begin ------------------------------------------------------------------------------------------------------------------------------------------
def ctrl_dicts(ctrl, slots):
    return [dict(zip(DEC_CTRL, (int(v) for v in ctrl[s]))) for s in slots]


def check_lists(out, ctrl_after, st, what):
    na, dl, rm = DR.build_lists(ctrl_after, st["slots"])
    assert out["counters"].tolist() == [na, len(dl), len(rm)], f"{what}: n_active, n_dirty, n_rows = {out['counters'].tolist()}, want {[na, len(dl), len(rm)]}"
    assert set(out["dlist"][:len(dl)].tolist()) == dl, f"{what}: dlist"
    assert set(out["rowmap"][:len(rm)].tolist()) == rm, f"{what}: rowmap"


@pytest.mark.parametrize("B,T", [(3, 4), (20, 4), (70, 5), (300, 2)])
def test_begin(sess, B, T):
    r = rng_of("begin", B, T)
    st = K.base_state(B, T, B + 3, "begin", n_dec=r.integers(0, T + 1, B).astype(np.int32))
    slots = st["slots"]
    st["ctrl"][slots, CT["dirty"]] = r.integers(0, 2, B)
    st["ctrl"][slots, CT["symbols"]] = r.integers(0, 10, B)
    st["ctrl"][slots, CT["t"]] = r.integers(0, T, B)
    st["key"] = r.integers(1, 2 ** 62, B * T).astype(np.uint64)
    with sess.scope("g") as sc:
        out = sc.call(st, CALL_BEGIN)
    want = st["ctrl"].copy()
    for b, s in enumerate(slots):
        nd = int(st["rows"][b, 5])
        w = want[s]
        w[CT["t"]], w[CT["n_frames"]], w[CT["symbols"]], w[CT["row"]], w[CT["active"]] = 0, nd, 0, b, int(nd > 0)
        w[CT["frame0"]] = st["ctrl"][s, CT["frame_next"]]
        w[CT["frame_next"]] = st["ctrl"][s, CT["frame_next"]] + nd
    assert np.array_equal(out["ctrl"], want)
    assert not out["key"].any()
    check_lists(out, want, st, f"begin B={B}")
    same(out, st, but("ctrl", "key", "counters", "dlist", "rowmap"), "begin")
    REACHED.add("k_dec_begin")


# ---- k_dec_commit alone -------------------------------------------------------------------------------------------------------------------------------------
def commit_streams(T):
    """(t0, n_frames, frame of the token or None, symbols, n_tok, frame0, active) of every stream of a commit-alone case"""
    last = T - 1
    return [dict(t=0, nf=T, tok_at=None, symbols=4),                          # all frames blank
            dict(t=1, nf=T, tok_at=1, symbols=3),                              # token on the first frame: symbols kept and counted on
            dict(t=0, nf=T, tok_at=2, symbols=5),                              # token on a middle frame: symbols reset when the frame moved
            dict(t=1, nf=T, tok_at=last, symbols=0),                           # token on the last frame
            dict(t=2, nf=T, tok_at=2, symbols=9),                              # the 10th symbol of a frame: the frame advances, symbols = 0
            dict(t=last, nf=T, tok_at=last, symbols=9),                        # ... of the last frame: the stream ends
            dict(t=0, nf=T, tok_at=1, symbols=9),                              # 9 symbols on an earlier frame do not count on the next one
            dict(t=1, nf=T, tok_at=2, symbols=2, active=0),                    # inactive: untouched
            dict(t=0, nf=T, tok_at=0, symbols=0, n_tok=4095),                  # the token rings wrap at 4096
            dict(t=0, nf=T, tok_at=1, symbols=0, n_tok=4096),
            dict(t=0, nf=T, tok_at=last, symbols=1, n_tok=8191),
            dict(t=0, nf=T, tok_at=last, symbols=0, frame0=3 * 4096 - 2),      # frame0 + f crosses a multiple of 4096 (the frame ring, tok_frame unmasked)
            dict(t=1, nf=3, tok_at=None, symbols=7),                           # ragged: n_frames < T
            dict(t=0, nf=0, tok_at=None, symbols=0, active=0)]                 # no frames this step


def commit_case(T, form, alt_k, alpha, seed=0):
    streams = commit_streams(T)
    B = len(streams)
    parts = DR.n_parts(B * T)
    r = rng_of("commit", T, form_id(form), seed)
    st = K.base_state(B, T, B + 3, ("commit", T, seed), n_dec=np.array([s["nf"] for s in streams], np.int32))
    slots = st["slots"]
    st = add_options(dict(st, boost_bonus=np.zeros((4, COLS), np.float32), boost_next=r.integers(0, 4, (4, COLS)).astype(np.int32),
                          boost_state=r.integers(0, 4, B + 3).astype(np.int32), lm_row=np.zeros((B + 3, COLS), np.float32)), form, parts, alt_k)
    if form.get("LMF"):
        st["lm_state"][:] = r.integers(0, 5, B + 3)
        st["lm_next"][:] = r.integers(0, 5, (B + 3, COLS))
        if r.integers(0, 2):
            st["boost_next"], st["boost_state"] = r.integers(0, 4, (4, COLS)).astype(np.int32), r.integers(0, 4, B + 3).astype(np.int32)     # lm_fusion with phrase_boost on too
    key = np.uint64(0x5555000000000000) + np.arange(B * T).astype(np.uint64)
    logits = (r.standard_normal((B * T, VOCAB)) * 3).astype(np.float32)
    best = np.full(B * T, BLANK)
    rowmap = []
    for b, s in enumerate(streams):
        ct = st["ctrl"][slots[b]]
        ct[CT["t"]], ct[CT["n_frames"]], ct[CT["symbols"]], ct[CT["active"]] = s["t"], s["nf"], s["symbols"], s.get("active", 1)
        ct[CT["dirty"]] = 0
        if "n_tok" in s:
            ct[CT["n_tok"]] = s["n_tok"]
        if "frame0" in s:
            ct[CT["frame0"]] = s["frame0"]
        if not s.get("active", 1):
            continue
        for f in range(s["t"], s["nf"]):
            ki = b * T + f
            rowmap.append((f << 16) | b)
            if s["tok_at"] is not None and f >= s["tok_at"] and (f == s["tok_at"] or r.integers(0, 2)):
                best[ki] = r.integers(0, BLANK)                 # frames behind the token may hold tokens too: they are not committed this iteration
            logits[ki, best[ki]] = logits[ki].max() + 2.0
            key[ki] = DR.pack_key(logits[ki, best[ki]] + (1.0 if form.get("BOOST") else 0.0), best[ki])      # with phrase_boost the key holds logit + bonus
    st["key"] = key
    st["rowmap"][:len(rowmap)] = r.permutation(np.array(rowmap, np.uint32))
    st["counters"][:] = (B, 0, 0)
    kis = np.array([(e & 0xffff) * T + (e >> 16) for e in rowmap])
    L32 = logits[kis]
    if form.get("LP"):
        m, s_ = DR.parts_of(L32.astype(np.float64), parts)
        st["lp_part"][kis] = np.stack([m, s_], -1).astype(np.float32)
        if form.get("BOOST"):
            pw = DR.part_width(parts)
            st["boost_raw"][kis, np.minimum(best[kis] // pw, parts - 1)] = L32[np.arange(len(kis)), best[kis]]
    if form.get("ALT"):
        st["alt_key"][kis] = DR.top_keys(L32, parts, alt_k)
    if form.get("ENT"):
        st["ent_part"][kis] = DR.ent_terms(L32.astype(np.float64), parts, alpha).astype(np.float32)
    if form.get("FB"):
        st["fb_row"][kis] = DR.log_softmax(L32.astype(np.float64))[:, BLANK].astype(np.float32)
    return st, streams, logits, best, parts


def expect_commit(st, streams, logits, best, parts, form, alt_k, alpha):
    """one commit per stream by the reference's rules (decode_ref.commit_stream); returns the expected buffers and the float64 values with their bounds"""
    T, slots = st["T"], st["slots"]
    want = {n: st[n].copy() for n in ALL_STATE if n in st}
    soft = []                                                   # (buffer, index, float64 value, bound)
    for b, s in enumerate(streams):
        slot = slots[b]
        ct = dict(zip(DEC_CTRL, (int(v) for v in st["ctrl"][slot])))
        if not ct["active"]:
            continue
        n = ct["n_tok"]
        tok, f, t0, t1 = DR.commit_stream(ct, lambda f: int(best[b * T + f]))
        want["ctrl"][slot] = [ct[k] for k in DEC_CTRL]
        want["key"][b * T + t0:b * T + s["nf"]] = 0             # the keys of [t0, n_frames) and no others
        if tok is not None:
            at = n & (DR.TOK_CAP - 1)
            want["tok_ring"][slot, at], want["tok_frame"][slot, at] = tok, ct["frame0"] + f
            row = logits[b * T + f].astype(np.float64)
            lsm = DR.log_softmax(row[None])[0]
            if form.get("LP"):
                soft.append(("tok_logprob", (slot, at), lsm[tok], LP_BOUND))
            if form.get("ALT"):
                order = np.argsort(-row, kind="stable")[:alt_k]
                want["alt_id"][slot, at] = order
                soft += [("alt_lp", (slot, at, j), lsm[v], LP_BOUND) for j, v in enumerate(order)]
            if form.get("ENT"):
                soft.append(("tok_entropy", (slot, at), DR.entropy(row[None], alpha)[0], ENT_BOUND))
            if form.get("LMF"):
                want["lm_state"][slot] = st["lm_next"][slot, tok]
            if form.get("BOOST") and "boost_next" in st:
                want["boost_state"][slot] = st["boost_next"][st["boost_state"][slot], tok]
        if form.get("FB"):
            for g in range(t0, t1):
                want["frame_blank"][slot, (ct["frame0"] + g) & (DR.FRAME_CAP - 1)] = st["fb_row"][b * T + g]
    return want, soft


COMMIT_FORMS = K.greedy_forms()


@pytest.mark.parametrize("T", [4, 6])
@pytest.mark.parametrize("form", COMMIT_FORMS, ids=form_id)
def test_commit_alone(sess, form, T):
    alt_k, alpha = (1 if T == 4 else 8), (1.0 if T == 4 else 2.0)
    st, streams, logits, best, parts = commit_case(T, form, alt_k, alpha)
    assert parts == (DR.TILE_PARTS if T == 4 else DR.WG_PARTS)
    kernel = K.commit_kernel(**form)
    with sess.scope("g") as sc:
        if form.get("LMF"):
            st["lm_blk"] = sc.lm_block()
        out = sc.call(st, CALL_ITER, alt_k=alt_k if form.get("ALT") else 0, alpha=alpha if form.get("ENT") else 0.0, n_states=4, lm_states=5)
    want, soft = expect_commit(st, streams, logits, best, parts, form, alt_k, alpha)
    what = f"{kernel} T={T}"
    for name, idx, val, bound in soft:                          # float64 from the planted parts, then the buffer bit for bit around them
        got = float(out[name][idx])
        assert np.isfinite(got) and abs(got - val) <= bound, f"{what}: {name}{idx} = {got}, float64 {val}"
        want[name][idx] = out[name][idx]
    check_lists(out, want["ctrl"], st, what)
    same(out, want, but("counters", "dlist", "rowmap"), what)
    REACHED.add(kernel)


# ---- the bias rows of "lm_fusion": k_lm_rows_slots, k_dec_lmrows, k_dec_pred<true> ----------------------------------------------------------------------------
def lm_model(seed=0):
    r = rng_of("lm", seed)
    states = np.zeros(5, np.dtype([("backoff", np.float32), ("back", np.int32)]))
    states["backoff"] = -r.random(5).astype(np.float32)
    uni = np.zeros(1027, np.dtype([("lp", np.float32), ("next", np.int32)]))
    uni["lp"], uni["next"] = -(r.random(1027) * 8).astype(np.float32), r.integers(0, 5, 1027)
    return states, uni, np.float32(0.5), np.float32(0.25)


def lm_rows_expected(states, uni, weight, bonus, lm_state, boost_row):
    """[COLS] bias row and next-state row of one slot by the definition of lmbias: (float)(weight * lp + token_bonus) in double, product and sum rounded on
    their own; lp = the back-off of a non-zero state (its one level finds no arc) + the unigram; blank, the padding and a disabled stream: 0, the state itself"""
    row, nxt = np.zeros(COLS, np.float32), np.full(COLS, lm_state, np.int32)
    if lm_state >= 0:
        lp = (np.float64(states["backoff"][lm_state]) if lm_state != 0 else 0.0) + uni["lp"][:1024].astype(np.float64)
        row[:1024] = (np.float64(weight) * lp + np.float64(bonus)).astype(np.float32)
        nxt[:1024] = uni["next"][:1024]
    return (boost_row + row).astype(np.float32) if boost_row is not None else row, nxt


@pytest.mark.parametrize("boost", [False, True], ids=["lm", "lm+boost"])
def test_lm_rows_slots(sess, boost):
    pool, slot0, n = 9, 2, 5
    states, uni, weight, bonus = lm_model()
    r = rng_of("lm rows", boost)
    st = dict(B=1, T=1, pool=pool, lm_state=r.integers(-1, 5, pool).astype(np.int32), lm_row=sent((pool, COLS)), lm_next=sent((pool, COLS), np.int32))
    if boost:
        st["boost_bonus"] = (r.integers(0, 4, (4, COLS)) * 0.5).astype(np.float32)
        st["boost_state"] = r.integers(0, 4, pool).astype(np.int32)
    with sess.scope() as sc:
        st["lm_blk"] = sc.lm_block(1, states.view(np.int32).reshape(-1, 2), uni.view(np.int32).reshape(-1, 2), weight, bonus)
        c, hs = DecCase(), {}
        for name in HANDLES:
            hs[name] = st[name] if isinstance(st.get(name), int) else sc.d.up(st[name], 512, written=name in ("lm_row", "lm_next")) if name in st else -1
            setattr(c, name, hs[name])
        c.n_slots, c.n_states, c.lm_states = pool, 4, 5
        sc.ok(sc.L.decode_harness_lm_rows(C.byref(c), slot0, n))
        out = sc.fetch({k: v for k, v in st.items() if k in ("lm_row", "lm_next")}, hs)
    want_row, want_next = st["lm_row"].copy(), st["lm_next"].copy()
    for s in range(slot0, slot0 + n):
        want_row[s], want_next[s] = lm_rows_expected(states, uni, weight, bonus, st["lm_state"][s], st["boost_bonus"][st["boost_state"][s]] if boost else None)
    assert np.array_equal(bits(out["lm_row"]), bits(want_row)) and np.array_equal(bits(out["lm_next"]), bits(want_next))
    REACHED.add("k_lm_rows_slots")


@pytest.mark.parametrize("boost", [False, True], ids=["lm", "lm+boost"])
@pytest.mark.parametrize("fold", [0, 1], ids=["k_dec_lmrows", "k_dec_pred<true>"])
def test_lm_rows_of_dirty_streams(sess, fold, boost):
    """launch_decode_iter with lm_row, n_dirty = 17, n_rows = 0, n_active = 0: the candidates of the dirty streams and, beside them, their bias rows"""
    states, uni, weight, bonus = lm_model(1)
    st = K.candidate_case(17, True, seed=("lm", fold, boost))
    r = rng_of("lm dirty", fold, boost)
    pool = st["pool"]
    st["counters"][0] = 0
    st.update(lm_state=r.integers(-1, 5, pool).astype(np.int32), lm_row=sent((pool, COLS)), lm_next=sent((pool, COLS), np.int32))
    st["lm_next"][st["slots"]] = 0                               # rows of the batch hold states (the harness checks what the commit could read)
    if boost:
        st["boost_bonus"], st["boost_state"] = (r.integers(0, 4, (4, COLS)) * 0.5).astype(np.float32), r.integers(0, 4, pool).astype(np.int32)
        st["boost_next"] = r.integers(0, 4, (4, COLS)).astype(np.int32)
    with sess.scope("g") as sc:
        st["lm_blk"] = sc.lm_block(1, states.view(np.int32).reshape(-1, 2), uni.view(np.int32).reshape(-1, 2), weight, bonus)
        out = sc.call(st, CALL_ITER, lm_fold=fold, n_states=4, lm_states=5)
        check_candidates({k: v for k, v in out.items() if k not in ("lm_row", "lm_next")}, {k: v for k, v in st.items() if k not in ("lm_row", "lm_next")}, sc.w, True,
                         f"candidates beside the bias rows, lm_fold={fold}")
    want_row, want_next = st["lm_row"].copy(), st["lm_next"].copy()
    for s in st["slots"][st["dirty"]]:
        want_row[s], want_next[s] = lm_rows_expected(states, uni, weight, bonus, st["lm_state"][s], st["boost_bonus"][st["boost_state"][s]] if boost else None)
    assert np.array_equal(bits(out["lm_row"]), bits(want_row)) and np.array_equal(bits(out["lm_next"]), bits(want_next))
    REACHED.update({"k_dec_pred<true>" if fold else "k_dec_lmrows", "k_dec_lstm<0>", "k_dec_lstm<1>", "k_dec_pred<false>"})


# ---- chained: begin, then iterations until no stream is active ----------------------------------------------------------------------------------------------
CHAIN_SEED = 2                # of decode_kernel_cases.chain_weights: chosen on the CPU, by the float64 trajectory alone, so that the margin condition holds


def chain_case(B, T, seed=0):
    r = rng_of("chain", B, T, seed)
    n_dec = r.integers(1, T + 1, B).astype(np.int32)
    n_dec[0] = T
    st = K.base_state(B, T, B + 3, ("chain", seed), n_dec=n_dec)
    slots = st["slots"]
    st["h"][slots] = r.uniform(-1, 1, (B, 2, 2, HID)).astype(np.float32)
    st["c"][slots] = r.uniform(-2, 2, (B, 2, 2, HID)).astype(np.float32)
    st["predg"][slots] = r.standard_normal((B, JNT)).astype(np.float32)
    st["ctrl"][slots, CT["dirty"]] = 1                          # a fresh stream: the candidate is stale
    st["ctrl"][slots, CT["symbols"]] = 0
    enc = sent((B, T, JNT))
    for b in range(B):
        enc[b, :n_dec[b]] = r.standard_normal((n_dec[b], JNT)).astype(np.float32)
    st["encproj"] = enc.reshape(B * T, JNT)
    return st


def chain_reference(st, w):
    """the per-stream greedy loop in float64 with, along the trajectory, the bound of every logit (the committed state's own error carried along) and
    the smallest margin / bound"""
    out = []
    worst = np.inf
    for b, slot in enumerate(st["slots"]):
        ct = dict(zip(DEC_CTRL, (int(v) for v in st["ctrl"][slot])))
        h, c = st["h"][slot, ct["cur"]].astype(np.float64), st["c"][slot, ct["cur"]].astype(np.float64)
        eh, ec = np.zeros((2, HID)), np.zeros((2, HID))
        enc = st["encproj"].reshape(st["B"], st["T"], JNT)[b]
        toks, frames, it, t, sym, prev, lps, fbs, dl = [], [], 0, 0, 0, ct["prev_token"], [], {}, []
        nf = int(st["rows"][b, 5])
        aw = DR.f64(w["out_w"], True)
        while t < nf:
            (h2, c2, g), (eh2, ec2, eg) = K.candidate_bounds(w, w["embed"][prev][None], h[None], c[None], SIGM_REL, TANHF_REL, eh[None], ec[None])
            e = enc[t].astype(np.float64)
            lg = DR.joint(e[None], g, w["out_w"], w["out_b"])[0]
            x = e + g[0]
            delta = (JNT + 4) * U24 * (aw @ np.maximum(x, 0) + np.abs(w["out_b"])) + aw @ (U24 * np.abs(x) + eg[0])
            s = np.sort(lg)
            worst = min(worst, (s[-1] - s[-2]) / delta.max())
            it += 1
            best = int(np.argmax(lg))
            fbs[t] = (DR.log_softmax(lg[None])[0, BLANK], delta.max())
            if best == BLANK:
                t, sym = t + 1, 0
                continue
            toks.append(best)
            frames.append(t)
            lps.append(DR.log_softmax(lg[None])[0, best])
            dl.append(delta.max())
            prev, h, c, eh, ec = best, h2[0], c2[0], eh2[0], ec2[0]
            sym += 1
            if sym >= DR.MAX_SYMBOLS:
                t, sym = t + 1, 0
        out.append(dict(toks=toks, frames=frames, it=it, prev=prev, sym=sym, h=h, c=c, eh=eh, ec=ec, lps=lps, fbs=fbs, dl=dl))
    return out, worst


@pytest.mark.parametrize("B,T", [(3, 4), (20, 4)])
def test_chained(sess, B, T):
    """launch_decode_begin, then launch_decode_iter until n_active is 0, in the LP + ALT + ENT + FB form: tokens, frames, iterations, prev_token, symbols bit for
    bit the float64 greedy loop's, committed h / c, ln P and the blank ring within the bounds carried along the trajectory"""
    form = dict(LP=True, BOOST=False, ALT=True, LMF=False, ENT=True, FB=True)
    st0 = chain_case(B, T)
    parts = DR.n_parts(B * T)
    with sess.scope("chain") as sc:
        ref, worst = chain_reference(st0, sc.w)
        assert worst >= 4.0, f"margin / bound along the reference trajectory: {worst}"
        st = add_options(st0, form, parts, 8)
        out = sc.call(st, CALL_BEGIN, alt_k=8, alpha=1.0)
        calls = 0
        while out["counters"][0] != 0:
            calls += 1
            assert calls <= 10 * T + 1, "the decode did not end within 10 T + 1 iterations"
            st = dict(st, **out)
            out = sc.call(st, CALL_ITER, alt_k=8, alpha=1.0)
    kernel = K.joint_kernel(B * T, **{k: v for k, v in form.items() if k != "FB"})
    for b, slot in enumerate(st0["slots"]):
        r_, ct0 = ref[b], dict(zip(DEC_CTRL, (int(v) for v in st0["ctrl"][slot])))
        ct = dict(zip(DEC_CTRL, (int(v) for v in out["ctrl"][slot])))
        n0, n = ct0["n_tok"], len(r_["toks"])
        at = (n0 + np.arange(n)) & (DR.TOK_CAP - 1)
        assert out["tok_ring"][slot, at].tolist() == r_["toks"], f"stream {b}: tokens"
        assert (out["tok_frame"][slot, at] - ct0["frame_next"]).tolist() == r_["frames"], f"stream {b}: frames"
        assert (ct["n_tok"], ct["iterations"] - ct0["iterations"], ct["prev_token"], ct["symbols"], ct["active"], ct["t"]) == (n0 + n, r_["it"], r_["prev"], r_["sym"], 0, ct["n_frames"]), f"stream {b}: control block"
        within(out["h"][slot, ct["cur"]], r_["h"], r_["eh"] + 1e-30, "chained", f"chained B={B} stream {b} committed h")
        within(out["c"][slot, ct["cur"]], r_["c"], r_["ec"] + 1e-30, "chained", f"chained B={B} stream {b} committed c")
        if n:
            within(out["tok_logprob"][slot, at], np.array(r_["lps"]), LP_BOUND + 2 * np.array(r_["dl"]), kernel, f"chained B={B} stream {b} ln P")
        fr = np.array(sorted(r_["fbs"]))
        within(out["frame_blank"][slot, (ct0["frame_next"] + fr) & (DR.FRAME_CAP - 1)], np.array([r_["fbs"][f][0] for f in fr]),
               FB_BOUND + 2 * np.array([r_["fbs"][f][1] for f in fr]), kernel, f"chained B={B} stream {b} ln P(blank)")
    REACHED.update({"k_dec_begin", kernel, K.commit_kernel(**form)})


# ---- every kernel is reached -------------------------------------------------------------------------------------------------------------------------------------
REACHED = set()
UNREACHED = {}            # kernel -> why no launcher takes it (none today)


def expected_kernels():
    """what the launchers of kernels_decode.hip can launch, from the rules restated in decode_kernel_cases (joint_kernel, commit_kernel)"""
    names = {"k_dec_begin", "k_dec_lstm<0>", "k_dec_lstm<1>", "k_dec_pred<false>", "k_dec_pred<true>", "k_dec_lmrows", "k_lm_rows_slots", "k_encproj",
             "k_dec_joint_tiled<true,false,true>", "k_dec_joint_tiled<true,true,true,true>"}
    for f in K.joint_forms():
        names |= {K.joint_kernel(17, **f), K.joint_kernel(81, **f)}
    for f in K.greedy_forms():
        names.add(K.commit_kernel(**f))
    return names


def test_every_decode_kernel_is_reached():
    """the __global__ functions of the source and the forms its launchers instantiate against the names the cases above are there for.  The forms come from
    following launch_decode_iter -> launch_joint_commit (template arguments, the ENT re-dispatch on ent_part, the FB commit on frame_blank)"""
    src = SOURCE.read_text()
    globs = set(re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", src))
    want = expected_kernels()
    assert globs == {n.split("<")[0] for n in want} | set(UNREACHED), globs
    # launch_joint_commit<LP, BOOST, ALT, LMF> instantiations in launch_decode_iter: each gives the form and its ENT twin (LP only), each with both commits (LP only)
    inst = set(re.findall(r"launch_joint_commit<([a-z, ]+)>\(p, st\);", src)) - {"LP, BOOST, ALT, LMF, true"}
    forms = set()
    for a in inst:
        v = [x.strip() == "true" for x in a.split(",")] + [False] * 2
        LP, BOOST, ALT, LMF = v[:4]
        for ENT in ((False, True) if LP else (False,)):
            forms.add((LP, BOOST, ALT, LMF, ENT))
    assert forms == {(f["LP"], f["BOOST"], f["ALT"], f["LMF"], f["ENT"]) for f in K.joint_forms()}, sorted(forms)
    assert "rows <= nasr_lp::SMALL_ROWS" in src and DR.SMALL_ROWS == 64
    for lit in ("k_dec_joint_tiled<true, false, true>", "k_dec_joint_tiled<true, true, true, true>", "k_dec_pred<true>", "k_dec_pred<false>", "k_dec_lstm<0>", "k_dec_lstm<1>"):
        assert lit in src, lit
    # the parametrised tests above name every one of them (collected here without a GPU; the GPU runs add to REACHED as they pass)
    planned = {"k_encproj", "k_dec_begin", "k_dec_lstm<0>", "k_dec_lstm<1>", "k_dec_pred<false>", "k_dec_pred<true>", "k_dec_lmrows", "k_lm_rows_slots",
               K.joint_kernel(17, beam=True, LP=True, ALT=True), K.joint_kernel(17, beam=True, LP=True, BOOST=True, ALT=True, BEAMB=True)}
    for f in K.joint_forms():
        planned |= {K.joint_kernel(5 * 4, **f), K.joint_kernel(22 * 4, **f)}
    for f in COMMIT_FORMS:
        planned.add(K.commit_kernel(**f))
    assert planned == want - set(UNREACHED), sorted(planned ^ want)
    assert REACHED <= want, sorted(REACHED - want)


def test_report_fractions():
    """the largest observed fraction of its bound per kernel, for profiles/decode_kernels.md (printed; nothing is asserted beyond what each test asserted)"""
    for k in sorted(FRACTIONS):
        print(f"largest fraction of its bound: {k}: {FRACTIONS[k]:.3f}")
