"""Every GEMM kernel of nemotron-asr.cpp_amd/csrc/kernels_gemm.hip, alone, against a float64 product (tests/gemm_ref.py).

tests/helpers/gemm_harness.hip runs ONE GEMM through the product's launcher (launch_gemm_bf16 / launch_gemm_f32: the plan and the kernel as the pair the
engine uses) on buffers with guard regions and returns every output buffer whole, together with the plan.  Each case names the kernel instance it is
there for and the test asserts the plan took it; the cases are the smallest shapes that reach each instance on a 256-CU chip.

Two modes per case:
  exact    A, W in {-3 .. 3}, integer biases and residuals, resid_scale 0.5: every product and partial sum is an integer below 9 x 4352 < 2^24, so the
           f32 result is the same in any summation order.  `==` on every element (bf16 outputs: the bf16 rounding of the exact value).  One dropped,
           doubled or misplaced product fails.  PART, QKV, the four BIAS epilogues and RESID.
  bounded  A ~ N(0, 1), W ~ U(+-sqrt(3 / K)), both rounded to the operand type, non-zero biases.  Per element
               |got - ref| <= K 2^-23 S[m, n],  S = |A| |W|^T                (bf16 kernels: twice the classical bound of an f32 sum of K exact products)
               |got - ref| <= K 2^-24 S[m, n]                                (f32 kernels: one fmaf chain)
           SiLU and GLU carry that bound through the epilogue (|silu'| <= 1.1, |v sigmoid'(g)| <= |v| / 4) and add EXPF_REL |ref| for __expf and
           v_rcp_f32; bf16 outputs add 2^-8 |ref| for their one rounding.
Both modes: every byte the GEMM does not own still holds the sentinel (rows >= M, columns >= N of an output with ldo > N, the regions in front of
and behind each buffer, the K / V ring rows and slots the case does not address), and the A rows behind row M - 1 are NaN, as are the gaps of
an A operand with lda > K or a row map: none of it may reach a row < M.

EXPF_REL: measured as max |got - e(s)| / |e(s)| where s is the kernel's OWN f32 sum (an EPI_PART_F32 run of the same case) and e the float64 epilogue,
over every f32-output SiLU / GLU case of this file on an MI355X: 3.15e-7 at the worst (k_gemm_f32_mfma<128, 128>, GLU; profiles/gemm_kernel_parity.md), times 4.
"""
from __future__ import annotations

import ctypes as C
import zlib
from dataclasses import dataclass, replace
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi
from tests import gemm_ref as R
from tests.test_gpu_parity import _acc

ROOT = Path(__file__).resolve().parent.parent
HELPER = ROOT / "tests" / "helpers" / "libgemm_harness.so"
ENGINE_LIB = capi.LIB_PATH          # the library under test (NASR_LIB_PATH: a diagnostic build of the same ABI)
GUARD = 256 * 1024            # bytes in front of and behind every buffer: more than one row of the widest output
EXPF_REL = 4 * 3.15e-7        # see the module docstring
CHIP_CUS = 256                # the cases below were chosen for the MI355X's 256 CUs
UNREACHED = {"k_gemm_skinny<4>"}          # the ladder takes <2> up to 32 rows and the skinny path ends there

PART, SILU, QKV, GLU, BIAS, BIAS_RELU_ACT, BIAS_RELU, BIAS_ACT, RESID = range(9)
EXACT_EPIS = (PART, QKV, BIAS, BIAS_RELU_ACT, BIAS_RELU, BIAS_ACT, RESID)


class CaseStruct(C.Structure):          # struct Case of gemm_harness.hip
    _fields_ = [(n, C.c_int) for n in ("M", "N", "K", "lda", "rows_per_batch", "batch_stride", "row_offset", "epi", "splits", "ldo", "ldo_act", "dtype")] + \
               [("resid_scale", C.c_float)] + \
               [(n, C.c_int) for n in ("T", "n_batch_rows", "n_slots", "coresident", "prio", "no_persist", "no_wide", "wide_rows", "tile_bands", "t64_tiles_p1",
                                       "wide_min_tiles", "wide_min_rows", "narrow_stores", "f32_fma_tile", "resid_in_place", "guard_bytes")] + \
               [(n, C.c_longlong) for n in ("a_elems", "out_f32_elems", "out_act_elems", "q_elems")]


class PlanStruct(C.Structure):
    _fields_ = [("inst", C.c_int), ("grid", C.c_int * 3), ("block", C.c_int), ("lds", C.c_int), ("n_groups", C.c_int), ("m_chunks", C.c_int), ("splits", C.c_int)]


@dataclass(frozen=True)
class Case:
    inst: str | None              # the kernel instance the case is there for (GEMM_INST_NAME without blanks and parentheses); None: an f32 case
    M: int
    N: int
    K: int
    epi: int = BIAS
    splits: int = 1
    opts: tuple = ()              # GemmParams option fields, (name, value) pairs; no_persist defaults to 1 (the engine's default)
    f32: bool = False
    lda: int = 0                  # 0: K
    rowmap: tuple | None = None   # (rows_per_batch, batch_stride, row_offset)
    T: int = 1                    # EPI_QKV: rows per stream
    qkv: str = "wrap"             # "wrap": kv_head + LCTX + i passes KVC inside the chunk; "perm": permuted slots, arbitrary heads; "both": permuted slots, wrapping heads
    in_place: bool = False        # EPI_RESID_F32: resid == out_f32

    def ident(self) -> str:
        s = f"{self.inst or 'f32'}-{self.M}x{self.N}x{self.K}-{R.EPI_NAMES[self.epi]}"
        if self.splits > 1: s += f"-s{self.splits}"
        if self.opts: s += "-" + ",".join(f"{k}={v}" for k, v in self.opts)
        if self.lda: s += f"-lda{self.lda}"
        if self.rowmap: s += "-map%d.%d.%d" % self.rowmap
        if self.epi == QKV: s += f"-T{self.T}{self.qkv}"
        if self.in_place: s += "-inplace"
        return s

    def struct(self) -> CaseStruct:
        c = CaseStruct()
        c.M, c.N, c.K, c.lda, c.epi, c.splits, c.T = self.M, self.N, self.K, self.lda or self.K, self.epi, self.splits, self.T
        if self.rowmap:
            c.rows_per_batch, c.batch_stride, c.row_offset = self.rowmap
        n_out = self.N // 2 if self.epi == GLU else self.N
        c.ldo, c.ldo_act = n_out + 8, n_out + 8          # eight guard columns behind every output row
        c.dtype, c.resid_scale, c.guard_bytes, c.no_persist = int(self.f32), 0.5, GUARD, 1
        c.resid_in_place = int(self.in_place)
        for k, v in self.opts:
            assert hasattr(c, k), k
            setattr(c, k, v)
        return c


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _o(**kw):
    return tuple(kw.items())


PIPE = _o(coresident=1, wide_min_rows=225, wide_min_tiles=1)          # a pipelined step whose 224-row tiles start at 225 rows
PERSIST = _o(no_persist=0, no_wide=1)
SK1, SK2, T64_4, T64_3, T64W = "k_gemm_skinny<1>", "k_gemm_skinny<2>", "k_gemm_t64<4>", "k_gemm_t64<3>", "k_gemm_t64w"
TILED2, ROLES, TILED3, K32 = "k_gemm_tiled2<4>", "k_gemm_roles<4>", "k_gemm_tiled3", "k_gemm_tiled2_k32<4>"
W2_256, W_256_7, W_256_8, W2_192 = "k_gemm_wide2<256,7>", "k_gemm_wide<256,7>", "k_gemm_wide<256,8>", "k_gemm_wide2<192,7>"
PERSIST_OF = {PART: "k_gemm_persist<EPI_PART_F32>", SILU: "k_gemm_persist<EPI_SILU_ACT>", QKV: "k_gemm_persist<EPI_QKV>", GLU: "k_gemm_persist<EPI_GLU>",
              BIAS: "k_gemm_persist<EPI_BIAS_F32>", BIAS_RELU: "k_gemm_persist<EPI_BIAS_RELU_F32>"}

# Epilogues an instance can be handed.  Every per-tile kernel ends in epi_quad / epi_oct / wave_epilogue_rows, which take all nine; EPI_RESID_F32 needs the whole
# K sum in one workgroup (gemm_resid_foldable: never the skinny kernel) and EPI_QKV needs N = 3072, so it runs at a shape of its own.
EPIS_NO_QKV = (PART, SILU, GLU, BIAS, BIAS_RELU_ACT, BIAS_RELU, BIAS_ACT, RESID)

# one base shape per instance (every epilogue but QKV runs on it) and one N = 3072 shape for QKV
BASE = {
    SK1: (Case(SK1, 16, 128, 64), Case(SK1, 16, 3072, 64)),
    SK2: (Case(SK2, 32, 128, 64), Case(SK2, 32, 3072, 64)),
    T64_4: (Case(T64_4, 33, 128, 64), Case(T64_4, 33, 3072, 64)),
    T64_3: (Case(T64_3, 33, 128, 64, opts=_o(coresident=2)), Case(T64_3, 33, 3072, 64, opts=_o(coresident=2))),
    TILED2: (Case(TILED2, 129, 5120, 64), Case(TILED2, 257, 3072, 64)),
    ROLES: (Case(ROLES, 129, 5120, 512), Case(ROLES, 257, 3072, 512)),
    TILED3: (Case(TILED3, 129, 5120, 512, opts=_o(coresident=2)), Case(TILED3, 257, 3072, 512, opts=_o(coresident=2))),
    K32: (Case(K32, 129, 5120, 512, opts=_o(coresident=2, prio=20)), Case(K32, 257, 3072, 512, opts=_o(coresident=2, prio=20))),
    W2_256: (Case(W2_256, 1025, 1024, 256, opts=PIPE), Case(W2_256, 1025, 3072, 256, opts=PIPE)),
    W_256_7: (Case(W_256_7, 1025, 1024, 256, opts=PIPE + _o(prio=20)), Case(W_256_7, 1025, 3072, 256, opts=PIPE + _o(prio=20))),
    W_256_8: (Case(W_256_8, 1025, 1024, 256, opts=PIPE + _o(wide_rows=256)), Case(W_256_8, 1025, 3072, 256, opts=PIPE + _o(wide_rows=256))),
    W2_192: (Case(W2_192, 2913, 3072, 256), Case(W2_192, 2913, 3072, 256)),
}


def _epilogue_cases(inst):
    base, qkv = BASE[inst]
    epis = [e for e in EPIS_NO_QKV if not (e == RESID and inst in (SK1, SK2))]
    # the 128 x 64 tiles take split-K partials at N = 1024 only (gemm_use_t64)
    out = [replace(base, epi=e, N=1024 if e == PART and inst in (T64_4, T64_3) else base.N) for e in epis]
    if qkv.M <= 300:
        out += [replace(qkv, epi=QKV, T=14, qkv="wrap"), replace(qkv, epi=QKV, T=1 if qkv.M <= 64 else 14, qkv="perm")]
    else:                                     # one run for both (a K / V pool of M / 14 slots)
        out += [replace(qkv, epi=QKV, T=14, qkv="both")]
    if inst in (T64_4, ROLES, W2_256):          # the four-columns-per-thread form of the 16-bit / paired epilogues (engine option "epilogue16" = 0)
        out += [replace(base, epi=e, opts=base.opts + _o(narrow_stores=1)) for e in (SILU, GLU)] + [replace(qkv, epi=QKV, T=14, opts=qkv.opts + _o(narrow_stores=1))]
    return out


def _ragged(inst, N, K, Ms, opts=()):
    return [Case(inst, M, N, K, opts=opts) for M in Ms]


M128 = (33, 127, 128, 129, 257)
FAMILIES: dict[str, list[Case]] = {
    "skinny": _epilogue_cases(SK1) + _epilogue_cases(SK2)
              + _ragged(SK1, 128, 64, (1, 15, 16)) + _ragged(SK2, 128, 64, (17, 31, 32))
              + [Case(SK1, 16, 128, 1024, epi=PART, splits=s) for s in (2, 4, 8)] + [Case(SK2, 31, 128, 1024, epi=PART, splits=4)]
              + [Case(SK1, 15, 128, 64, lda=72), Case(SK2, 31, 128, 64, lda=72)],
    "t64": _epilogue_cases(T64_4) + _epilogue_cases(T64_3)
           + _ragged(T64_4, 128, 64, M128) + _ragged(T64_3, 128, 64, M128, _o(coresident=2))
           + [Case(T64_4, 129, 1024, 256, epi=PART, splits=4), Case(T64_4, 300, 1024, 512, epi=PART, splits=2),
              Case(T64_3, 129, 1024, 256, epi=PART, splits=4, opts=_o(coresident=2)), Case(T64_4, 127, 128, 64, lda=72)],
    "t64w": [Case(T64W, M, 1024, K, epi=RESID, splits=2, in_place=ip) for (M, K) in ((257, 256), (300, 512)) for ip in (False, True)]
            + [Case(T64W, 257, 1024, 256, epi=RESID, splits=2, lda=264)],
    "tiled128": _epilogue_cases(TILED2) + _epilogue_cases(ROLES) + _epilogue_cases(TILED3) + _epilogue_cases(K32)
                + [Case(K32, 129, 5120, 64, opts=_o(coresident=2))]
                + _ragged(TILED2, 8320, 64, M128) + _ragged(ROLES, 8320, 512, M128) + _ragged(TILED3, 8320, 512, M128, _o(coresident=2))
                + _ragged(K32, 8320, 512, M128, _o(coresident=2, prio=20))
                # split-K on the 128 x 128 tiles: more than 64 tiles at N = 1024
                + [Case(TILED2, 1100, 1024, 512, epi=PART, splits=2), Case(ROLES, 1100, 1024, 1024, epi=PART, splits=2),
                   Case(TILED3, 1100, 1024, 1024, epi=PART, splits=2, opts=_o(coresident=2)), Case(K32, 1100, 1024, 256, epi=PART, splits=4, opts=_o(coresident=2))]
                + [Case(TILED2, 129, 5120, 64, lda=72), Case(ROLES, 129, 5120, 512, lda=520), Case(TILED3, 129, 5120, 512, lda=520, opts=_o(coresident=2)),
                   Case(K32, 129, 5120, 512, lda=520, opts=_o(coresident=2, prio=20))],
    "wide": _epilogue_cases(W2_256) + _epilogue_cases(W_256_7) + _epilogue_cases(W_256_8) + _epilogue_cases(W2_192)
            + [Case(W2_256, 1121, 1024, 256, opts=PIPE), Case(W_256_7, 1121, 1024, 256, opts=PIPE + _o(prio=20)), Case(W2_192, 3361, 3072, 256)]
            + [Case(W_256_7, M, 1024, K, opts=PIPE) for K in (224, 128, 96, 64, 32) for M in (1025, 1121)]          # fewer chunks than the ring has slots
            + [Case(W_256_8, 3585, 4096, 64)]                                                                          # the synchronous form
            # TitaNet's K = 128 GEMMs as spk_gemm launches them (nasr_diar.hip: zeroed params, no_persist = 1, coresident = 1), 10 sub-segments of 160 rows
            + [Case(W_256_7, 1600, 1024, 128, opts=_o(coresident=1)), Case(W_256_7, 1600, 3072, 128, epi=BIAS_RELU, opts=_o(coresident=1))]
            + [Case(W2_256, 1025, 1024, 256, lda=264, opts=PIPE), Case(W_256_7, 1025, 1024, 96, lda=104, opts=PIPE), Case(W_256_8, 1025, 1024, 256, lda=264, opts=PIPE + _o(wide_rows=256)),
               Case(W2_192, 2913, 3072, 256, lda=264)],
    "persist": [Case(PERSIST_OF[e], 1665, 4096, 1024, epi=e, opts=PERSIST) for e in (PART, SILU, GLU, BIAS, BIAS_RELU)]
               + [Case(PERSIST_OF[QKV], 2311, 3072, 1024, epi=QKV, T=14, qkv="both", opts=PERSIST)]
               + [Case(PERSIST_OF[GLU], 1665, 4096, 1024, epi=GLU, opts=PERSIST + _o(narrow_stores=1))],
    # the out projection of the subsampling (run_sub_out, nasr_encoder.hip): A rows through the batched row map (T rows per stream out of T + 2, the first
    # DROP_EXTRA = 2 dropped), K = lda = 17 x 256, on every kernel family B x T rows can reach
    "rowmap": [Case(SK1, 16, 1024, 4352, rowmap=(1, 3 * 4352, 2)), Case(SK2, 28, 1024, 4352, rowmap=(14, 16 * 4352, 2)),
               Case(T64_4, 42, 1024, 4352, rowmap=(14, 16 * 4352, 2)), Case(T64_3, 784, 1024, 4352, rowmap=(14, 16 * 4352, 2), opts=_o(coresident=1)),
               Case(ROLES, 1036, 1024, 4352, rowmap=(14, 16 * 4352, 2)), Case(TILED3, 1036, 1024, 4352, rowmap=(14, 16 * 4352, 2), opts=_o(coresident=1)),
               Case(K32, 1036, 1024, 4352, rowmap=(14, 16 * 4352, 2), opts=_o(coresident=1, prio=20)),
               Case(W2_256, 1582, 1024, 4352, rowmap=(14, 16 * 4352, 2), opts=_o(coresident=1)),
               Case(W_256_7, 1582, 1024, 4352, rowmap=(14, 16 * 4352, 2), opts=_o(coresident=1, prio=20))],
}

# f32 kernels through launch_gemm_f32 (no plan: the kernel follows from the launcher's conditions, named here for the reader)
F32_EPIS = (PART, SILU, GLU, BIAS, BIAS_RELU_ACT, BIAS_RELU, BIAS_ACT)
F32_FAMILIES: dict[str, list[Case]] = {
    # k_gemm_f32_rows: M <= 4; K a multiple of its 1008-deep chunk, and not
    "f32_rows": [Case(None, M, 64, K, f32=True) for M in (1, 4) for K in (2016, 1024)] + [Case(None, 4, 64, 1024, epi=e, f32=True) for e in F32_EPIS]
                + [Case(None, 3, 3072, 64, epi=QKV, T=1, qkv="perm", f32=True), Case(None, 4, 64, 1024, lda=1032, f32=True)],
    # k_gemm_f32_mfma<64, 64>
    "f32_mfma64": [Case(None, M, 128, 64, f32=True) for M in (5, 63, 64, 65)] + [Case(None, 65, 128, 96, epi=e, f32=True) for e in F32_EPIS + (RESID,)]
                  + [Case(None, 65, 3072, 64, epi=QKV, T=14, qkv="wrap", f32=True), Case(None, 65, 128, 96, lda=104, f32=True),
                     Case(None, 28, 1024, 4352, rowmap=(14, 16 * 4352, 2), f32=True)],
    # k_gemm_f32_mfma<128, 128>: from 192 tiles
    "f32_mfma128": [Case(None, 1537, 2048, 64, f32=True), Case(None, 1537, 2048, 64, epi=GLU, f32=True), Case(None, 1537, 2048, 64, epi=RESID, f32=True, in_place=True)],
    # k_gemm_f32: asked for (f32_fma_tile = 1), or an lda that is no multiple of 4
    "f32_fma": [Case(None, M, 128, 64, f32=True, opts=_o(f32_fma_tile=1)) for M in (5, 16, 17)] + [Case(None, 17, 128, 96, epi=e, f32=True, opts=_o(f32_fma_tile=1)) for e in F32_EPIS]
               + [Case(None, 2, 128, 64, lda=66, f32=True), Case(None, 17, 128, 64, lda=66, f32=True),
                  Case(None, 17, 3072, 64, epi=QKV, T=14, qkv="wrap", f32=True, opts=_o(f32_fma_tile=1))],
}


def _modes(case: Case):
    return ("exact", "bounded") if case.epi in EXACT_EPIS else ("bounded",)


def _groups(families, split=(), budget=60e6):
    """test groups: a family, or (the two large families) its cases per instance, cut into parts of at most `budget` output elements x modes, so that
    every parametrised test stays at a few seconds (what a run costs here is the float64 arithmetic on its outputs); duplicates dropped"""
    whole: dict[str, list[Case]] = {}
    for fam, cases in families.items():
        for c in cases:
            g = whole.setdefault(f"{fam}-{c.inst}" if fam in split else fam, [])
            if c not in g:
                g.append(c)
    out: dict[str, list[Case]] = {}
    for name, cases in whole.items():
        parts, cost = [[]], 0.0
        for c in cases:
            w = float(c.M) * c.N * len(_modes(c)) * (1 + c.K / 2048)
            if parts[-1] and cost + w > budget:
                parts.append([])
                cost = 0.0
            parts[-1].append(c)
            cost += w
        for i, part in enumerate(parts):
            out[name if len(parts) == 1 else f"{name}-{i + 1}of{len(parts)}"] = part
    return out


GROUPS = _groups(FAMILIES, split=("tiled128", "wide"))
F32_GROUPS = _groups(F32_FAMILIES)


def all_bf16_cases():
    return [c for cs in GROUPS.values() for c in cs]


# ---- the harness ---------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def harness():
    if not HELPER.exists():
        pytest.skip("tests/helpers/libgemm_harness.so not built (python __graft_entry__.py warns when the helper fails to compile)")
    C.CDLL(str(ENGINE_LIB), mode=C.RTLD_GLOBAL)          # the helper's undefined nasr:: symbols resolve against the product library
    L = C.CDLL(str(HELPER))
    L.gemm_harness_error.restype = C.c_char_p
    L.gemm_harness_inst_name.restype = C.c_char_p
    L.gemm_harness_total_bytes.restype = C.c_longlong
    L.gemm_harness_total_bytes.argtypes = [C.c_longlong, C.c_int]
    L.gemm_harness_plan.argtypes = [C.POINTER(CaseStruct), C.c_int, C.POINTER(PlanStruct)]
    L.gemm_harness_plan.restype = None
    L.gemm_harness_run.argtypes = [C.c_int, C.POINTER(CaseStruct)] + [C.c_void_p] * 10 + [C.POINTER(PlanStruct), C.POINTER(C.c_int)]
    assert L.gemm_harness_case_bytes() == C.sizeof(CaseStruct)
    return L


def inst_names(L) -> list[str]:
    return [L.gemm_harness_inst_name(i).decode().replace(" ", "").replace("(", "").replace(")", "") for i in range(L.gemm_harness_inst_count())]


def planned_instance(L, case: Case, num_cus: int = CHIP_CUS) -> str:
    cs, pl = case.struct(), PlanStruct()
    L.gemm_harness_plan(C.byref(cs), num_cus, C.byref(pl))
    return inst_names(L)[pl.inst]


@pytest.fixture(scope="module")
def gpu_harness():
    L = harness()
    cus = L.gemm_harness_num_cus(0)
    if cus != CHIP_CUS:
        pytest.skip(f"the cases are chosen for a {CHIP_CUS}-CU chip (gemm_plan_bf16 reads the CU count); device 0 reports {cus}")
    return L


# ---- inputs and references, one per (operand type, mode, shape), shared by every epilogue and option set run on it --------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


class Operands:
    def __init__(self, f32: bool, mode: str, M: int, N: int, K: int):
        rng = _rng("operands", f32, mode, M, N, K)
        if mode == "exact":
            self.A = rng.integers(-3, 4, (M, K)).astype(np.float32)
            self.W = rng.integers(-3, 4, (N, K)).astype(np.float32)
        else:
            rnd = (lambda x: x) if f32 else R.bf16_round
            self.A = rnd(rng.standard_normal((M, K)).astype(np.float32))
            self.W = rnd(rng.uniform(-np.sqrt(3.0 / K), np.sqrt(3.0 / K), (N, K)).astype(np.float32))
        self.mode, self._P, self._S, self._slices = mode, None, None, {}

    @property
    def P(self):          # the exact product; integers below 2^24 are exact in an f32 matmul as well, whatever its order
        if self._P is None:
            self._P = (self.A @ self.W.T).astype(np.float64) if self.mode == "exact" else R.product(self.A, self.W)
        return self._P

    @property
    def S(self):
        if self._S is None:
            self._S = R.abs_product(self.A, self.W)
        return self._S

    def slices(self, bounds):
        key = tuple(bounds)
        if key not in self._slices:
            self._slices[key] = R.product_slices(self.A, self.W, bounds)
        return self._slices[key]


_OPERANDS: dict = {}


def operands(f32, mode, M, N, K) -> Operands:
    key = (f32, mode, M, N, K)
    if key not in _OPERANDS:
        if len(_OPERANDS) >= 6:          # the large shapes come in runs: keep memory flat
            _OPERANDS.pop(next(iter(_OPERANDS)))
        _OPERANDS[key] = Operands(*key)
    return _OPERANDS[key]


def bias_of(mode, N):
    rng = _rng("bias", mode, N)
    if mode == "exact":
        return rng.integers(-8, 9, N).astype(np.float32)
    return (rng.uniform(0.1, 1.0, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32)


def resid_of(mode, M, N):
    rng = _rng("resid", mode, M, N)
    return rng.integers(-50, 51, (M, N)).astype(np.float32) if mode == "exact" else rng.standard_normal((M, N)).astype(np.float32)


def qkv_rows(case: Case):
    """-> (slot [B], kv_head [B], n_slots); two slots of the pool stay unaddressed"""
    B = (case.M + case.T - 1) // case.T
    rng = _rng("rows", case.M, case.T, case.qkv)
    slot = np.arange(B, dtype=np.int32) if case.qkv == "wrap" else rng.permutation(B + 2)[:B].astype(np.int32)
    if case.qkv in ("wrap", "both"):          # stream b's ring rows pass KVC at frame b % T of the chunk (T = 1: every second stream's only row is the wrapped one)
        head = (R.KVC - R.LCTX - np.arange(B) % max(case.T, 2)).astype(np.int32)
    else:
        head = rng.integers(0, R.KVC, B).astype(np.int32)
    return slot, head, B + 2


# ---- one run ---------------------------------------------------------------------------------------------------------------------
RATIOS: dict[str, float] = {}          # kernel -> worst |got - ref| / bound of its bounded runs with f32 outputs
RATIOS_16: dict[str, float] = {}       # ... with bf16 outputs: their own rounding, up to 2^-8 |ref| of the bound, is most of the error, so these sit near 1 by construction
EXPF_SEEN: dict[str, float] = {}       # kernel -> worst relative error of the SiLU / GLU epilogue alone
_SENT16 = 0xFFC5


class Out:
    """one output buffer as the harness returns it: [guard | body | guard]"""

    def __init__(self, L, elems: int, dtype):
        self.dtype, self.elems = np.dtype(dtype), elems
        self.raw = np.zeros(L.gemm_harness_total_bytes(elems * self.dtype.itemsize, GUARD), dtype=np.uint8) if elems else None

    def ptr(self):
        return self.raw.ctypes.data if self.raw is not None else None

    def check(self, written: np.ndarray, what: str) -> np.ndarray:
        """written: bool mask over the body's elements -> the body as values, after checking that everything else still holds the sentinel"""
        bits = self.raw.view(np.uint16 if self.dtype.itemsize == 2 else np.uint32)
        sent = _SENT16 if self.dtype.itemsize == 2 else (_SENT16 << 16 | _SENT16)
        g = GUARD // self.dtype.itemsize
        keep = np.ones(bits.size, dtype=bool)
        keep[g:g + self.elems] = ~written.ravel()
        bad = np.flatnonzero(keep & (bits != sent))
        assert bad.size == 0, (f"{what}: {bad.size} elements outside the GEMM's output were overwritten; first at body offset {int(bad[0]) - g} "
                               f"(body = {self.elems} elements; negative: the front guard)")
        body = bits[g:g + self.elems]
        return R.bf16_to_f32(body) if self.dtype.itemsize == 2 else body.view(np.float32)


def _compare(what, mode, got, ref, bound, bf16_out, worst):
    """exact: got == ref after the output type's rounding.  bounded: |got - ref| <= bound (+ 2^-8 |ref| for a bf16 output); -> worst ratio"""
    if mode == "exact":
        want = ref.astype(np.float32)
        if bf16_out:
            want = R.bf16_round(want)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ from the exact result; first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, "
                                 f"want {want[tuple(bad[0])]!r}; rows {sorted(set(bad[:, 0].tolist()))[:8]}, columns {sorted(set(bad[:, -1].tolist()))[:8]}")
        return worst
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} non-finite values in the output"          # finiteness first: max() swallows NaN
    err = np.abs(got.astype(np.float64) - ref)
    _acc(0.0, err)
    if bf16_out:
        bound = bound + 2.0 ** -8 * np.abs(ref)
    ratio = err / bound
    r = float(ratio.max())
    at = np.unravel_index(int(ratio.argmax()), ratio.shape)
    assert r <= 1.0, f"{what}: |got - ref| = {err[at]:.3e} exceeds the bound {bound[at]:.3e} at {tuple(int(i) for i in at)} (ratio {r:.3f})"
    return max(worst, r)


def launch(L, case: Case, mode: str, epi=None):          # epi: run the case with another epilogue (the instance is then not checked)
    """runs the case -> (plan instance name or None, dict of checked outputs as values, operands, extras)"""
    check_inst = epi is None
    if epi is not None:
        case = replace(case, epi=epi)
    cs = case.struct()
    M, N, K, f32 = case.M, case.N, case.K, case.f32
    ops = operands(f32, mode, M, N, K)
    # A image: every row the map addresses; everything else (lda gaps, the rows a row map skips) is NaN
    off = R.a_row_offsets(M, cs.lda, cs.rows_per_batch, cs.batch_stride, cs.row_offset)
    a_elems = int(off.max()) + cs.lda
    if case.rowmap:
        a_elems = ((M + cs.rows_per_batch - 1) // cs.rows_per_batch) * cs.batch_stride
    img = np.full(a_elems, np.nan, dtype=np.float32)
    img[(off[:, None] + np.arange(K)[None, :]).ravel()] = ops.A.ravel()
    cs.a_elems = a_elems
    act = np.float32 if f32 else np.uint16
    n_out = N // 2 if case.epi == GLU else N
    n_slabs = case.splits if case.epi == PART else 1          # [split][M][ldo] partial slabs; every other epilogue owns the whole K sum
    bias = bias_of(mode, N) if case.epi in R.HAS_BIAS else None
    resid_img = None
    if case.epi == RESID:          # [M][ldo]; the guard columns hold the sentinel (in place they are the output's guard columns)
        resid_img = np.full((M, cs.ldo), _SENT16 << 16 | _SENT16, dtype=np.uint32).view(np.float32)
        resid_img[:, :N] = resid_of(mode, M, N)
    slot = head = None
    if case.epi == QKV:
        assert N == 3 * R.D
        slot, head, cs.n_slots = qkv_rows(case)
        cs.n_batch_rows, cs.q_elems = len(slot), M * R.D
    elif case.epi in R.ACT_OUT:
        cs.out_act_elems = M * cs.ldo_act
    else:
        cs.out_f32_elems = n_slabs * M * cs.ldo
    o_f32, o_act, o_q = Out(L, cs.out_f32_elems, np.float32), Out(L, cs.out_act_elems, act), Out(L, cs.q_elems, np.float32)
    o_kv = Out(L, cs.n_slots * 2 * R.KVC * R.D, act)
    W = np.ascontiguousarray(ops.W)
    pl, cus = PlanStruct(), C.c_int(0)
    p = lambda a: a.ctypes.data if a is not None else None
    rc = L.gemm_harness_run(0, C.byref(cs), p(img), p(W), p(bias), p(resid_img), p(slot), p(head), o_f32.ptr(), o_act.ptr(), o_q.ptr(), o_kv.ptr(), C.byref(pl), C.byref(cus))
    if rc != 0:
        # a HIP error leaves the device context unusable: nothing more of this session may start on the GPU
        pytest.exit(f"{case.ident()} [{mode}]: {L.gemm_harness_error().decode()}", returncode=3)
    name = None
    if not f32:
        name = inst_names(L)[pl.inst]
        assert not check_inst or name == case.inst, f"{case.ident()}: the plan took {name} (grid {list(pl.grid)}, {cus.value} CUs), the case is there for {case.inst}"
    what = f"{case.ident()} [{mode}]"
    outs = {}
    if case.epi == QKV:
        outs["q"] = o_q.check(np.ones(M * R.D, dtype=bool), what + " q_out").reshape(M, R.D)
        s_of, r_of = R.kv_index(M, case.T, slot, head)
        written = np.zeros((cs.n_slots, 2, R.KVC, R.D), dtype=bool)
        written[s_of, :, r_of, :] = True
        kv = o_kv.check(written, what + " kv_pool").reshape(cs.n_slots, 2, R.KVC, R.D)
        outs["k"], outs["v"] = kv[s_of, 0, r_of, :], kv[s_of, 1, r_of, :]
    elif case.epi in R.ACT_OUT:
        written = np.zeros((M, cs.ldo_act), dtype=bool)
        written[:, :n_out] = True
        outs["act"] = o_act.check(written, what + " out_act").reshape(M, cs.ldo_act)[:, :n_out]
    else:
        written = np.zeros((n_slabs * M, cs.ldo), dtype=bool)
        written[:, :n_out] = True
        outs["f32"] = o_f32.check(written, what + " out_f32").reshape(n_slabs, M, cs.ldo)[:, :, :n_out]
    return name, outs, ops, dict(bias=bias, resid=resid_img[:, :N] if resid_img is not None else None, unit=32 if (name or "").startswith("k_gemm_skinny") else 64)


def run_case(L, case: Case, mode: str):
    name, outs, ops, ex = launch(L, case, mode)
    what, key = f"{case.ident()} [{mode}]", name or _f32_kernel(case)
    K, f32, epi = case.K, case.f32, case.epi
    b_acc = None if mode == "exact" else K * 2.0 ** (-24 if f32 else -23) * ops.S
    worst = 0.0
    if epi == PART and case.splits > 1:
        bounds = R.k_slice_bounds(K, case.splits, ex["unit"])
        ref = ops.slices(bounds)
        b_sl = None
        if mode != "exact":          # the bound of each slice's own sum: its K_s products and its share of S
            ks = np.diff(bounds).astype(np.float64)[:, None, None]
            b_sl = ks * 2.0 ** -23 * R.product_slices(np.abs(ops.A), np.abs(ops.W), bounds)
        worst = _compare(what, mode, outs["f32"], ref, b_sl, False, worst)
    elif epi == QKV:
        for nm, lo, bf in (("q", 0, False), ("k", R.D, not f32), ("v", 2 * R.D, not f32)):
            worst = _compare(f"{what} {nm}", mode, outs[nm], ops.P[:, lo:lo + R.D], None if mode == "exact" else b_acc[:, lo:lo + R.D], bf, worst)
    else:
        ref = R.epilogue(epi, ops.P, ex["bias"], ex["resid"], 0.5)
        bound = None
        if mode != "exact":
            bound = R.epilogue_bound(epi, ops.P, b_acc) * (0.5 if epi == RESID else 1.0)
            if epi in (SILU, GLU):
                bound = bound + EXPF_REL * np.abs(ref)
        got = outs["act"] if epi in R.ACT_OUT else outs["f32"][0]
        worst = _compare(what, mode, got, ref, bound, epi in R.ACT_OUT and not f32, worst)
        if mode != "exact" and epi in (SILU, GLU) and got.dtype == np.float32 and (f32 or epi == GLU):
            # the epilogue alone: against the float64 epilogue of the kernel's own f32 sums (a PART run of the same case)
            _, part, _, _ = launch(L, case, mode, epi=PART)
            own = R.epilogue(epi, part["f32"][0].astype(np.float64))
            nz = own != 0
            rel = float((np.abs(got.astype(np.float64) - own)[nz] / np.abs(own[nz])).max())
            assert np.isfinite(rel)
            EXPF_SEEN[key] = max(EXPF_SEEN.get(key, 0.0), rel)
            print(f"EXPF {key} {R.EPI_NAMES[epi]} {case.M}x{case.N}x{case.K} rel {rel:.3e}")
    if mode != "exact":
        table = RATIOS_16 if not f32 and (epi in R.ACT_OUT or epi == QKV) else RATIOS          # (QKV: the worst of q, k and v: the 16-bit rings decide it)
        table[key] = max(table.get(key, 0.0), worst)
        print(f"RATIO {key} {what} {worst:.4f}")


def _f32_kernel(case: Case) -> str:
    """launch_gemm_f32's ladder (kernels_gemm.hip), for the report only"""
    lda = case.lda or case.K
    if case.M <= 4 and case.N % 4 == 0 and case.K % 4 == 0 and lda % 4 == 0:
        return "k_gemm_f32_rows"
    if not dict(case.opts).get("f32_fma_tile") and case.M > 4 and case.N % 64 == 0 and case.K % 32 == 0 and lda % 4 == 0:
        return "k_gemm_f32_mfma<128,128>" if case.N % 128 == 0 and (case.N // 128) * ((case.M + 127) // 128) >= 192 else "k_gemm_f32_mfma<64,64>"
    return "k_gemm_f32"


def _run_family(L, cases):
    assert len({c.ident() for c in cases}) == len(cases)
    failed = []
    for case in cases:          # every case runs, so that one report names all that fail (a HIP error ends the session in launch())
        for mode in _modes(case):
            try:
                run_case(L, case, mode)
            except AssertionError as exc:
                failed.append(str(exc))
    assert not failed, f"{len(failed)} failing runs:\n" + "\n".join(failed)


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(GROUPS))
def test_bf16_gemm_family_matches_the_float64_product(gpu_harness, family):
    _run_family(gpu_harness, GROUPS[family])


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(F32_GROUPS))
def test_f32_gemm_family_matches_the_float64_product(gpu_harness, family):
    _run_family(gpu_harness, F32_GROUPS[family])


@pytest.mark.gpu
def test_every_kernel_instance_has_a_case(gpu_harness):
    """the instances the cases reach on this chip are all of NASR_GEMM_INSTANCES but UNREACHED: a new instance, or a rule that reaches k_gemm_skinny<4>,
    fails here until it has a case (each run above asserts that the instance it names is the one the launcher's plan took)"""
    L = gpu_harness
    reached = {planned_instance(L, c, L.gemm_harness_num_cus(0)) for c in all_bf16_cases()}
    assert reached == set(inst_names(L)) - UNREACHED
    for k in sorted(set(RATIOS) | set(RATIOS_16)):
        print(f"WORST {k} ratio f32 outputs {RATIOS.get(k, float('nan')):.4f} bf16 outputs {RATIOS_16.get(k, float('nan')):.4f} epilogue alone {EXPF_SEEN.get(k, float('nan')):.3e}")


def test_cases_name_the_instance_the_plan_takes_at_256_cus():
    """no GPU: gemm_plan_bf16 through the helper's host-only entry, for every case, at the CU count the cases were chosen for"""
    L = harness()
    wrong = [(c.ident(), planned_instance(L, c)) for c in all_bf16_cases() if planned_instance(L, c) != c.inst]
    assert not wrong, wrong
    assert {c.inst for c in all_bf16_cases()} == set(inst_names(L)) - UNREACHED
    assert UNREACHED <= set(inst_names(L))
