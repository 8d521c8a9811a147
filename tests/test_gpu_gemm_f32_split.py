"""k_gemm_f32_split (GemmParams::f32_fma_tile = 2, engine option "f32_split") alone, through launch_gemm_f32 and the harness of
tests/test_gpu_gemm_kernels.py, against float64 products: a.w as a_hi.w_hi + a_hi.w_lo + a_lo.w_hi, hi = bf16(x), lo = bf16(x - hi), f32 accumulation.
  exact        integer operands in {-3 .. 3}: every low part is zero, `==` on every element (indexing, masking, guard regions, every epilogue).
  split-exact  operands h + l / 1024, h in {+-2, +-3}, l in {-3 .. 3}: hi = h, lo = l / 1024, no residue; the three kept products summed in float64 are
               multiples of 2^-10 below 2^14 for K <= 1024, exact in f32 in any order: `==`.  An f32 kernel returns the full product, with
               sum lo.lo', and differs -- as does a kernel that drops or doubles one of the three terms.
  bounded      A ~ N(0, 1), W ~ U(+-sqrt(3 / K)), unrounded f32, K <= 96: |got - ref| <= (3 2^-16 + 3 K 2^-23) S, S = |A| |W|^T: RNE to 8 significand bits
               is within 2^-8, so each dropped term (lo.lo', r.w, a.r') is <= 2^-16 |a||w|; 3 K f32 accumulations, doubled as for the bf16 kernels.
The launcher's tile rule (64 x 128 tiles from 384 of them, else 64 x 64) names the kernel beside each case; every form, the 128 x 128 one of A/B runs
included, is reached for certain by forcing it (bits 4-5 of f32_fma_tile), and all forms and the rule must return the same bits."""
from dataclasses import replace

import numpy as np
import pytest

from tests import gemm_ref as R
from tests import test_gpu_gemm_kernels as G
from tests.test_gpu_gemm_kernels import BIAS, EXACT_EPIS, F32_EPIS, GLU, PART, QKV, RESID, SILU, Case, gpu_harness  # noqa: F401  (fixture)

def _c(M, N, K, **kw):
    return Case(None, M, N, K, f32=True, opts=G._o(f32_fma_tile=2), **kw)


CASES = ([_c(M, 128, 64) for M in (5, 63, 64, 65)] + [_c(65, 128, 96, epi=e) for e in F32_EPIS + (RESID,)]                      # <64,64>
         + [_c(65, 3072, 64, epi=QKV, T=14, qkv="wrap"), _c(65, 128, 96, lda=104), _c(28, 1024, 4352, rowmap=(14, 16 * 4352, 2))]      # <64,64>
         + [_c(257, 2048, 64), _c(257, 2048, 64, epi=GLU)]                                                                       # <64,64>, 160 workgroups
         + [_c(1537, 2048, 64), _c(1537, 2048, 64, epi=GLU), _c(1537, 2048, 64, epi=RESID, in_place=True)])                      # <64,128>


def _bounded(L, case):          # run_case's bounded mode with the split kernel's own accumulation bound
    _, outs, ops, ex = G.launch(L, case, "bounded")
    what, K, epi = f"{case.ident()} [bounded]", case.K, case.epi
    b_acc = (3 * 2.0 ** -16 + 3 * K * 2.0 ** -23) * ops.S
    if epi == QKV:
        worst = max(G._compare(f"{what} {nm}", "bounded", outs[nm], ops.P[:, lo:lo + R.D], b_acc[:, lo:lo + R.D], False, 0.0) for nm, lo in (("q", 0), ("k", R.D), ("v", 2 * R.D)))
    else:
        ref = R.epilogue(epi, ops.P, ex["bias"], ex["resid"], 0.5)
        bound = R.epilogue_bound(epi, ops.P, b_acc) * (0.5 if epi == RESID else 1.0)
        if epi in (SILU, GLU):
            bound = bound + G.EXPF_REL * np.abs(ref)
        worst = G._compare(what, "bounded", outs["act"] if epi in R.ACT_OUT else outs["f32"][0], ref, bound, False, 0.0)
    print(f"RATIO {what} {worst:.4f}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.ident())
def test_split_gemm_matches_the_float64_product(gpu_harness, case):
    if case.epi in EXACT_EPIS:
        G.run_case(gpu_harness, case, "exact")
    if case.K <= 96:
        _bounded(gpu_harness, case)


def _split_operands(M, N, K):
    """operands whose hi / lo split has no residue, and the float64 sum of the three products the kernel keeps"""
    ops = G.Operands(True, "split", M, N, K)
    rng = G._rng("split", M, N, K)
    for name, shape in (("A", (M, K)), ("W", (N, K))):
        setattr(ops, name, (rng.choice([-3, -2, 2, 3], shape) + rng.integers(-3, 4, shape) / 1024.0).astype(np.float32))
    (ah, al), (wh, wl) = [(R.bf16_round(x), R.bf16_round(x - R.bf16_round(x))) for x in (ops.A, ops.W)]
    assert np.array_equal(ah + al, ops.A) and np.array_equal(wh + wl, ops.W) and np.abs(al).max() == 3 / 1024 and np.abs(ah).min() == 2          # the split is exact
    ah, al, wh, wl = [x.astype(np.float64) for x in (ah, al, wh, wl)]
    ops._P = ah @ wh.T + ah @ wl.T + al @ wh.T
    assert np.array_equal(ops._P.astype(np.float32).astype(np.float64), ops._P) and np.abs(ops._P).max() < 2 ** 14
    assert not np.array_equal(ops._P, ops.A.astype(np.float64) @ ops.W.astype(np.float64).T)          # ... and is not the full product
    return ops


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(65, 128, 64), (65, 128, 96), (65, 128, 1024), (257, 2048, 64), (1537, 2048, 64)])
def test_split_gemm_keeps_exactly_the_three_products(gpu_harness, M, N, K):
    G._OPERANDS[(True, "split", M, N, K)] = ops = _split_operands(M, N, K)
    case = _c(M, N, K, epi=PART)
    _, outs, _, _ = G.launch(gpu_harness, case, "split")
    G._compare(f"{case.ident()} [split-exact]", "exact", outs["f32"][0], ops.P, None, False, 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,epi", [(257, 2048, 96, PART), (70, 3072, 64, QKV)])
def test_split_gemm_bits_do_not_depend_on_the_tile_form(gpu_harness, M, N, K, epi):          # the rule's choice and the three forced forms
    runs = [G.launch(gpu_harness, _c(M, N, K, epi=epi, T=14), "bounded")[1] if f == 0 else
            G.launch(gpu_harness, replace(_c(M, N, K, epi=epi, T=14), opts=G._o(f32_fma_tile=2 + 16 * f)), "bounded")[1] for f in range(4)]
    for other in runs[1:]:
        for k, v in runs[0].items():
            assert np.array_equal(v.view(np.uint32), other[k].view(np.uint32)), k
