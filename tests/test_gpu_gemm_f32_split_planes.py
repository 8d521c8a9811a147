"""k_gemm_f32_split_planes (GemmParams::f32_fma_tile = 3, engine option "f32_split_planes") and k_split_weight_planes alone, through launch_gemm_f32 and
tests/helpers/gemm_planes_harness.hip: the split GEMM whose weight operand arrives as bf16 hi / lo planes.
  plane   row n, 32-deep chunk c = 64 B hi of k = 32 c .. + 31, then 64 B lo: `==` the numpy split hi = RNE_bf16(x), lo = RNE_bf16(x - hi).
  bits    kind 3's output `==` kind 2's (k_gemm_f32_split on the f32 weights), in the launcher's tile rule and in every forced form.
  bounded K <= 96: |got - float64 product| <= (3 2^-16 + 3 K 2^-23) |A| |W|^T, the derived bound of tests/test_gpu_gemm_f32_split.py.
Operands are that file's bounded mode: A ~ N(0, 1), W ~ U(+-sqrt(3 / K)), unrounded f32."""
import ctypes as C

import numpy as np
import pytest

from tests import gemm_ref as R
from tests import test_gpu_gemm_kernels as G

HELPER = G.ROOT / "tests" / "helpers" / "libgemm_planes_harness.so"
#        M, N, K, lda (0: K), forced tile form (0: the rule; 1: 128 x 128, 2: 64 x 128, 3: 64 x 64)
CASES = ([(5, 128, 64, 0, 0), (64, 128, 64, 0, 0), (65, 128, 96, 0, 0), (65, 64, 32, 0, 0), (65, 128, 96, 104, 0)]          # <64,64>; one chunk and N % 128 != 0; a row pitch
         + [(257, 2048, 96, 0, f) for f in range(4)]                                                                        # the rule (<64,64>, 160 workgroups) and each form
         + [(1537, 2048, 64, 0, 0)])                                                                                        # the rule takes <64,128>


@pytest.fixture(scope="module")
def lib():
    assert HELPER.exists(), "tests/helpers/libgemm_planes_harness.so not built (python __graft_entry__.py)"
    C.CDLL(str(G.ENGINE_LIB), mode=C.RTLD_GLOBAL)
    L = C.CDLL(str(HELPER))
    L.gemm_planes_error.restype = C.c_char_p
    L.gemm_planes_run.argtypes = [C.c_int] + [C.c_void_p] * 2 + [C.c_int] * 5 + [C.c_void_p] * 3
    return L


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,lda,force", CASES, ids=lambda v: str(v))
def test_planes_gemm_has_the_split_kernels_bits(lib, M, N, K, lda, force):
    ops = G.operands(True, "bounded", M, N, K)
    lda = lda or K
    A = np.full((M, lda), np.nan, np.float32)          # the columns past K are never read
    A[:, :K] = ops.A
    out2, out3, plane = np.empty((M, N), np.float32), np.empty((M, N), np.float32), np.empty((N, K // 32, 2, 32), np.uint16)
    rc = lib.gemm_planes_run(0, A.ctypes.data, ops.W.ctypes.data, M, N, K, lda, force, out2.ctypes.data, out3.ctypes.data, plane.ctypes.data)
    assert rc == 0, lib.gemm_planes_error().decode()
    hi = R.bf16_round(ops.W)
    want = np.stack([R.bf16_bits(hi).reshape(N, K // 32, 32), R.bf16_bits(ops.W - hi).reshape(N, K // 32, 32)], axis=2).astype(np.uint16)
    assert np.array_equal(plane, want)
    assert np.isfinite(out3).all() and np.array_equal(out3.view(np.uint32), out2.view(np.uint32))
    if K <= 96:
        ratio = (np.abs(out3.astype(np.float64) - ops.P) / ((3 * 2.0 ** -16 + 3 * K * 2.0 ** -23) * ops.S)).max()
        print(f"RATIO planes {M}x{N}x{K} form {force}: {ratio:.4f}")
        assert ratio <= 1.0
