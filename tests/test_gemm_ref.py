"""Pins tests/gemm_ref.py, the float64 reference tests/test_gpu_gemm_kernels.py compares the GEMM kernels with.  No GPU."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import gemm_ref as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def test_bf16_rounding_ties_subnormals_and_infinities():
    # ties go to the even 16-bit pattern; just above / below a tie go to the nearer one
    assert R.bf16_bits(_f32([0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF])).tolist() == [0x3F80, 0x3F82, 0x3F81, 0x3F81]
    # the largest finite f32 rounds up to +inf, as the source's integer addition does; +-inf and +-0 stay
    assert R.bf16_bits(_f32([0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000])).tolist() == [0x7F80, 0x7F80, 0xFF80, 0x0000, 0x8000]
    # f32 subnormals: 0x00008000 is a tie between bf16 0x0000 (even) and 0x0001; 0x00018000 between 0x0001 and 0x0002 (even)
    assert R.bf16_bits(_f32([0x00008000, 0x00018000, 0x00008001, 0x007FFFFF, 0x80008001])).tolist() == [0x0000, 0x0002, 0x0001, 0x0080, 0x8001]
    # NaN stays NaN whatever its payload (a payload in the low half only must not round to inf)
    assert R.bf16_bits(_f32([0x7F800001, 0x7FC00000, 0xFFFFFFFF])).tolist() == [0x7FC0, 0x7FC0, 0xFFFF]
    x = np.array([1.0, -2.5, 3.0e38, 1e-40], dtype=np.float32)
    assert np.array_equal(R.bf16_round(R.bf16_round(x)), R.bf16_round(x))
    assert R.bf16_round(np.float32([257.0]))[0] == 256.0 and R.bf16_round(np.float32([259.0]))[0] == 260.0      # 8 significant bits


def test_bf16_rounding_equals_f32_to_bf16_of_the_source(tmp_path):
    """the same bits as nasr::f32_to_bf16 (nasr_internal.h), compiled for the host, on edge patterns and 200 000 random ones"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text(
        "#pragma once\n#include <cstring>\ntypedef struct ihipStream_t *hipStream_t;\n#define __device__\n#define __forceinline__ inline\n"
        "static inline float __uint_as_float(unsigned u) { float f; memcpy(&f, &u, 4); return f; }\n"
        "static inline unsigned __float_as_uint(float f) { unsigned u; memcpy(&u, &f, 4); return u; }\n")
    (tmp_path / "cvt.cpp").write_text(
        '#include "nasr_internal.h"\n#include <cstdio>\n'
        "int main() { unsigned u; while (fread(&u, 4, 1, stdin) == 1) { float f; memcpy(&f, &u, 4); unsigned short b = nasr::f32_to_bf16(f); fwrite(&b, 2, 1, stdout); } return 0; }\n")
    subprocess.check_call([cxx, "-std=c++17", "-O1", f"-I{tmp_path}", f"-I{CSRC}", f"-I{ROOT / 'include'}", str(tmp_path / "cvt.cpp"), "-o", str(tmp_path / "cvt")])
    rng = np.random.default_rng(7)
    edge = np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0x00008000, 0x00018000, 0x007FFFFF,
                     0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001], dtype=np.uint32)
    u = np.concatenate([edge, rng.integers(0, 2**32, 200000, dtype=np.uint64).astype(np.uint32), (rng.integers(0, 2**16, 4096, dtype=np.uint32) << 16) | 0x8000])
    out = subprocess.run([str(tmp_path / "cvt")], input=u.tobytes(), capture_output=True, check=True).stdout
    assert np.array_equal(np.frombuffer(out, dtype=np.uint16), R.bf16_bits(u.view(np.float32)))


def test_glu_pairs_even_value_with_odd_gate():
    acc = np.array([[2.0, 0.0, -3.0, 50.0, 5.0, -50.0]])
    got = R.epilogue(R.EPI_GLU, acc)
    assert got.shape == (1, 3)
    np.testing.assert_allclose(got[0], [2.0 * 0.5, -3.0 * 1.0, 5.0 * 0.0], atol=1e-12)
    # the bound: the value's own error, plus the gate's through |v| / 4
    b = R.epilogue_bound(R.EPI_GLU, acc, np.full_like(acc, 1e-3))
    np.testing.assert_allclose(b[0], [1e-3 * (1 + 2 / 4), 1e-3 * (1 + 3 / 4), 1e-3 * (1 + 5 / 4)])


def test_kv_ring_wraps_at_kvc():
    assert R.KVC == 326
    rows = R.ring_rows([0, 249, 255, 256, 325], 14)
    assert rows[0].tolist() == list(range(70, 84))
    assert rows[1].tolist() == list(range(319, 326)) + list(range(0, 7))          # wraps inside the chunk
    assert rows[2, 0] == 325 and rows[2, 1] == 0
    assert rows[3, 0] == 0 and rows[4, 0] == 69
    assert rows.min() >= 0 and rows.max() < R.KVC
    slot, ring = R.kv_index(5, 2, [7, 3, 9], [325, 0, 255])
    assert slot.tolist() == [7, 7, 3, 3, 9] and ring.tolist() == [69, 70, 70, 71, 325]


def test_row_map_follows_a_row_ptr():
    assert R.a_row_offsets(3, 40).tolist() == [0, 40, 80]
    # rows_per_batch 2, batch_stride 1000, row_offset 2, lda 100: row m -> (m / 2) * 1000 + (2 + m % 2) * 100
    assert R.a_row_offsets(5, 100, 2, 1000, 2).tolist() == [200, 300, 1200, 1300, 2200]


@pytest.mark.parametrize("K,splits,unit", [(1024, 8, 32), (1024, 4, 64), (256, 4, 64), (512, 2, 64), (96, 2, 32), (4352, 4, 64), (192, 4, 64)])
def test_k_slices_tile_k_and_sum_to_the_product(K, splits, unit):
    b = R.k_slice_bounds(K, splits, unit)
    assert b[0] == 0 and b[-1] == K and all(x <= y for x, y in zip(b, b[1:])) and all(x % unit == 0 for x in b)
    rng = np.random.default_rng(K + splits)
    A, W = rng.integers(-3, 4, (5, K)).astype(np.float64), rng.integers(-3, 4, (16, K)).astype(np.float64)
    parts = R.product_slices(A, W, b)
    assert parts.shape == (splits, 5, 16)
    assert np.array_equal(parts.sum(axis=0), R.product(A, W))          # integers: exact in any order
    assert np.all(R.abs_product(A, W) >= np.abs(R.product(A, W)))


def test_k_slices_of_the_kernels():
    assert R.k_slice_bounds(1024, 8, 32) == [0, 128, 256, 384, 512, 640, 768, 896, 1024]
    assert R.k_slice_bounds(192, 4, 64) == [0, 0, 64, 128, 192]          # 3 chunks over 4 slices: the first slice is empty (integer division, as k_slice)
    assert R.k_slice_bounds(96, 2, 32) == [0, 32, 96]


def test_linear_epilogues():
    acc, bias, resid = np.array([[1.0, -4.0]]), np.array([0.5, 1.0]), np.array([[10.0, 20.0]])
    assert R.epilogue(R.EPI_BIAS_F32, acc, bias).tolist() == [[1.5, -3.0]]
    assert R.epilogue(R.EPI_BIAS_RELU_ACT, acc, bias).tolist() == [[1.5, 0.0]]
    assert R.epilogue(R.EPI_RESID_F32, acc, resid=resid, resid_scale=0.5).tolist() == [[10.5, 18.0]]
    np.testing.assert_allclose(R.epilogue(R.EPI_SILU_ACT, np.array([[0.0, 1.0]])), [[0.0, 1.0 / (1.0 + np.exp(-1.0))]])
