"""Float64 reference of the GEMMs of nemotron-asr.cpp_amd/csrc/kernels_gemm.hip: out = epilogue(A . W^T).  numpy only, no GPU.

What is taken from the source, and where:
  * bf16 rounding: `f32_to_bf16` (nasr_internal.h) -- round to nearest even on the upper 16 bits, NaN kept NaN (quiet bit set);
  * the A row map: `a_row_ptr` (nasr_epilogue.h);
  * K slices of a split-K launch: slice s of `splits` is the chunks [C s / splits, C (s + 1) / splits) (integer division) of C = K / unit chunks;
    unit = 32 in k_gemm_skinny, 64 in the LDS-tiled kernels (`k_slice`); partial slabs are [split][M][ldo];
  * the epilogues: `epi_quad` (nasr_epilogue.h) and `epi_elem_f32` (kernels_gemm.hip), applied here in float64 to the float64 sum;
  * the K / V ring row of batch row b, frame i: (kv_head[b] + LCTX + i) mod KVC in slot rows[b].slot, pool layout [slot][2][KVC][1024].
tests/test_gemm_ref.py pins this file; tests/test_gpu_gemm_kernels.py compares the kernels with it."""
from __future__ import annotations

import numpy as np

D, LCTX, MAXNEW = 1024, 70, 256
KVC = LCTX + MAXNEW

EPI_PART_F32, EPI_SILU_ACT, EPI_QKV, EPI_GLU, EPI_BIAS_F32, EPI_BIAS_RELU_ACT, EPI_BIAS_RELU_F32, EPI_BIAS_ACT, EPI_RESID_F32 = range(9)
EPI_NAMES = ["PART_F32", "SILU_ACT", "QKV", "GLU", "BIAS_F32", "BIAS_RELU_ACT", "BIAS_RELU_F32", "BIAS_ACT", "RESID_F32"]
ACT_OUT = (EPI_SILU_ACT, EPI_BIAS_RELU_ACT, EPI_BIAS_ACT)          # epilogues whose output has the activation dtype (out_act)
HAS_BIAS = (EPI_BIAS_F32, EPI_BIAS_RELU_ACT, EPI_BIAS_RELU_F32, EPI_BIAS_ACT)


# ---- bf16 ----------------------------------------------------------------------------------------------------------------------
def bf16_bits(x) -> np.ndarray:
    """f32 -> the 16 bits f32_to_bf16 gives: RNE, NaN -> (u >> 16) | 0x40"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_to_f32(bits) -> np.ndarray:
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x) -> np.ndarray:
    """f32 -> the nearest bf16 value (ties to even), as f32"""
    return bf16_to_f32(bf16_bits(x))


# ---- operands ------------------------------------------------------------------------------------------------------------------
def a_row_offsets(M, lda, rows_per_batch=0, batch_stride=0, row_offset=0) -> np.ndarray:
    """element offset of row m of the A operand (a_row_ptr)"""
    m = np.arange(M, dtype=np.int64)
    if rows_per_batch > 0:
        b, i = m // rows_per_batch, m % rows_per_batch
        return b * batch_stride + (row_offset + i) * lda
    return m * lda


def k_slice_bounds(K, splits, unit) -> list[int]:
    """k boundaries of the K slices: splits + 1 values from 0 to (K // unit) * unit"""
    c = K // unit
    return [(c * s // splits) * unit for s in range(splits + 1)]


def product(A, W) -> np.ndarray:
    """A [M][K] . W [N][K]^T in float64"""
    return np.asarray(A, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T


def product_slices(A, W, bounds) -> np.ndarray:
    """[splits][M][N]: the product over each K slice"""
    A, W = np.asarray(A, dtype=np.float64), np.asarray(W, dtype=np.float64)
    return np.stack([A[:, k0:k1] @ W[:, k0:k1].T for k0, k1 in zip(bounds[:-1], bounds[1:])])


def abs_product(A, W) -> np.ndarray:
    """S = |A| . |W|^T: the scale of the rounding-error bound of the sum"""
    return np.abs(np.asarray(A, dtype=np.float64)) @ np.abs(np.asarray(W, dtype=np.float64)).T


# ---- epilogues, in float64 -------------------------------------------------------------------------------------------------------
def sigmoid(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def silu(x):
    return np.asarray(x, dtype=np.float64) * sigmoid(x)


def glu(acc) -> np.ndarray:
    """columns (2c, 2c + 1) = (value c, gate c) -> [M][N / 2]"""
    return acc[:, 0::2] * sigmoid(acc[:, 1::2])


def ring_rows(kv_head, T) -> np.ndarray:
    """[B][T] ring row of frame i of batch row b"""
    r = np.asarray(kv_head, dtype=np.int64)[:, None] + LCTX + np.arange(T, dtype=np.int64)[None, :]
    return np.where(r >= KVC, r - KVC, r)


def kv_index(M, T, slot, kv_head):
    """(slot [M], ring row [M]) of GEMM row m = b T + i"""
    m = np.arange(M)
    b, i = m // T, m % T
    return np.asarray(slot, dtype=np.int64)[b], ring_rows(kv_head, T)[b, i]


def epilogue(epi, acc, bias=None, resid=None, resid_scale=0.0) -> np.ndarray:
    """the epilogue's value for the complete K sum acc [M][N] (EPI_PART_F32 with one slice and EPI_QKV: acc itself; the caller places the QKV columns)"""
    acc = np.asarray(acc, dtype=np.float64)
    if epi in (EPI_PART_F32, EPI_QKV):
        return acc
    if epi == EPI_SILU_ACT:
        return silu(acc)
    if epi == EPI_GLU:
        return glu(acc)
    if epi in (EPI_BIAS_F32, EPI_BIAS_ACT):
        return acc + np.asarray(bias, dtype=np.float64)[None, :]
    if epi in (EPI_BIAS_RELU_F32, EPI_BIAS_RELU_ACT):
        return np.maximum(acc + np.asarray(bias, dtype=np.float64)[None, :], 0.0)
    if epi == EPI_RESID_F32:
        return float(resid_scale) * acc + np.asarray(resid, dtype=np.float64)
    raise ValueError(epi)


def epilogue_bound(epi, acc, b_acc) -> np.ndarray:
    """|epilogue(x) - epilogue(acc)| for |x - acc| <= b_acc, to first order with the derivative bounds |silu'| <= 1.1 and |v sigmoid'(g)| <= |v| / 4;
    the linear epilogues pass b_acc through (ReLU is 1-Lipschitz; EPI_RESID_F32's factor is applied by the caller)"""
    if epi == EPI_SILU_ACT:
        return 1.1 * b_acc
    if epi == EPI_GLU:
        return b_acc[:, 0::2] + np.abs(acc[:, 0::2]) / 4.0 * b_acc[:, 1::2]
    return b_acc
