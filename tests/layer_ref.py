"""Float64 reference of the non-GEMM operations of one cached conformer layer, as the reference model defines them (not as the kernels of
nemotron-asr.cpp_amd/csrc/kernels_layer.hip and kernels_fused.hip index them).  numpy only, no GPU.

Every function takes the kernel's own inputs of ONE stream and ONE chunk, operands already rounded to the type the kernel reads them in:
  * post        x + scale * sum of the split-K partials, then the optional LayerNorms           (reference src/nemo-stream.cpp:580-591, :633-634, :687)
  * attention   cached relative-position attention: (q + u) . K and (q + v) . P, the rel-shift written as the reference's pad-and-reshape,
                the -1e9 validity mask, softmax, P . V                                           (:419-461, :463-573, :1037-1043)
  * dwconv      cached causal depthwise conv + LayerNorm + SiLU, and the new conv cache           (:336-412, :671-674)
The caller cuts the logical windows out of the rings (`ring_window`): the keys of chunk g of a launch are the 70 + T ring rows from
kv_head + g T, with the validity min(valid_len + g T, 70) that chunk would have seen.
Products and bf16 rounding are tests/gemm_ref.py's.  tests/test_layer_ref.py pins this file against the oracle; tests/test_gpu_layer_kernels.py
compares the kernels with it."""
from __future__ import annotations

import numpy as np

from tests import gemm_ref as R

D, NH, DH, LCTX, KVC = 1024, 8, 128, R.LCTX, R.KVC
LN_EPS = 1e-5
MASK = -1e9


def layer_norm(x, w, b) -> np.ndarray:
    """LayerNorm over the last axis: biased variance, eps 1e-5"""
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + LN_EPS) * np.asarray(w, dtype=np.float64) + np.asarray(b, dtype=np.float64)


def post(x, part=None, scale=0.0, ln1=None, ln2=None):
    """x [M][1024], part [splits][M][1024] or None -> (x', a): x' = [LN1](x + scale * sum_s part[s]), a = LN2(x') or None; ln = (weight, bias)"""
    x = np.asarray(x, dtype=np.float64)
    if part is not None and len(part):
        x = x + float(scale) * np.asarray(part, dtype=np.float64).sum(0)
    if ln1 is not None:
        x = layer_norm(x, *ln1)
    return x, (layer_norm(x, *ln2) if ln2 is not None else None)


def rel_shift(x, klen) -> np.ndarray:
    """x [qlen][pos_len] -> [qlen][klen], the reference's pad-and-reshape (build_cached_rel_shift): one zero column in front, the buffer read as
    [pos_len + 1][qlen], its first row dropped, read as [qlen][pos_len] again, the first klen columns kept"""
    x = np.asarray(x)
    qlen, pos_len = x.shape
    padded = np.concatenate([np.zeros((qlen, 1), x.dtype), x], axis=1)
    back = padded.reshape(pos_len + 1, qlen)[1:].reshape(qlen, pos_len)
    return back[:, :klen]


def rel_shift_index(x, klen) -> np.ndarray:
    """the same as an index map: out[i][j] = x[i][j + qlen - 1 - i]; with position row r <-> rel = (70 + qlen - 1) - r that is rel = (70 + i) - j"""
    x = np.asarray(x)
    qlen = x.shape[0]
    i, j = np.arange(qlen)[:, None], np.arange(klen)[None, :]
    return x[i, j + qlen - 1 - i]


def ring_window(pool_half, head, n) -> np.ndarray:
    """rows head .. head + n - 1 (mod KVC) of a [KVC][1024] ring"""
    return np.asarray(pool_half)[(int(head) + np.arange(n)) % KVC]


def attention_weights(q, K, P, bias_u, bias_v, valid_len):
    """q [T][1024] f32 values, K [70 + T][1024] keys in logical order, P [70 + 2 T - 1][1024] position rows (row r <-> rel = (70 + T - 1) - r),
    bias_u / bias_v [1024] -> (weights [8][T][70 + T], unmasked [70 + T] bool, score parts for the error bound)"""
    q, K, P = (np.asarray(a, dtype=np.float64) for a in (q, K, P))
    T, KV = q.shape[0], K.shape[0]
    assert KV == LCTX + T and P.shape[0] == KV + T - 1
    valid = min(int(valid_len), LCTX)
    unmasked = np.arange(KV) >= LCTX - valid
    qu = q + np.asarray(bias_u, dtype=np.float64).reshape(1, D)
    qv = q + np.asarray(bias_v, dtype=np.float64).reshape(1, D)
    w = np.zeros((NH, T, KV))
    for h in range(NH):
        sl = slice(h * DH, (h + 1) * DH)
        s = (qu[:, sl] @ K[:, sl].T + rel_shift(qv[:, sl] @ P[:, sl].T, KV)) / np.sqrt(float(DH))
        s = s + np.where(unmasked, 0.0, MASK)[None, :]
        e = np.exp(s - s.max(-1, keepdims=True))
        w[h] = e / e.sum(-1, keepdims=True)
    return w, unmasked, (qu, qv)


def attention(q, K, V, P, bias_u, bias_v, valid_len) -> np.ndarray:
    """the context rows [T][1024] of one chunk of one stream"""
    w, _, _ = attention_weights(q, K, P, bias_u, bias_v, valid_len)
    V = np.asarray(V, dtype=np.float64)
    return np.concatenate([w[h] @ V[:, h * DH:(h + 1) * DH] for h in range(NH)], axis=1)


def dwconv_taps(cache, glu, dw):
    """cache [ks - 1][1024], glu [T][1024], dw [ks][1024] -> (conv [T][1024], new cache [ks - 1][1024] = the last ks - 1 rows of [cache ; glu])"""
    z = np.concatenate([np.asarray(cache), np.asarray(glu)]).astype(np.float64)
    dw = np.asarray(dw, dtype=np.float64)
    ks, T = dw.shape[0], len(glu)
    assert len(cache) == ks - 1
    conv = sum(z[k:k + T] * dw[k] for k in range(ks))
    return conv, np.concatenate([np.asarray(cache), np.asarray(glu)])[T:]


def dwconv(cache, glu, dw, ln_w, ln_b):
    """-> (silu(LayerNorm(conv)) [T][1024], new cache)"""
    conv, new_cache = dwconv_taps(cache, glu, dw)
    return R.silu(layer_norm(conv, ln_w, ln_b)), new_cache


# ---- error bounds of the f32 kernels against these float64 values ---------------------------------------------------------------------------
U32 = 2.0 ** -24          # unit roundoff of f32


def layer_norm_bound(x, w, b, dx=0.0) -> np.ndarray:
    """|f32 two-pass LayerNorm - layer_norm| per element, for an input row known to |dx| (derivation: tests/test_gpu_layer_kernels.py)"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    mu = x.mean(-1, keepdims=True)
    d = x - mu
    var = (d ** 2).mean(-1, keepdims=True)
    sd = np.sqrt(var + LN_EPS)
    dx = np.broadcast_to(np.asarray(dx, dtype=np.float64), x.shape)
    e_mu = (n + 1) * U32 * np.abs(x).mean(-1, keepdims=True) + dx.mean(-1, keepdims=True)   # the mean: an n-term f32 sum in any order, one multiply
    e_d = e_mu + U32 * np.abs(d) + dx                                            # one subtraction
    e_var = (2 * np.abs(d) * e_d).mean(-1, keepdims=True) + (n + 3) * U32 * var  # squares of perturbed terms; n-term sum, square, multiply
    e_inv = (e_var / (2 * sd ** 2) + 4 * U32) / sd                               # d(1/sqrt(v)) = -dv / (2 v^1.5); sqrt, add, divide
    y = d / sd
    e_y = e_d / sd + np.abs(d) * e_inv + U32 * np.abs(y)
    w, b = np.abs(np.asarray(w, dtype=np.float64)), np.asarray(b, dtype=np.float64)
    out = y * np.asarray(w) + b
    return e_y * w + 2 * U32 * (np.abs(y) * w + np.abs(out))
