"""float64 references of the TitaNet-L side-car's operations (kernels_spk.hip, kernels_diar.hip from k_spk_depthwise on), numpy only.

Activations are [S][160][C], channels innermost; lens [S] are the valid frames of each sub-segment.  Every function takes and returns float64 and knows nothing
about tiles, waves or accumulation order: tests/spk_kernel_cases.py builds operands, float32 restatements and bound terms on top, tests/test_spk_kernel_ref.py
checks these functions against direct loops on small shapes."""
from __future__ import annotations

import numpy as np

T, TVALID, NMEL = 160, 150, 80
U24 = 2.0 ** -24          # unit roundoff of f32
BF16_REL = 2.0 ** -8      # a bf16 store, relative to the stored value


def f64(x):
    return np.asarray(x, np.float64)


def mask(lens):
    """[S][160][1] bool: frame t of segment s is valid"""
    return (np.arange(T)[None, :] < np.asarray(lens)[:, None])[:, :, None]


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-f64(z)))


def pointwise(a, w, bias, lens, relu=False, masked=True):
    """pointwise conv a [S][160][K] . w [N][K]^T + bias (+ ReLU), frames >= L zero (MaskedConv1d) when `masked`"""
    y = np.einsum("stk,nk->stn", f64(a), f64(w)) + f64(bias)
    if relu:
        y = np.maximum(y, 0.0)
    return np.where(mask(lens), y, 0.0) if masked else y


def pointwise_abs(a, w, bias):
    """sum |a| |w| + |bias|: what a rounding bound of the product multiplies"""
    return np.einsum("stk,nk->stn", np.abs(f64(a)), np.abs(f64(w))) + np.abs(f64(bias))


def depthwise(x, w, lens):
    """'same' depthwise conv along time, taps w [k][C]: input frames >= L read as zero, output frames >= L are zero"""
    x, w = f64(x), f64(w)
    k = w.shape[0]
    pad = (k - 1) // 2
    m = mask(lens)
    xp = np.pad(np.where(m, x, 0.0), ((0, 0), (pad, pad), (0, 0)))
    out = np.zeros_like(x)
    for i in range(k):
        out += xp[:, i:i + T, :] * w[i][None, None, :]
    return np.where(m, out, 0.0)


def colmean(y, lens):
    """masked mean over time [S][C]"""
    return np.where(mask(lens), f64(y), 0.0).sum(1) / f64(lens)[:, None]


def combine(y, z, r, lens, mask_out=False):
    """relu(mask(y) * sigmoid(z) + r); r None = no residual; mask_out: frames >= L of the result are zero (the bf16 engine's X), else relu(r) stands there"""
    m = mask(lens)
    v = np.where(m, f64(y), 0.0) * sigmoid(z)[:, None, :]
    if r is not None:
        v = v + f64(r)
    v = np.maximum(v, 0.0)
    return np.where(m, v, 0.0) if mask_out else v


def stats(x, lens):
    """masked mean and std over time: std = sqrt(clamp(mean((x - mean)^2), 1e-10, 1e30))"""
    m = mask(lens)
    L = f64(lens)[:, None]
    mean = np.where(m, f64(x), 0.0).sum(1) / L
    var = np.where(m, (f64(x) - mean[:, None, :]) ** 2, 0.0).sum(1) / L
    return mean, np.sqrt(np.clip(var, 1e-10, 1e30))


def featnorm(mel):
    """per-feature normalisation over the 150 valid frames: (x - mean) / (std + 1e-5), std Bessel-corrected; mel [S][>= 150][80] -> [S][150][80]"""
    x = f64(mel)[:, :TVALID, :]
    mean = x.mean(1, keepdims=True)
    std = np.sqrt(((x - mean) ** 2).sum(1, keepdims=True) / (TVALID - 1))
    return (x - mean) / (std + 1e-5)


def asp(x, logits, lens, sc, bi):
    """attentive statistics pooling with folded BN: softmax of the logits over the valid frames per channel, weighted mean and std (variance clamped at 1e-10)
    of x, pool [S][2 C] = (mu * sc[:C] + bi[:C] ; sigma * sc[C:] + bi[C:]).  Also returns (weights, mu, var) for the bounds."""
    x, lg = f64(x), f64(logits)
    C = x.shape[2]
    m = mask(lens)
    lg = np.where(m, lg, -np.inf)
    e = np.exp(lg - lg.max(1, keepdims=True))
    wgt = e / e.sum(1, keepdims=True)
    xm = np.where(m, x, 0.0)
    mu = (wgt * xm).sum(1)
    var = (wgt * (xm - mu[:, None, :]) ** 2).sum(1)
    sigma = np.sqrt(np.maximum(var, 1e-10))
    sc, bi = f64(sc), f64(bi)
    return np.concatenate([mu * sc[:C] + bi[:C], sigma * sc[C:] + bi[C:]], 1), (wgt, mu, var)


def linear(x, w, b, relu=False):
    """the small linears: x [M][K] . w [N][K]^T + b"""
    y = f64(x) @ f64(w).T + f64(b)
    return np.maximum(y, 0.0) if relu else y


def att_const(mean, stdv, w1, b1):
    """the per-segment constant of the attention conv: w1 [A][3 C], c[s][a] = w1[a][C:2C] . mean[s] + w1[a][2C:] . std[s] + b1[a]"""
    C = np.asarray(mean).shape[1]
    w1 = f64(w1)
    return f64(mean) @ w1[:, C:2 * C].T + f64(stdv) @ w1[:, 2 * C:].T + f64(b1)


def att_post(g, c, sc, bi):
    """tanh(BN(relu(g + c))): g [S][160][A], c [S][A]"""
    return np.tanh(np.maximum(f64(g) + f64(c)[:, None, :], 0.0) * f64(sc) + f64(bi))


# ---- bf16 (round to nearest even) on the host, as nasr_internal.h's f32_to_bf16 ------------------------------------------------------------------
def bf16_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_values(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_values(bf16_bits(x))
