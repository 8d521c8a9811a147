"""Float64 reference of the operations of nemotron-asr.cpp_amd/csrc/kernels_offline.hip, as the reference model defines them (not as the kernels
index them).  numpy only, no GPU.  Operands arrive already rounded to the type the kernel reads them in.

  * attention   full-context relative-position attention of ONE utterance and ONE head (reference src/nemo-ggml.cpp:668-755):
                score(i, j) = ((q_i + u) . K_j + (q_i + v) . Pos[j - i + 2047]) / sqrt(128), softmax over j < T, times V.  The position row of
                (i, j) is gathered by that index; no pad-and-reshape rel-shift is involved.
  * dwconv      causal depthwise conv from a zero history, LayerNorm, SiLU: tests/layer_ref.py's dwconv with a zero cache (:1038-1079).
  * conv_front  conv0 (3x3, stride 2, 1 -> 256 channels) + ReLU + depthwise 3x3 stride 2, pads 2 before / 1 after on both axes (:905-913,
                :936-943, :969-978), on a whole [n_mel][128] utterance -> [H2][33][256], H1 = n_mel // 2 + 1, H2 = H1 // 2 + 1.
tests/test_offline_kernel_ref.py pins this file; tests/test_gpu_offline_kernels.py compares the kernels with it."""
from __future__ import annotations

import numpy as np

from tests import layer_ref as LR

DH, MAX_T = 128, 2048
NREL = 2 * MAX_T - 1            # rows of the position table, row r <-> rel = i - j = 2047 - r
NMEL, SUBC, W1, W2 = 128, 256, 65, 33


def pos_scores(qv, pos, rows, T) -> np.ndarray:
    """qv [n][128] (query rows `rows` of the utterance), pos [4095][128] -> [n][T]: element (i, j) = qv_i . pos[j - rows[i] + 2047]"""
    qv, pos, rows = np.asarray(qv, dtype=np.float64), np.asarray(pos, dtype=np.float64), np.asarray(rows)
    assert pos.shape[0] == NREL and 1 <= T <= MAX_T and rows.min() >= 0 and rows.max() < T
    lo = MAX_T - T                                            # the table rows an utterance of T frames can address: 2047 - (T - 1) .. 2047 + (T - 1)
    full = qv @ pos[lo:lo + 2 * T - 1].T                      # [n][2 T - 1]
    idx = np.arange(T)[None, :] - rows[:, None] + (MAX_T - 1)
    return np.take_along_axis(full, idx - lo, axis=1)


def attention(q, K, V, pos, bias_u, bias_v, rows=None):
    """q, K, V [T][128] of one utterance and head, pos [4095][128], bias_u / bias_v [128]; rows: the query rows wanted (all by default)
    -> (context [n][128], weights [n][T], (q + u, q + v) of those rows)"""
    q, K, V = (np.asarray(a, dtype=np.float64) for a in (q, K, V))
    T = K.shape[0]
    rows = np.arange(T) if rows is None else np.asarray(rows)
    qu = q[rows] + np.asarray(bias_u, dtype=np.float64)[None, :]
    qv = q[rows] + np.asarray(bias_v, dtype=np.float64)[None, :]
    s = (qu @ K.T + pos_scores(qv, pos, rows, T)) / np.sqrt(float(DH))
    e = np.exp(s - s.max(-1, keepdims=True))
    w = e / e.sum(-1, keepdims=True)
    return w @ V, w, (qu, qv)


def attention_loops(q, K, V, pos, bias_u, bias_v) -> np.ndarray:
    """the same, one (i, j) at a time: the definition read aloud, for small T (tests/test_offline_kernel_ref.py pins `attention` to it)"""
    T = len(K)
    out = np.zeros((T, DH))
    for i in range(T):
        s = np.array([(np.dot(q[i] + bias_u, K[j]) + np.dot(q[i] + bias_v, pos[j - i + 2047])) / np.sqrt(128.0) for j in range(T)], np.float64)
        e = np.exp(s - s.max())
        out[i] = (e / e.sum()) @ np.asarray(V, np.float64)
    return out


def dwconv(glu, dw, ln_w, ln_b):
    """glu [T][1024] of one utterance, dw [ks][1024] -> (silu(LayerNorm(conv)) [T][1024], conv [T][1024]); the history in front of frame 0 is zero"""
    ks = np.asarray(dw).shape[0]
    zero = np.zeros((ks - 1, np.asarray(glu).shape[1]), np.float32)
    out, _ = LR.dwconv(zero, glu, dw, ln_w, ln_b)
    conv, _ = LR.dwconv_taps(zero, glu, dw)
    return out, conv


def sub_len(n: int) -> int:
    return n // 2 + 1


def conv3x3_s2(x, w, b, depthwise: bool) -> np.ndarray:
    """x [H][W] (one input channel) or [H][W][C] (depthwise), w [C][3][3], b [C] -> [H // 2 + 1][W // 2 + 1][C]: stride 2, 2 rows / columns of zeros in
    front and 1 behind"""
    x, w, b = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64).reshape(-1, 3, 3), np.asarray(b, dtype=np.float64)
    if not depthwise:
        x = x[:, :, None]
    H, W = x.shape[:2]
    Ho, Wo = sub_len(H), sub_len(W)
    xp = np.zeros((H + 3, W + 3, x.shape[2]))
    xp[2:2 + H, 2:2 + W] = x
    out = np.zeros((Ho, Wo, w.shape[0]))
    for kh in range(3):
        for kw in range(3):
            out += xp[kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] * w[:, kh, kw]
    return out + b


def conv_front(mel, w0, b0, w2, b2, parts=False):
    """mel [n_mel][128], w0 / w2 [256][3][3] (the model's conv.0 / conv.2 weights), b0 / b2 [256] -> [H2][33][256]; n_mel = 0 gives no rows.
    parts: also the conv0 activations [H1][65][256]"""
    mel = np.asarray(mel, dtype=np.float64).reshape(-1, NMEL)
    if mel.shape[0] == 0:
        return (np.zeros((0, W2, SUBC)), np.zeros((0, W1, SUBC))) if parts else np.zeros((0, W2, SUBC))
    a0 = np.maximum(conv3x3_s2(mel, w0, b0, depthwise=False), 0.0)
    out = conv3x3_s2(a0, w2, b2, depthwise=True)
    return (out, a0) if parts else out
