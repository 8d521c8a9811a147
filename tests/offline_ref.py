"""Numpy restatement of the reference's OFFLINE encoder (test infrastructure, not product code).

The reference's `nemo_encode` (src/nemo-ggml.cpp:1038-1079) runs ConvSubsampling over the whole mel (no drop-2), then every
conformer layer with full-context relative-position attention (build_rel_pos_mha :668-755: no mask, no cache; the score of
query i and key j reads the position row of rel = i - j from the T-centred slice of the sinusoid table) and a depthwise conv
from a zero history, then prompt fusion (:1087-1105).  OracleModel.layer_chunk0 is this layer at T <= 64 but must not be called
beyond (its score array holds 70 + 64 keys), so this module states it for any T <= 2048 in float64.  tests/test_offline_reference.py
pins it to layer_chunk0 and to the compiled reference.
"""
from __future__ import annotations

import numpy as np

from oracle import binding as ob

MAX_FRAMES = 2048
_TABLE = None


def sub_len(n: int) -> int:
    return n // 2 + 1


def enc_frames(n_mel: int) -> int:
    return 0 if n_mel <= 0 else sub_len(sub_len(sub_len(n_mel)))


def pos_table() -> np.ndarray:
    """[4095][1024] sinusoid rows, row r <-> relative position 2047 - r (the oracle's pos_emb, = the reference's compute_pos_emb)"""
    global _TABLE
    if _TABLE is None:
        _TABLE = np.stack([ob.pos_emb(MAX_FRAMES - 1 - r) for r in range(2 * MAX_FRAMES - 1)]).astype(np.float32)
    return _TABLE


def pos_slice(T: int) -> np.ndarray:
    """the 2T - 1 rows of relative positions T-1 .. -(T-1)"""
    return pos_table()[MAX_FRAMES - T: MAX_FRAMES + T - 1]


def _ln(x, w, b):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + 1e-5) * w + b


def _silu(x):
    return x / (1.0 + np.exp(-x))


def _w(weights, name):
    return np.asarray(weights[name], np.float64)


def rel_pos_attention(q, k, v, pos, bias_u, bias_v) -> np.ndarray:
    """the attention of `layer`: q, k, v [T][8][128], pos [2 T - 1][8][128] (relative positions T-1 .. -(T-1)), biases [8][128] -> context [T][1024]"""
    T, H, dh = q.shape
    qu = q + bias_u[None]
    qv = q + bias_v[None]
    quh, qvh, kh, vh = (t.transpose(1, 0, 2) for t in (qu, qv, k, v))          # [H][T][dh]
    ac = quh @ kh.transpose(0, 2, 1)                                            # [H][i][j]
    bd_full = qvh @ pos.transpose(1, 2, 0)                                      # [H][i][r]
    i_idx, j_idx = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    bd = bd_full[:, i_idx, j_idx + T - 1 - i_idx]
    s = (ac + bd) / np.sqrt(dh)
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    w = e / e.sum(-1, keepdims=True)
    return (w @ vh).transpose(1, 0, 2).reshape(T, H * dh)


def layer(weights: dict, l: int, x: np.ndarray, kernel_size: int = 9) -> np.ndarray:
    """ConformerLayer::forward on all T rows of one utterance, float64; returns float32"""
    p = f"encoder.layers.{l}."
    W = lambda k: _w(weights, p + k)  # noqa: E731
    x = np.asarray(x, np.float64).copy()
    T, D = x.shape
    H, dh = 8, 128

    def ffn(n, i):
        h = _ln(x, W(f"norm_feed_forward{i}.weight"), W(f"norm_feed_forward{i}.bias"))
        return _silu(h @ W(f"feed_forward{i}.linear1.weight").T) @ W(f"feed_forward{i}.linear2.weight").T

    x = x + 0.5 * ffn(None, 1)
    a = _ln(x, W("norm_self_att.weight"), W("norm_self_att.bias"))
    q = (a @ W("self_attn.linear_q.weight").T).reshape(T, H, dh)
    k = (a @ W("self_attn.linear_k.weight").T).reshape(T, H, dh)
    v = (a @ W("self_attn.linear_v.weight").T).reshape(T, H, dh)
    pos = (pos_slice(T).astype(np.float64) @ W("self_attn.linear_pos.weight").T).reshape(2 * T - 1, H, dh)
    ctx = rel_pos_attention(q, k, v, pos, W("self_attn.pos_bias_u"), W("self_attn.pos_bias_v"))
    x = x + ctx @ W("self_attn.linear_out.weight").T
    a = _ln(x, W("norm_conv.weight"), W("norm_conv.bias"))
    y = a @ W("conv.pointwise_conv1.weight").T
    g = y[:, :D] / (1.0 + np.exp(-y[:, D:]))
    ks1 = kernel_size - 1
    z = np.concatenate([np.zeros((ks1, D)), g])
    dw = W("conv.depthwise_conv.weight")                       # [ks][D]
    c = sum(z[kk:kk + T] * dw[kk] for kk in range(kernel_size))
    c = _silu(_ln(c, W("conv.batch_norm.weight"), W("conv.batch_norm.bias")))
    x = x + c @ W("conv.pointwise_conv2.weight").T
    x = x + 0.5 * ffn(None, 2)
    x = _ln(x, W("norm_out.weight"), W("norm_out.bias"))
    return x.astype(np.float32)


def prompt_fuse(weights: dict, x: np.ndarray, prompt: int, num_prompts: int) -> np.ndarray:
    idx = prompt if 0 <= prompt < num_prompts else 0
    w1 = _w(weights, "prompt_kernel.0.weight")               # [2048][1024 + P]
    h = np.asarray(x, np.float64) @ w1[:, :1024].T + w1[:, 1024 + idx] + _w(weights, "prompt_kernel.0.bias")
    h = np.maximum(h, 0.0)
    return (h @ _w(weights, "prompt_kernel.2.weight").T + _w(weights, "prompt_kernel.2.bias")).astype(np.float32)


def encode(model: ob.OracleModel, weights: dict, mel: np.ndarray, n_layers: int, prompt: int = -1, num_prompts: int = 0):
    """whole-utterance encoder: (subsampled [T][1024], [layer outputs], encoder output)"""
    sub = model.subsampling(mel)
    assert sub.shape[0] == enc_frames(mel.shape[0])
    x, outs = sub, []
    for l in range(n_layers):
        x = layer(weights, l, x)
        outs.append(x)
    enc = prompt_fuse(weights, x, prompt, num_prompts) if num_prompts > 0 else x
    return sub, outs, enc


def greedy(model: ob.OracleModel, enc: np.ndarray, prompt: int = -1):
    """the reference's greedy decode (blank start, <= 10 symbols per frame, first maximum) -> (tokens, frames from 0)"""
    st = ob.OracleStream(model, 0, prompt)
    toks = st.decode(enc)
    return toks, st.token_frames()[:len(toks)]
