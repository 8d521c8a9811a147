"""k_attention_f32_split (kernels_attn_split.hip) alone: launch_attention with act_bf16 = 2 through tests/helpers/layer_harness.hip, f32 buffers, on the
setups, selector cases and conventions of tests/test_gpu_layer_kernels.py (poison, sentinels, ownership: see there; for a non-zero integer the harness sizes
its range checks for 2-byte elements, so with f32 buffers it under-checks, never refuses).  Selector mode (`==`): operands exact in bf16, every lo part zero,
every softmax one-hot: the context row is the selected V row bit for bit.  Bounded mode: unrounded f32 operands against float64,
    |got - ref| <= (2 . 6 Delta + omega + EXPF_REL) sum_j w_j |V_jd| + 2^-23 |ref|,    nothing measured on the kernel:
  Delta = 2^-16 (|q + u| . |K| + |q + v| . |Pos| shifted) / sqrt(128), largest over the row's unmasked keys; 6: three dropped terms of a split product, each
  <= 2^-16 |a||b|, and 3 . 128 . 2^-23 for the accumulation of three products; omega = 3 . 2^-16 + 3 (70 + T) 2^-23 + 2 . 2^-23: the P.V
  split, its accumulation, the normalisation.  Two operand mixes: bounded_case's, and that with K scaled by 2^-4 (the position term is nearly all of Delta).
Scratch mutants dropping one lo product each (not committed), worst ratio over the cases below, first mix / position-heavy (the kernel: 0.011 / 0.022):
K_lo (q+u)_hi 1.32 / 0.15, K_hi (q+u)_lo 1.59 / 0.16, Pos_lo (q+v)_hi 1.63 / 2.65, Pos_hi (q+v)_lo 1.50 / 2.45, V_lo w_hi 2.61 / 4.84, V_hi w_lo 2.17 / 4.43:
all six leave the bound, the content mutants in the first mix only."""
import ctypes as C

import numpy as np
import pytest
from tests import layer_ref as LR
from tests.test_gpu_gemm_kernels import EXPF_REL
from tests.test_gpu_layer_kernels import (D, DH, LCTX, NH, AttnCase, AttnSetup, Dev, _no_handles, _selector_runs, act_bits, act_values, bounded_case,
                                          rest_is_sentinel, selector_case, slack_rows)

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 3), (1, 16), (1, 18), (2, 4), (2, 22), (7, 7), (7, 14), (14, 14), (14, 42), (14, 252)]


def run(dev: Dev, s: AttnSetup, q, Kv, Vv, P, bu, bv):
    M = s.B * s.TS
    c = _no_handles(AttnCase())
    c.q = dev.up(q, slack_rows(M) * D * 4)
    c.kv_pool, c.n_slots, c.act_bf16 = dev.up(s.pool(Kv, Vv, False)), s.n_slots, 2          # AttnParams::act_bf16 = 2: f32 operands on the split-bf16 kernel
    c.posproj = dev.up(act_bits(P, False))
    c.bias_u, c.bias_v, c.rows = dev.up(bu), dev.up(bv), dev.up(s.rows())
    c.B, c.T, c.TS = s.B, s.T, s.TS
    c.ctx_out = dev.new((M + slack_rows(M)) * D * 4)
    assert dev.L.layer_harness_attention(C.byref(c)) == 0, dev.err()
    out = dev.get(c.ctx_out, np.uint32)
    rest_is_sentinel(out, M * D, "ctx_out")
    got = act_values(out[:M * D], False).reshape(M, D)
    assert np.all(np.isfinite(got)), "a context element is not finite (unwritten, or poison reached it)"
    return got


@pytest.mark.parametrize("T,TS", SHAPES)
def test_selector(T, TS):
    for rn, seed, target in _selector_runs():
        s = AttnSetup(3, T, TS, rot=seed)
        q, Kv, Vv, P, bu, bv, exp = selector_case(s, rn, seed, target)
        with Dev() as dev:
            got = run(dev, s, q, Kv, Vv, P, bu, bv)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, f"{rn} seed {seed} target {target}: {len(bad)} elements differ, first (row, column) {bad[0]}: got {got[tuple(bad[0])]}, want {exp[tuple(bad[0])]}"


def reference(s: AttnSetup, q, Kv, Vv, P, bu, bv):
    T, scale = s.T, 1.0 / np.sqrt(float(DH))
    omega = 3 * 2.0 ** -16 + 3 * (LCTX + T) * 2.0 ** -23 + 2 * 2.0 ** -23
    ref, bound = np.zeros((s.B * s.TS, D)), np.zeros((s.B * s.TS, D))
    for b, g, v, offs, unm in s.chunks():
        rows = slice(b * s.TS + g * T, b * s.TS + (g + 1) * T)
        K, V = Kv[b, offs].astype(np.float64), Vv[b, offs].astype(np.float64)
        w, _, (qu, qv) = LR.attention_weights(q[rows], K, P, bu, bv, v)
        for h in range(NH):
            sl = slice(h * DH, (h + 1) * DH)
            a = np.abs(qu[:, sl]) @ np.abs(K[:, sl]).T + LR.rel_shift(np.abs(qv[:, sl]) @ np.abs(P[:, sl].astype(np.float64)).T, LCTX + T)
            delta = (scale * 2.0 ** -16 * a)[:, unm].max(-1)
            ref[rows, sl] = w[h] @ V[:, sl]
            bound[rows, sl] = (12 * delta + omega + EXPF_REL)[:, None] * (w[h] @ np.abs(V[:, sl]))
    return ref, bound + 2.0 ** -23 * np.abs(ref)


@pytest.mark.parametrize("k_scale", [1.0, 2.0 ** -4], ids=["mix", "position-heavy"])
@pytest.mark.parametrize("T,TS", SHAPES)
def test_bounded(T, TS, k_scale):
    s = AttnSetup(3, T, TS)
    q, Kv, Vv, P, bu, bv, _, _ = bounded_case(s, False, "f32")
    Kv = (Kv * np.float32(k_scale)).astype(np.float32)
    ref, bound = reference(s, q, Kv, Vv, P, bu, bv)
    with Dev() as dev:
        got = run(dev, s, q, Kv, Vv, P, bu, bv)
    err = np.abs(got - ref)
    print(f"k_attention_f32_split T {T} TS {TS} K x {k_scale}: worst |got - ref| / bound = {(err / bound).max():.3f}")
    assert np.all(err <= bound), f"worst ratio {(err / bound).max()} at {np.unravel_index(np.argmax(err / bound), err.shape)}"
