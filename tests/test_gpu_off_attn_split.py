"""k_off_attn_f32_split (kernels_attn_split.hip) alone: launch_off_attention with the integer 2 through tests/helpers/offline_harness.hip, f32 buffers,
against the cases, the float64 reference and the conventions of tests/test_gpu_offline_kernels.py (layouts, sentinels, ownership: see there).  For a
non-zero integer the harness sizes its own range checks for 2-byte elements; the f32 buffers uploaded here are twice that, so it under-checks, never refuses.

Selector mode (`==`): every operand is exact in bf16, so every lo part is zero, every product and sum exact, every softmax one-hot: the context row
equals the selected V row bit for bit.  Covers indexing, masking, the band skew, the 64-key block boundaries and table rows 0 and 4094 (T = 2048).

Bounded mode: unrounded f32 operands (`bounded_case(T, False)`: rho = 0, so its Delta is the f32 kernel's, scale 2^-16 (|q + u| . |K| + |q + v| . |Pos|)).
The bound is DESIGN section 23's per product, carried through the softmax as for the other attention kernels; nothing is measured on the kernel:
    |got - ref| <= (2 . 6 Delta + omega + EXPF_REL) sum_j w_j |V_jd| + 2^-23 |ref|
  6 Delta: the three dropped terms of a score product are each <= 2^-16 |a||b| and the three products' f32 accumulation is 3 K 2^-23 = 3 . 2^-16 at K = 128.
  omega = 3 . 2^-16 + 3 T 2^-23 + ceil(T / 64) 2^-23: the split of P.V, its accumulation over T keys in three products, one rescale per key block.
About 20 x below k_off_attn_bf16's bound.  Checked once with scratch mutants that drop one lo product each (worst ratio over the T below; the kernel: 0.012):
K_lo (q+u)_hi 3.59, K_hi (q+u)_lo 1.15 (T = 63 only), V_lo p_hi 2.97 and V_hi p_lo 1.77 leave the bound; Pos_lo (q+v)_hi 0.87 and Pos_hi (q+v)_lo 0.78 stay inside."""
import ctypes as C

import numpy as np
import pytest

from tests.offline_kernel_cases import BOUNDED_T, SELECTOR_BATCHES, Packed, bounded_case, selector_case, selector_runs
from tests.test_gpu_gemm_kernels import EXPF_REL
from tests.test_gpu_layer_kernels import Dev, act_bits, act_values
from tests.test_gpu_offline_kernels import D, DH, MAX_T, QKV_LD, SLACK, AttnCase, dev, harness, owned_rows_only

pytestmark = pytest.mark.gpu
KIND = 2          # launch_off_attention's integer: f32 operands on the split-bf16 kernel


def run(dv: Dev, lay: Packed, qkv, pos, bu, bv, only=None):
    """one launch -> context rows [M][1024], NaN where not launched; ownership checked"""
    M, qb = lay.M, harness().offline_harness_attn_qb(KIND)
    assert qb == 64
    items = lay.items(qb, only)
    c = AttnCase()
    c.qkv, c.pos = dv.up(act_bits(qkv, False), SLACK * QKV_LD * 4), dv.up(act_bits(pos, False))
    c.bias_u, c.bias_v, c.items, c.n_items = dv.up(bu), dv.up(bv), dv.up(items), len(items)
    c.ctx, c.M, c.act_bf16 = dv.new((M + SLACK) * D * 4), M, KIND
    assert dv.L.offline_harness_attention(C.byref(c)) == 0, dv.err()
    out = dv.get(c.ctx, np.uint32)
    out = out[:(len(out) // D) * D].reshape(-1, D)
    owned = np.zeros(len(out), bool)
    owned[:M] = lay.rows_of(only)
    owned_rows_only(out, owned, "ctx")
    got = np.full((M, D), np.nan, np.float32)
    got[owned[:M]] = act_values(out[:M][owned[:M]].reshape(-1), False).reshape(-1, D)
    assert np.all(np.isfinite(got[owned[:M]])), "a context element is not finite (unwritten, or poison reached it)"
    return got


@pytest.mark.parametrize("Ts", SELECTOR_BATCHES + [(MAX_T,)], ids=str)
def test_selector(Ts):
    lay = Packed(Ts)
    for rn, seed, target in selector_runs((0,) if Ts == (MAX_T,) else (0, 1, 2)):
        qkv, pos, bu, bv, exp = selector_case(lay, rn, seed, target)
        with dev() as dv:
            got = run(dv, lay, qkv, pos, bu, bv)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, f"T {Ts} {rn} seed {seed} target {target}: {len(bad)} elements differ, first (row, column) {bad[0]}: got {got[tuple(bad[0])]}, want {exp[tuple(bad[0])]}"


@pytest.mark.parametrize("T", BOUNDED_T + (MAX_T,))
def test_bounded(T):
    lay, k, qkv, pos, bu, bv, rows, ref, delta, wabsv = bounded_case(T, False)
    omega = 3 * 2.0 ** -16 + 3 * T * 2.0 ** -23 + -(-T // 64) * 2.0 ** -23
    bound = np.repeat(12 * delta + omega + EXPF_REL, DH, axis=1) * wabsv + 2.0 ** -23 * np.abs(ref)
    with dev() as dv:
        got = run(dv, lay, qkv, pos, bu, bv, only=[k])
    err = np.abs(got[lay.offs[k] + rows] - ref)
    print(f"k_off_attn_f32_split T {T}: worst |got - ref| / bound = {(err / bound).max():.3f}")
    assert np.all(err <= bound), f"worst ratio {(err / bound).max()} at {np.unravel_index(np.argmax(err / bound), err.shape)}"
