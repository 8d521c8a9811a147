"""Pins tests/offline_kernel_ref.py (CPU, no GPU), and checks with the references alone what tests/test_gpu_offline_kernels.py expects of the kernels:
the attention against its own definition one (i, j) at a time and against tests/offline_ref.py's layer attention; the conv front against the oracle's
whole subsampling (orf.encode's `sub`: the oracle exposes no conv stage, so the remaining stages -- pointwise conv3 + ReLU, depthwise conv5, pointwise
conv6 + ReLU, the flatten and the output linear -- are completed here in float64 on top of offline_kernel_ref.conv_front); the selector expectations
against the float64 attention of the same operands; the bounded cases' Delta_i and peakedness conditions at every shape.  The cases are tests/offline_kernel_cases.py's (numpy only)."""
import numpy as np
import pytest

from oracle import binding as ob
from tests import gemm_ref as R
from tests import offline_kernel_ref as OR
from tests import offline_ref as orf
from tests import offline_kernel_cases as G

D, NH, DH = 1024, 8, 128


def _operands(T, seed):
    rng = np.random.default_rng(seed)
    q, K, V = (rng.standard_normal((T, D)) for _ in range(3))
    pos = rng.standard_normal((OR.NREL, D))
    return q, K, V, pos, rng.standard_normal(D), rng.standard_normal(D)


@pytest.mark.parametrize("T", [1, 2, 5, 17])
def test_attention_is_its_definition_and_the_layer_attention(T):
    q, K, V, pos, bu, bv = _operands(T, T)
    ctx = np.zeros((T, D))
    for h in range(NH):
        sl = slice(h * DH, (h + 1) * DH)
        ctx[:, sl], w, _ = OR.attention(q[:, sl], K[:, sl], V[:, sl], pos[:, sl], bu[sl], bv[sl])
        assert w.shape == (T, T) and np.allclose(w.sum(-1), 1.0, rtol=0, atol=1e-12)
        assert np.abs(ctx[:, sl] - OR.attention_loops(q[:, sl], K[:, sl], V[:, sl], pos[:, sl], bu[sl], bv[sl])).max() < 1e-12
    # offline_ref.layer's attention takes the 2 T - 1 rows of rel = T - 1 .. -(T - 1): rows 2048 - T .. 2046 + T of the table
    sub = pos[OR.MAX_T - T:OR.MAX_T - 1 + T].reshape(2 * T - 1, NH, DH)
    want = orf.rel_pos_attention(q.reshape(T, NH, DH), K.reshape(T, NH, DH), V.reshape(T, NH, DH), sub, bu.reshape(NH, DH), bv.reshape(NH, DH))
    assert np.abs(ctx - want).max() < 1e-12


def test_attention_rows_subset():
    q, K, V, pos, bu, bv = _operands(40, 3)
    full, w, _ = OR.attention(q[:, :DH], K[:, :DH], V[:, :DH], pos[:, :DH], bu[:DH], bv[:DH])
    rows = np.array([0, 7, 39])
    part, wp, _ = OR.attention(q[:, :DH], K[:, :DH], V[:, :DH], pos[:, :DH], bu[:DH], bv[:DH], rows)
    assert np.abs(part - full[rows]).max() < 1e-12 and np.abs(wp - w[rows]).max() < 1e-12


def test_layer_is_unchanged_by_the_factored_attention(weights1):
    """offline_ref.layer gives the numbers it gave with the attention lines inline (they moved to rel_pos_attention unchanged): the oracle still agrees"""
    x = np.random.default_rng(16).standard_normal((16, 1024)).astype(np.float32)
    assert np.abs(orf.layer(weights1, 0, x) - ob.OracleModel(weights1, 1).layer_chunk0(0, x)).max() < 2e-4


def test_dwconv_has_a_zero_history():
    rng = np.random.default_rng(0)
    glu, dw, w, b = rng.standard_normal((5, D)), rng.standard_normal((3, D)), rng.standard_normal(D), rng.standard_normal(D)
    out, conv = OR.dwconv(glu, dw, w, b)
    assert np.allclose(conv[0], glu[0] * dw[2]) and np.allclose(conv[1], glu[0] * dw[1] + glu[1] * dw[2]) and np.allclose(conv[4], glu[2] * dw[0] + glu[3] * dw[1] + glu[4] * dw[2])
    assert np.allclose(out, R.silu(OR.LR.layer_norm(conv, w, b)))


@pytest.mark.parametrize("n_mel", [1, 9, 33, 70])
def test_conv_front_completes_to_the_oracle_subsampling(weights1, n_mel):
    """the comparison used: offline_ref.encode's `sub` (= OracleModel.subsampling, f32) against conv_front + the remaining stages in float64"""
    mel = np.random.default_rng(n_mel).standard_normal((n_mel, 128)).astype(np.float32)
    W = lambda k: np.asarray(weights1["encoder.pre_encode." + k], np.float64)  # noqa: E731
    x = OR.conv_front(mel, W("conv.0.weight"), W("conv.0.bias"), W("conv.2.weight"), W("conv.2.bias"))
    H1 = n_mel // 2 + 1
    assert x.shape == (H1 // 2 + 1, 33, 256)
    x = np.maximum(x @ W("conv.3.weight").reshape(256, 256).T + W("conv.3.bias"), 0.0)
    x = OR.conv3x3_s2(x, W("conv.5.weight"), W("conv.5.bias"), depthwise=True)
    x = np.maximum(x @ W("conv.6.weight").reshape(256, 256).T + W("conv.6.bias"), 0.0)           # [H3][17][256]
    flat = x.transpose(0, 2, 1).reshape(x.shape[0], 256 * 17)                                    # flat[t][c * 17 + w]
    want = flat @ W("out.weight").T + W("out.bias")
    sub = ob.OracleModel(weights1, 1).subsampling(mel)
    assert sub.shape == want.shape == (orf.enc_frames(n_mel), 1024)
    assert np.abs(sub - want).max() < 1e-3 * max(1.0, float(np.abs(want).max()))                 # f32 against float64 through five stages and a 4352-term sum
    assert OR.conv_front(mel[:0], W("conv.0.weight"), W("conv.0.bias"), W("conv.2.weight"), W("conv.2.bias")).shape == (0, 33, 256)


def test_conv_front_f32_restatement_is_the_reference():
    """the float32 operation-order restatement the GPU test holds k_off_conv0_dw<false> to, against the float64 reference within that test's bound"""
    s = G.SubSetup(seed=0)
    for k in s.tested:
        ref, bound = s.reference(k)
        if len(ref):
            got = G.conv_front_f32(s.utterance(k), s.wt(s.w0), s.b0, s.wt(s.w2), s.b2)
            assert got.dtype == np.float32 and np.all(np.abs(got - ref) <= bound)
            assert float(np.median(bound / np.maximum(np.abs(ref), 1e-30))) < 1e-4


# ---- what the GPU test expects, with the references alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ts", [(1, 15, 64, 2), (16, 129, 17), (3, 70, 5)])
def test_selector_expectation_is_the_float64_attention(Ts):
    lay = G.Packed(Ts)
    for run, seed, target in G.selector_runs(seeds=(0,)):
        qkv, pos, bu, bv, exp = G.selector_case(lay, run, seed, target)
        assert np.array_equal(R.bf16_round(qkv), qkv) and np.array_equal(R.bf16_round(pos), pos), "the operands are exact in bf16"
        assert set(np.unique(G.selector_ranks(lay, run, seed, target)[0])) == set(range(lay.M if run == "content" else OR.NREL))
        for off, T in zip(lay.offs, lay.Ts):
            for h in (0, 5):
                sl = slice(h * DH, (h + 1) * DH)
                ctx, w, _ = OR.attention(qkv[off:off + T, sl], qkv[off:off + T, D + h * DH:D + (h + 1) * DH], qkv[off:off + T, 2 * D + h * DH:2 * D + (h + 1) * DH],
                                         pos[:, sl], bu[sl], bv[sl])
                assert np.all(w.max(-1) == 1.0), "one-hot"
                assert np.array_equal(ctx.astype(np.float32), exp[off:off + T, sl]), (run, target, T, h)


def test_selector_targets_put_the_top_rank_where_they_say():
    lay = G.Packed((63, 200, 65))
    r = G.selector_ranks(lay, "content", 9, "first_rows")
    assert all(r[h, lay.offs[k] + lay.Ts[k]] > r[h, lay.offs[k]:lay.offs[k] + lay.Ts[k]].max() for h in range(NH) for k in (0, 1)), "row off + T outranks the utterance"
    assert all(np.argmax(r[h, lay.offs[k]:lay.offs[k] + lay.Ts[k]]) == 0 for h in range(NH) for k in range(3))
    r = G.selector_ranks(lay, "content", 9, "last_rows")
    assert all(r[h, lay.offs[k] - 1] > r[h, lay.offs[k]:lay.offs[k] + lay.Ts[k]].max() for h in range(NH) for k in (1, 2)), "row off - 1 outranks the utterance"
    assert all(np.argmax(r[h, lay.offs[k]:lay.offs[k] + lay.Ts[k]]) == lay.Ts[k] - 1 for h in range(NH) for k in range(3))
    for key in (63, 64):
        r = G.selector_ranks(lay, "content", 9, f"key{key}")
        assert [int(np.argmax(r[0, lay.offs[k]:lay.offs[k] + lay.Ts[k]])) for k in (1, 2)] == [key, key]
    # either order of the weights across key blocks occurs in the random seeds too: the winner in the first block, and behind it
    wins = [int(np.argmax(G.selector_ranks(lay, "content", s, None)[h, 63:263])) // 64 for s in G.SEEDS for h in range(NH)]
    assert 0 in wins and max(wins) > 0
    lay = G.Packed((OR.MAX_T,))
    assert all(np.argmax(G.selector_ranks(lay, "position", 9, "rel_plus")[h]) == 0 for h in range(NH))
    assert all(np.argmax(G.selector_ranks(lay, "position", 9, "rel_minus")[h]) == OR.NREL - 1 for h in range(NH))
    assert all(np.argmax(G.selector_ranks(lay, "position", 9, "rel_zero")[h]) == OR.MAX_T - 1 for h in range(NH))


@pytest.mark.parametrize("Ts", G.SELECTOR_BATCHES + [(OR.MAX_T,)])
def test_position_targets_decide_the_extreme_pairs_of_every_utterance(Ts):
    """for every T of every batch: under rel_plus query T - 1 selects key 0 (table row 2048 - T, which no shorter reach touches and no longer utterance's row
    outranks within this one's reach), under rel_minus query 0 selects key T - 1 (row 2046 + T), under rel_zero every query selects itself (row 2047)"""
    for T in Ts:
        i, j = np.arange(T)[:, None], np.arange(T)[None, :]
        win = {t: [np.argmax(G.selector_ranks(G.Packed(Ts), "position", 9, t)[h][j - i + OR.MAX_T - 1], axis=1) for h in range(NH)] for t in G.POSITION_TARGETS}
        for h in range(NH):
            assert win["rel_plus"][h][T - 1] == 0, (Ts, T, h)
            assert win["rel_minus"][h][0] == T - 1, (Ts, T, h)
            assert np.array_equal(win["rel_zero"][h], np.arange(T)), (Ts, T, h)


def test_v_marks_tell_any_two_frames_apart():
    v = G.v_marks(G.Packed((OR.MAX_T,)))
    assert np.array_equal(R.bf16_round(v), v)
    assert len(np.unique(v[:, :2], axis=0)) == OR.MAX_T


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("T", G.BOUNDED_T + (OR.MAX_T,))
def test_bounded_case_is_peaked_and_within_delta(T, bf16):
    """bounded_case asserts Delta_i <= 0.05 and a median largest weight >= 0.2 itself; here also: the bound stays a small part of the values"""
    lay, k, qkv, pos, bu, bv, rows, ref, delta, wabsv = G.bounded_case(T, bf16)
    bound = G.attention_bound(ref, delta, wabsv, T, bf16, 0.0)               # without the __expf allowance, which the GPU test adds
    assert lay.Ts[k] == T and len(rows) == (T if T < OR.MAX_T else 192) and ref.shape == bound.shape == (len(rows), D)
    assert float(np.median(bound)) < (0.15 if bf16 else 1e-3)
    if bf16:
        assert np.array_equal(R.bf16_round(qkv), qkv) and np.array_equal(R.bf16_round(pos), pos)
