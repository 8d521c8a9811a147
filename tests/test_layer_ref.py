"""Pins tests/layer_ref.py (CPU, no GPU): the rel-shift against its index form and the compiled reference, and one streaming conformer layer composed
from layer_ref operations and gemm_ref products against the oracle (OracleModel.layer_chunk0, OracleStream's layer tap and K / V / conv caches), at
kernel sizes 9 and 5.  The difference is float64 against the oracle's f32: asserted at the oracle's own ladder, 2e-3 per layer."""
import numpy as np
import pytest

from nemotron_asr_amd import synth
from oracle import binding as ob
from tests import gemm_ref as R
from tests import layer_ref as LR
from tests.golden import inputs as gi

LAYER_TOL = 2e-3


# ---- rel-shift ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 7, 14])
def test_rel_shift_is_the_index_form(T):
    KV, n_rel = 70 + T, 70 + 2 * T - 1
    # every element names its (query, position row): the value at row r is rel = (70 + T - 1) - r
    x = np.arange(T)[:, None] * 1000.0 + ((70 + T - 1) - np.arange(n_rel))[None, :]
    got = LR.rel_shift(x, KV)
    assert got.shape == (T, KV)
    assert np.array_equal(got, LR.rel_shift_index(x, KV))
    i, j = np.arange(T)[:, None], np.arange(KV)[None, :]
    assert np.array_equal(got, i * 1000.0 + (70 + i) - j)                      # rel = (70 + i) - j


@pytest.mark.parametrize("q", [1, 2, 7, 14])
def test_rel_shift_is_the_references(q):
    if not ob.have_ref() or not hasattr(ob.ref(), "ref_rel_shift"):
        pytest.skip("the compiled reference is not built on this machine")
    x = np.random.default_rng(q).standard_normal((8, q, 2 * q - 1)).astype(np.float32)
    want = ob.ref_rel_shift(x)
    for h in range(8):
        assert np.array_equal(LR.rel_shift(x[h], q), want[h])


# ---- the operations on small hand-made cases -------------------------------------------------------------------------------------------------
def test_layer_norm_and_post():
    rng = np.random.default_rng(0)
    x, part = rng.standard_normal((3, 1024)), rng.standard_normal((4, 3, 1024))
    w, b = rng.standard_normal(1024), rng.standard_normal(1024)
    xn, a = LR.post(x, part, 0.5, ln2=(w, b))
    assert np.allclose(xn, x + 0.5 * part.sum(0), rtol=0, atol=1e-12)
    y = (a - b) / w
    assert np.abs(y.mean(-1)).max() < 1e-12 and np.abs((y ** 2).mean(-1) - xn.var(-1) / (xn.var(-1) + 1e-5)).max() < 1e-12
    const, _ = LR.post(np.full((1, 1024), 3.0), None, ln1=(w, b))
    assert np.array_equal(const[0], b)                                         # variance 0: the bias


def test_attention_one_unmasked_key():
    """valid_len = 0, T = 1: only key 70 (the new row) is unmasked, whatever the scores"""
    rng = np.random.default_rng(1)
    q, K, V, P = rng.standard_normal((1, 1024)), rng.standard_normal((71, 1024)), rng.standard_normal((71, 1024)), rng.standard_normal((71, 1024))
    u, v = rng.standard_normal(1024), rng.standard_normal(1024)
    assert np.array_equal(LR.attention(q, K, V, P, u, v, 0), V[70:71])
    w, unmasked, _ = LR.attention_weights(q, K, P, u, v, 3)
    assert unmasked.sum() == 4 and np.all(w[:, :, :67] == 0) and np.allclose(w.sum(-1), 1)


def test_dwconv_cache_mixes_old_and_new_rows():
    rng = np.random.default_rng(2)
    for ks, T in ((9, 1), (9, 14), (5, 2), (32, 7)):
        cache, glu, dw = rng.standard_normal((ks - 1, 1024)), rng.standard_normal((T, 1024)), rng.standard_normal((ks, 1024))
        conv, new = LR.dwconv_taps(cache, glu, dw)
        z = np.concatenate([cache, glu])
        assert np.array_equal(new, z[-(ks - 1):]) and new.shape == cache.shape
        t, c = T - 1, 17
        assert np.isclose(conv[t, c], sum(z[t + k, c] * dw[k, c] for k in range(ks)), rtol=1e-12)


# ---- one streaming layer composed from layer_ref and gemm_ref --------------------------------------------------------------------------------
class RefLayer:
    """float64 streaming conformer layer: the launch sequence of the engine's layer with layer_ref's operations in the places of k_post, k_attention and
    k_dwconv and gemm_ref's products and epilogues in the places of the GEMMs; state = K / V windows (70 rows), validity, conv cache"""

    def __init__(self, W, layer, T, ks):
        self.g = lambda k: W[f"encoder.layers.{layer}.{k}"].astype(np.float64)
        self.T, self.ks = T, ks
        self.kc, self.vc, self.cc, self.valid = np.zeros((70, 1024)), np.zeros((70, 1024)), np.zeros((ks - 1, 1024)), 0
        rels = (70 + T - 1) - np.arange(70 + 2 * T - 1)
        emb = np.stack([ob.pos_emb(int(r)) for r in rels]).astype(np.float64)
        self.P = R.product(emb, self.g("self_attn.linear_pos.weight"))

    def ln(self, name):
        return self.g(name + ".weight"), self.g(name + ".bias")

    def ffn(self, x, which):
        _, a = LR.post(x, ln2=self.ln(f"norm_feed_forward{which}"))
        h = R.epilogue(R.EPI_SILU_ACT, R.product(a, self.g(f"feed_forward{which}.linear1.weight")))
        return LR.post(x, R.product(h, self.g(f"feed_forward{which}.linear2.weight"))[None], 0.5)[0]

    def step(self, x):
        g, T = self.g, self.T
        x = self.ffn(np.asarray(x, dtype=np.float64), 1)
        _, a = LR.post(x, ln2=self.ln("norm_self_att"))
        q = R.product(a, g("self_attn.linear_q.weight"))
        K = np.concatenate([self.kc, R.product(a, g("self_attn.linear_k.weight"))])
        V = np.concatenate([self.vc, R.product(a, g("self_attn.linear_v.weight"))])
        ctx = LR.attention(q, K, V, self.P, g("self_attn.pos_bias_u").reshape(-1), g("self_attn.pos_bias_v").reshape(-1), self.valid)
        self.kc, self.vc, self.valid = K[T:], V[T:], min(70, self.valid + T)
        x, a = LR.post(x, R.product(ctx, g("self_attn.linear_out.weight"))[None], 1.0, ln2=self.ln("norm_conv"))
        y = R.product(a, g("conv.pointwise_conv1.weight"))
        glu = y[:, :1024] * R.sigmoid(y[:, 1024:])
        c, self.cc = LR.dwconv(self.cc, glu, g("conv.depthwise_conv.weight"), *self.ln("conv.batch_norm"))
        x = LR.post(x, R.product(c, g("conv.pointwise_conv2.weight"))[None], 1.0)[0]
        x = self.ffn(x, 2)
        return LR.post(x, ln1=self.ln("norm_out"))[0]


@pytest.fixture(scope="module", params=[9, 5])
def model(request):
    ks = request.param
    W = synth.make_weights(n_layers=1, kernel_size=ks)
    return ks, W, ob.OracleModel(W, 1, kernel_size=ks)


@pytest.mark.parametrize("T", [1, 14])
def test_composed_layer_is_layer_chunk0(model, T):
    ks, W, om = model
    x = gi.layer_input(T)
    got = RefLayer(W, 0, T, ks).step(x)
    assert np.abs(got - om.layer_chunk0(0, x)).max() < LAYER_TOL


@pytest.mark.parametrize("R_ctx,n_chunks", [(0, 12), (13, 8)])
def test_composed_layer_is_the_oracle_stream(model, R_ctx, n_chunks):
    ks, W, om = model
    T = 1 + R_ctx
    st = ob.OracleStream(om, R_ctx)
    sub_tap, lay_tap = st.enable_taps()
    ref = RefLayer(W, 0, T, ks)
    mel = (np.random.default_rng(7).standard_normal((9 + 8 * T * n_chunks, 128)) * 2 - 4).astype(np.float32)
    for c in range(n_chunks):
        st.encode_chunk(mel[c * 8 * T: c * 8 * T + st.chunk_mel])
        got = ref.step(sub_tap)                                               # the oracle's own layer input of this chunk: no drift between the two
        assert np.abs(got - lay_tap[0]).max() < LAYER_TOL, c
        assert ref.valid == st.cache_valid_len
        for which, mine in ((0, ref.kc), (1, ref.vc), (2, ref.cc)):
            assert np.abs(mine - st.get_cache(which, 0)).max() < LAYER_TOL, (c, which)
