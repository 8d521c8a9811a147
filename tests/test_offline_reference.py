"""Pins tests/offline_ref.py, the numpy restatement of the reference's offline encoder that tests/test_gpu_offline.py trusts:
to OracleModel.layer_chunk0 (= the reference's offline layer, tests/test_oracle_golden.py) where that may be called (T <= 64),
and to the compiled reference beyond (where oracle/_ref exists)."""
import numpy as np
import pytest

from oracle import binding as ob
from tests import offline_ref as orf


@pytest.fixture(scope="module")
def model1(weights1):
    return ob.OracleModel(weights1, 1)


@pytest.mark.parametrize("T", [1, 16, 64])
def test_layer_equals_layer_chunk0(model1, weights1, T):
    x = np.random.default_rng(T).standard_normal((T, 1024)).astype(np.float32)
    assert np.abs(orf.layer(weights1, 0, x) - model1.layer_chunk0(0, x)).max() < 2e-4


@pytest.mark.parametrize("T", [129, 300])
def test_layer_equals_compiled_reference(weights1, T):
    if not ob.have_ref():
        pytest.skip("oracle/_ref not built (no reference sources on this machine)")
    x = np.random.default_rng(T).standard_normal((T, 1024)).astype(np.float32)
    assert np.abs(orf.layer(weights1, 0, x) - ob.ref_conformer_layer(weights1, 0, x)).max() < 2e-3


def test_position_rows_equal_reference_table():
    tab = orf.pos_table()
    assert tab.shape == (4095, 1024)
    if ob.have_ref():
        assert np.abs(tab - ob.ref_pos_emb(2048)).max() < 1e-5
    assert np.array_equal(orf.pos_slice(5), np.stack([ob.pos_emb(4 - i) for i in range(9)]))


def test_one_layer_twenty_seconds_decodes_like_reference(model1, weights1):
    rng = np.random.default_rng(20)
    mel = rng.standard_normal((2000, 128)).astype(np.float32)         # 20 s of 10 ms frames
    sub, outs, enc = orf.encode(model1, weights1, mel, 1)
    assert sub.shape[0] == orf.enc_frames(2000) == 251
    toks, frames = orf.greedy(model1, enc)
    assert len(toks) == len(frames) and frames == sorted(frames) and (not frames or frames[-1] < 251)
    if ob.have_ref():
        assert np.abs(sub - ob.ref_subsampling(weights1, mel)).max() < 1e-3
        assert toks == ob.ref_greedy(weights1, enc)
