"""Engine option "f32_split" through the C ABI: an F32 engine whose encoder GEMMs above four rows run as three bf16 MFMA products of split operands
(k_gemm_f32_split).  Two layers of the speech checkpoint, 6 streams (6 and 84 rows per step): layer taps within the tolerances of
tests/test_gpu_parity.py::test_f32_engine_matches_f32_oracle, tokens and emission frames equal to the F32 oracle's, and bits that do not depend on the
batch: a stream stepped alone (R = 13: 14 rows, still the split kernel) or in another, larger batch (R = 0, where a stream alone is one row and takes
the <= 4-row f32 kernel, by design another arithmetic) gives the same encoder output.  One offline call gives the offline oracle's output and tokens."""
import numpy as np
import pytest

from nemotron_asr_amd import capi, synth
from oracle import binding as ob
from tests import offline_ref as orf
from tests.test_gpu_parity import N_LAYERS, _acc

pytestmark = pytest.mark.gpu
TOL_SUB, TOL_LAYER, B = 1e-3, 2e-3, 6          # the arguments of _compare_chunks in test_f32_engine_matches_f32_oracle (the offline test asserts 2e-3 too)


@pytest.fixture(scope="module")
def model():
    W = synth.make_weights(N_LAYERS, margins="speech")
    return W, ob.OracleModel(W, N_LAYERS)


def _engine(W, n_streams):
    eng = capi.Engine(W, n_layers=N_LAYERS, dtype=capi.DTYPE_F32, max_streams=n_streams)
    for v in (-1, 2, 16):          # 0 and 1, nothing else
        with pytest.raises(capi.NasrError, match="0 or 1"):
            eng.set_option("f32_split", v)
    eng.set_option("f32_split", 0)
    eng.set_option("f32_split", 1)
    eng.set_debug(True)
    return eng


def _run(model, pcms, R, order):
    """steps streams `order` of pcms as one batch -> per stream: tokens, frames, encoder output of every step; stream order[0] against the oracle"""
    piece, T = synth.shift_samples(R), 1 + R
    eng = _engine(model[0], len(order))
    sts = [eng.stream(R) for _ in order]
    toks, encs, worst, ref = {b: [] for b in order}, {b: [] for b in order}, dict(sub=0.0, layer=0.0), []
    ost = ob.OracleStream(model[1], R)
    sub_tap, lay_tap = ost.enable_taps()
    for k in range(pcms[0].size // piece):
        for st, b, t in zip(sts, order, eng.step(sts, [pcms[b][k * piece:(k + 1) * piece] for b in order])):
            toks[b] += t
            encs[b].append(st.tap(capi.TAP_ENCODER_OUT).reshape(-1, 1024)[:T].copy())
        ref += ost.process(pcms[order[0]][k * piece:(k + 1) * piece])
        assert sts[0].stats().chunks == ost.total_chunks
        if ost.total_chunks:
            worst["sub"] = _acc(worst["sub"], sts[0].tap(capi.TAP_SUBSAMPLED).reshape(T, 1024) - sub_tap)
            for l in range(N_LAYERS):
                worst["layer"] = _acc(worst["layer"], sts[0].tap(capi.TAP_LAYER_OUT, l).reshape(T, 1024) - lay_tap[l])
    with pytest.raises(capi.NasrError, match="before the first"):          # the arithmetic of an engine is fixed once it has stepped
        eng.set_option("f32_split", 0)
    for b, t in zip(order, eng.finalize(sts)):
        toks[b] += t
    frames = {b: st.token_frames() for st, b in zip(sts, order)}
    assert ost.total_chunks >= 4 and worst["sub"] < TOL_SUB and worst["layer"] < TOL_LAYER, worst
    assert toks[order[0]] == ref + ost.finalize() and frames[order[0]] == ost.token_frames()
    eng.close()
    return toks, frames, encs


@pytest.mark.parametrize("R", [0, 13])
def test_split_engine_matches_the_oracle_and_batch_equals_alone(model, R):
    piece, n_steps = synth.shift_samples(R), 5 if R else 30          # 5.6 s / 2.4 s of audio
    pcms = [synth.make_speech_pcm(b, n_steps * piece / 16000.0 + 0.1)[0][:n_steps * piece] for b in range(2 * B)]
    toks, frames, encs = _run(model, pcms, R, list(range(B)))
    for order in ([[0], [B - 1]] if R >= 4 else [list(range(2 * B))[::-1]]):          # alone where that is still more than four rows, else among twice as many streams
        t2, f2, e2 = _run(model, pcms, R, order)
        for b in set(order) & set(range(B)):
            assert t2[b] == toks[b] and f2[b] == frames[b], b
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(encs[b], e2[b])), b


def test_split_engine_offline_call_gives_the_oracle_tokens(model):
    W, om = model
    pcms = [synth.make_speech_pcm(u, s)[0] for u, s in ((0, 1.3), (1, 2.1))]
    eng = _engine(W, 2)
    toks, frames = eng.transcribe(pcms)
    for u, p in enumerate(pcms):
        mel = ob.OraclePreproc(W["preprocessor.featurizer.fb"], W["preprocessor.featurizer.window"]).process(p)
        enc = orf.encode(om, W, mel, N_LAYERS)[2]
        assert enc.shape[0] > 4          # above four rows: the split kernel
        assert _acc(0.0, eng.offline_tap(capi.TAP_ENCODER_OUT, u) - enc) < TOL_LAYER
        assert (toks[u], frames[u]) == orf.greedy(om, enc)
    with pytest.raises(capi.NasrError, match="before the first"):          # ... or has run an offline call
        eng.set_option("f32_split", 0)
    eng.close()
