"""Engine option "f32_split_planes" through the C ABI: an F32 engine with "f32_split" whose split GEMMs read pre-split bf16 hi / lo weight planes
(k_gemm_f32_split_planes).  The planes hold the bits the split kernel forms in registers, so everything an engine with the option
computes equals, bit for bit, what an engine with "f32_split" alone computes: taps, tokens, emission frames; streaming (896 rows: W1 and QKV in 64 x 128
tiles, the rest in 64 x 64; 6 and 84 rows: the position projections of both chunk lengths) and offline.  Two layers of the speech checkpoint."""
import numpy as np
import pytest

from nemotron_asr_amd import capi, synth
from oracle import binding as ob
from tests.test_gpu_f32_split import TOL_LAYER, TOL_SUB
from tests.test_gpu_offline import mel_for
from tests.test_gpu_parity import N_LAYERS, _acc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def weights():
    return synth.make_weights(N_LAYERS, margins="speech")


def _engine(W, n_streams, planes, split=1, dtype=capi.DTYPE_F32):
    eng = capi.Engine(W, n_layers=N_LAYERS, dtype=dtype, max_streams=n_streams)
    eng.set_option("f32_split_planes", planes)          # before "f32_split": the planes are made when both are known, in either order
    eng.set_option("f32_split", split)
    eng.set_debug(True)
    on = planes and split and dtype == capi.DTYPE_F32          # the planes exist exactly where they are read: one more copy of the GEMM weights
    assert (eng.counter("weight_plane_bytes") > 4 * N_LAYERS * 12 * 1024 * 1024) == bool(on) and (on or eng.counter("weight_plane_bytes") == 0)
    return eng


def _stream_run(eng, pcms, R, oracle=None):
    """steps every stream through pcms -> (tokens, frames, [per step: taps of every stream]); with an oracle model, stream 0 against it"""
    piece, T, B = synth.shift_samples(R), 1 + R, len(pcms)
    sts = [eng.stream(R) for _ in range(B)]
    toks, taps = [[] for _ in range(B)], []
    ost = ob.OracleStream(oracle, R) if oracle else None
    sub_tap, lay_tap = ost.enable_taps() if ost else (None, None)
    ref, worst = [], dict(sub=0.0, layer=0.0)
    for k in range(pcms[0].size // piece):
        for b, t in enumerate(eng.step(sts, [p[k * piece:(k + 1) * piece] for p in pcms])):
            toks[b] += t
        if ost:
            ref += ost.process(pcms[0][k * piece:(k + 1) * piece])
            assert sts[0].stats().chunks == ost.total_chunks
        if not sts[0].stats().chunks:          # the first push completes no chunk
            continue
        taps.append([[st.tap(capi.TAP_SUBSAMPLED)[:T * 1024], st.tap(capi.TAP_ENCODER_OUT)[:T * 1024]]
                     + [st.tap(capi.TAP_LAYER_OUT, l)[:T * 1024] for l in range(N_LAYERS)] for st in sts])
        if ost:
            worst["sub"] = _acc(worst["sub"], taps[-1][0][0].reshape(T, 1024) - sub_tap)
            for l in range(N_LAYERS):
                worst["layer"] = _acc(worst["layer"], taps[-1][0][2 + l].reshape(T, 1024) - lay_tap[l])
    with pytest.raises(capi.NasrError, match="before the first"):
        eng.set_option("f32_split_planes", 0)
    for b, t in enumerate(eng.finalize(sts)):
        toks[b] += t
    frames = [st.token_frames() for st in sts]
    if ost:
        assert ost.total_chunks >= 4 and worst["sub"] < TOL_SUB and worst["layer"] < TOL_LAYER, worst
        assert toks[0] == ref + ost.finalize() and frames[0] == ost.token_frames()
    eng.close()
    return toks, frames, taps


def _same(a, b):
    assert a[0] == b[0] and a[1] == b[1]          # tokens, emission frames
    assert len(a[2]) == len(b[2])
    for sa, sb in zip(a[2], b[2]):
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for ta, tb in zip(sa, sb) for x, y in zip(ta, tb))


@pytest.mark.parametrize("B,R,pushes,oracle", [(64, 13, 3, False), (6, 0, 30, True), (6, 13, 5, True)], ids=["896rows", "6rows", "84rows"])
def test_planes_engine_equals_the_split_engine_bit_for_bit(weights, B, R, pushes, oracle):
    piece = synth.shift_samples(R)
    pcms = [synth.make_speech_pcm(b, pushes * piece / 16000.0 + 0.1)[0][:pushes * piece] for b in range(B)]
    om = ob.OracleModel(weights, N_LAYERS) if oracle else None
    _same(_stream_run(_engine(weights, B, 0), pcms, R), _stream_run(_engine(weights, B, 1), pcms, R, om))


def test_planes_engine_offline_call_equals_the_split_engine(weights):
    rng = np.random.default_rng(26)
    mels = [mel_for(T, rng) for T in (1, 65, 300)]
    got = []
    for planes in (0, 1):
        eng = _engine(weights, 3, planes)
        res = [eng.transcribe_mel(mels)]
        res += [eng.offline_tap(w, u, l) for u in range(3) for w, l in [(capi.TAP_SUBSAMPLED, 0), (capi.TAP_ENCODER_OUT, 0)] + [(capi.TAP_LAYER_OUT, l) for l in range(N_LAYERS)]]
        with pytest.raises(capi.NasrError, match="before the first"):
            eng.set_option("f32_split_planes", 1 - planes)
        eng.close()
        got.append(res)
    assert got[0][0] == got[1][0] and sum(len(t) for t in got[0][0][0]) > 0
    assert all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got[0][1:], got[1][1:]))


@pytest.mark.parametrize("dtype,split", [(capi.DTYPE_BF16, 1), (capi.DTYPE_F32, 0)], ids=["bf16", "f32_split=0"])
def test_option_takes_0_and_1_and_is_inert_without_the_split_f32_engine(weights, dtype, split):
    R, pushes, B = 13, 3, 6
    piece = synth.shift_samples(R)
    pcms = [synth.make_speech_pcm(b, pushes * piece / 16000.0 + 0.1)[0][:pushes * piece] for b in range(B)]
    eng = _engine(weights, B, 1, split, dtype)
    for v in (-1, 2):
        with pytest.raises(capi.NasrError, match="0 or 1"):
            eng.set_option("f32_split_planes", v)
    _same(_stream_run(_engine(weights, B, 0, split, dtype), pcms, R), _stream_run(eng, pcms, R))
