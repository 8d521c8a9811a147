"""Engine option "f32_split_attn" through the C ABI: an F32 engine whose offline attention runs on k_off_attn_f32_split (three bf16 MFMA products of split
operands for the content scores, the position scores and P.V).  Two layers of the speech checkpoint, one offline call of two utterances of about 6 s and
11 s (76 and 139 frames: more than one 64-query block and one 64-key block each), with option "f32_split" off and on: encoder output within the 2e-3 the
f32 offline tests assert, tokens and frames the offline oracle's, and the second utterance alone bit-identical to itself in the batch."""
import numpy as np
import pytest

from nemotron_asr_amd import capi, synth
from oracle import binding as ob
from tests import offline_ref as orf
from tests.test_gpu_parity import N_LAYERS, _acc

pytestmark = pytest.mark.gpu
TOL = 2e-3


@pytest.fixture(scope="module")
def model():
    W = synth.make_weights(N_LAYERS, margins="speech")
    om = ob.OracleModel(W, N_LAYERS)
    pcms = [synth.make_speech_pcm(u, s)[0] for u, s in ((0, 6.0), (1, 11.0))]
    mels = [ob.OraclePreproc(W["preprocessor.featurizer.fb"], W["preprocessor.featurizer.window"]).process(p) for p in pcms]          # a preprocessor per utterance: it keeps state
    encs = [orf.encode(om, W, m, N_LAYERS)[2] for m in mels]
    return W, pcms, encs, [orf.greedy(om, e) for e in encs]


def _call(W, pcms, dtype, attn, gemm=0):
    eng = capi.Engine(W, n_layers=N_LAYERS, dtype=dtype, max_streams=len(pcms))
    eng.set_option("f32_split", gemm)
    eng.set_option("f32_split_attn", attn)
    eng.set_debug(True)
    toks, frames = eng.transcribe(pcms)
    encs = [eng.offline_tap(capi.TAP_ENCODER_OUT, u).copy() for u in range(len(pcms))]
    with pytest.raises(capi.NasrError, match="before the first"):
        eng.set_option("f32_split_attn", 0)
    eng.close()
    return toks, frames, encs


@pytest.mark.parametrize("gemm", [0, 1])
def test_offline_call_matches_the_oracle_and_batch_equals_alone(model, gemm):
    W, pcms, ref_enc, ref_greedy = model
    toks, frames, encs = _call(W, pcms, capi.DTYPE_F32, 1, gemm)
    for u in range(2):
        assert ref_enc[u].shape[0] > 64
        worst = _acc(0.0, encs[u] - ref_enc[u])
        print(f"f32_split {gemm}, utterance {u} ({ref_enc[u].shape[0]} frames): max |enc - oracle| = {worst:.3e}")
        assert worst < TOL
        assert (toks[u], frames[u]) == ref_greedy[u]
    t1, f1, e1 = _call(W, pcms[1:], capi.DTYPE_F32, 1, gemm)
    assert (t1[0], f1[0]) == (toks[1], frames[1])
    assert np.array_equal(e1[0].view(np.uint32), encs[1].view(np.uint32))


def test_option_values_and_bf16_engine(model):
    W, pcms = model[0], [model[1][0][:32000]]
    eng = capi.Engine(W, n_layers=N_LAYERS, dtype=capi.DTYPE_F32, max_streams=1)
    for v in (-1, 2, 16):
        with pytest.raises(capi.NasrError, match="0 or 1"):
            eng.set_option("f32_split_attn", v)
    eng.close()
    a, b = _call(W, pcms, capi.DTYPE_BF16, 0), _call(W, pcms, capi.DTYPE_BF16, 1)
    assert a[:2] == b[:2] and np.array_equal(a[2][0].view(np.uint32), b[2][0].view(np.uint32))
