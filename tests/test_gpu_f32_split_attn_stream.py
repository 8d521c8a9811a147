"""Engine option "f32_split_attn_stream" through the C ABI: an F32 engine whose streaming attention launches run on k_attention_f32_split (three bf16
MFMA products of split operands), with and without "f32_split".  The model, the streams, the oracle comparison (`_run`: layer taps within the F32 oracle tolerances,
tokens and frames equal to the oracle's) and the alone / larger-batch orders are tests/test_gpu_f32_split.py's.  0 and 1 before the first step only; inert on bf16."""
import numpy as np
import pytest
from nemotron_asr_amd import capi, synth
from tests import test_gpu_f32_split as fs
from tests.test_gpu_f32_split import B, model          # noqa: F401 (the module's fixture)
from tests.test_gpu_parity import N_LAYERS

pytestmark = pytest.mark.gpu
OPT = "f32_split_attn_stream"


def _engine(W, n_streams, dtype=capi.DTYPE_F32, on=1, gemm_split=0):
    eng = capi.Engine(W, n_layers=N_LAYERS, dtype=dtype, max_streams=n_streams)
    for v in (-1, 2, 16):
        with pytest.raises(capi.NasrError, match="0 or 1"):
            eng.set_option(OPT, v)
    eng.set_option(OPT, on)
    eng.set_option("f32_split", gemm_split)
    eng.set_debug(True)
    return eng


@pytest.mark.parametrize("gemm_split", [0, 1])
@pytest.mark.parametrize("R", [0, 13])
def test_matches_the_oracle_and_batch_equals_alone(model, monkeypatch, R, gemm_split):
    monkeypatch.setattr(fs, "_engine", lambda W, n: _engine(W, n, gemm_split=gemm_split))
    piece, n_steps = synth.shift_samples(R), 5 if R else 30
    pcms = [synth.make_speech_pcm(b, n_steps * piece / 16000.0 + 0.1)[0][:n_steps * piece] for b in range(2 * B)]
    toks, frames, encs = fs._run(model, pcms, R, list(range(B)))
    for order in ([[0], [B - 1]] if R >= 4 else [list(range(2 * B))[::-1]]):          # that file's orders: no comparison crosses the four-row GEMM boundary
        t2, f2, e2 = fs._run(model, pcms, R, order)
        for b in set(order) & set(range(B)):
            assert t2[b] == toks[b] and f2[b] == frames[b], b
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(encs[b], e2[b])), b


def _steps(eng, R=13, n=4):
    piece = synth.shift_samples(R)
    pcm, st, toks, encs = synth.make_speech_pcm(0, n * piece / 16000.0 + 0.1)[0], eng.stream(R), [], []
    for k in range(n):
        toks += eng.step([st], [pcm[k * piece:(k + 1) * piece]])[0]
        encs.append(st.tap(capi.TAP_ENCODER_OUT).view(np.uint32))
    return toks + eng.finalize([st])[0], np.concatenate(encs)


def test_refused_after_the_first_step_and_inert_on_a_bf16_engine(model):
    eng = _engine(model[0], 1)
    _steps(eng, n=1)
    with pytest.raises(capi.NasrError, match="before the first"):
        eng.set_option(OPT, 0)
    eng.close()
    out = []
    for v in (0, 1):
        eng = _engine(model[0], 1, capi.DTYPE_BF16, on=v)
        out.append(_steps(eng))
        eng.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
