"""The eager completion of a graph step's decode (finish_step_decode, nasr_pipeline.hip) where nothing asserted on it: behind the grouped
pipeline's decode graph and behind the synchronous step graph.  (The pipelined one: tests/test_gpu_parity.py,
test_pipelined_decode_fallback_path.)"""
import numpy as np
import pytest

from nemotron_asr_amd import capi, synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu


def test_grouped_pipeline_decode_fallback_equals_synchronous_steps():
    """pipeline = 8 with "decode_graph_iterations" = 1: the decode graph carries two iterations, so every frame that emits two or more
    symbols is finished eagerly in gp_finish_decode.  Tokens, token frames and decoder state equal synchronous stepping.
    make_pcm seeds 70 and 71: the commit before the shared step driver fell back 2 times (2 rounds) on this input (its NASR_STATS line)."""
    L = 8
    W = synth.make_weights(n_layers=L)
    pcms = [synth.make_pcm(70 + b, 6.0) for b in range(2)]
    res = {}
    for mode in (0, 8):
        eng = capi.Engine(W, n_layers=L, dtype=capi.DTYPE_BF16, max_streams=2)
        eng.set_option("decode_graph_iterations", 1)
        eng.set_option("pipeline", mode)
        sts = [eng.stream(0), eng.stream(0)]
        toks = [[], []]
        for k in range(75):
            out = eng.step(sts, [p[k * 1280:(k + 1) * 1280] for p in pcms])
            toks[0] += out[0]; toks[1] += out[1]
        out = eng.finalize(sts)
        toks[0] += out[0]; toks[1] += out[1]
        res[mode] = (toks, [s.token_frames() for s in sts], np.stack([s.tap(capi.TAP_DEC_STATE) for s in sts]),
                     eng.counter("grouped_steps"), eng.counter("decode_fallbacks"), eng.counter("decode_fallback_rounds"))
        eng.close()
    assert res[8][3] > 40 and res[0][3] == 0
    assert res[8][4] > 0 and res[8][5] >= res[8][4], res[8][3:]
    assert res[8][0] == res[0][0] and sum(len(t) for t in res[0][0]) > 0
    assert res[8][1] == res[0][1]
    assert np.array_equal(res[8][2], res[0][2])


def test_synchronous_graph_step_decode_fallback_equals_oracle():
    """The synchronous step graph carries decode_blind_iterations(2) = 5 iterations at R = 1, as many as the pipelined engine of
    test_pipelined_decode_fallback_path (pipe_blind_iterations(2, 1)), which must fall back on these inputs: tokens equal the f32 oracle."""
    W = synth.make_weights(n_layers=2)
    B, R = 4, 1
    piece = synth.shift_samples(R)
    pcms = [synth.make_pcm(80 + b, 6.0) for b in range(B)]
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=B)
    eng.set_option("pipeline", 0)
    sts = [eng.stream(R) for _ in range(B)]
    toks = [[] for _ in range(B)]
    for k in range(pcms[0].size // piece):
        out = eng.step(sts, [p[k * piece:(k + 1) * piece] for p in pcms])
        for b in range(B):
            toks[b] += out[b]
    out = eng.finalize(sts)
    for b in range(B):
        toks[b] += out[b]
    fallbacks, replays = eng.counter("decode_fallbacks"), eng.counter("graph_replays")
    eng.close()
    om = ob.OracleModel(W, 2)
    for b in range(B):
        ost = ob.OracleStream(om, R)
        ref = []
        for k in range(pcms[b].size // piece):
            ref += ost.process(pcms[b][k * piece:(k + 1) * piece])
        ref += ost.finalize()
        assert toks[b] == ref, "oracle mismatch on stream %d" % b
    assert sum(len(t) for t in toks) > 20
    assert replays > 0 and fallbacks > 0, (replays, fallbacks)
