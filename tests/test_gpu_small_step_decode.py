"""The one-frame step of the fused family (bf16, up to four rows): its decode graph carries 3 iterations by default
(nasr_step::pipe_decode_iterations) and its lane cut is its own (nasr_step::fused_cut), so steps of the two families never share the
lanes (pipe_step: cut identity, counter "cut_drains").  What that must not change: a burst beyond the short graph is finished by
finish_step_decode's fallback, a stream whose steps alternate between the families while steps are in flight keeps its caches, and quiet
audio never pays the fallback."""
from collections import Counter

import numpy as np
import pytest

from nemotron_asr_amd import capi, synth

pytestmark = pytest.mark.gpu

L = 4
N = synth.shift_samples(0)          # 1280 samples: one frame per push at R = 0


@pytest.fixture(scope="module")
def W4():
    return synth.make_weights(n_layers=L)


def _one_stream(W, n_layers, pcm, n_push, pipeline):
    eng = capi.Engine(W, n_layers=n_layers, dtype=capi.DTYPE_BF16, max_streams=1)
    eng.set_option("pipeline", pipeline)
    st = eng.stream(0)
    toks = []
    for k in range(n_push):
        toks += eng.step([st], [pcm[k * N:(k + 1) * N]])[0]
    toks += eng.finalize([st])[0]
    res = dict(tokens=toks, frames=st.token_frames(), dec=st.tap(capi.TAP_DEC_STATE).copy(), fallbacks=eng.counter("decode_fallbacks"),
               pipelined=eng.counter("pipelined_steps"), grouped=eng.counter("grouped_steps"), cut_drains=eng.counter("cut_drains"))
    eng.close()
    return res


@pytest.fixture(scope="module")
def burst_sync(W4):
    pcm = synth.make_pcm(31, 100 * N / 16000 + 0.01)[:100 * N]
    return pcm, _one_stream(W4, L, pcm, 100, 0)


@pytest.mark.parametrize("pipeline", [4, 8])
def test_a_burst_beyond_the_short_decode_graph_is_finished_eagerly(W4, burst_sync, pipeline):
    """Near-tie checkpoint, make_pcm(31), 100 one-frame pushes: frames that emit three or more symbols need four or more iterations, one more
    than the default graph carries, so the fallback must run -- and tokens, token frames and decoder state equal synchronous stepping.  (The
    f32 oracle on these inputs: 6 of the 11 emitting frames emit 3, 3, 3, 4, 4, 4 symbols.)  The burst is asserted on the synchronous engine's
    own token frames, so a quiet input fails here instead of passing without the fallback.  The grouped launches of "pipeline" = 8 need a layer count that is a multiple
    of 8 (tests/test_gpu_step_driver.py covers their fallback on 8 layers): on this 4-layer model the option runs the four lanes."""
    pcm, sync = burst_sync
    per_frame = Counter(sync["frames"])
    assert per_frame and max(per_frame.values()) >= 3, sorted(per_frame.values())
    got = _one_stream(W4, L, pcm, 100, pipeline)
    assert got["pipelined"] + got["grouped"] > 0
    if pipeline == 4:
        assert got["pipelined"] > 0
    assert got["fallbacks"] > 0, got
    assert got["tokens"] == sync["tokens"] and len(sync["tokens"]) > 0
    assert got["frames"] == sync["frames"]
    assert np.array_equal(got["dec"], sync["dec"])


def _mixed_run(W, pipeline, n_calls, mixed):
    """stream 0 alone (a fused step of one row); with `mixed`, every third call together with five others (an unfused step of six rows)"""
    B = 6
    eng = capi.Engine(W, n_layers=L, dtype=capi.DTYPE_BF16, max_streams=B)
    eng.set_option("pipeline", pipeline)
    sts = [eng.stream(0) for _ in range(B)]
    pcms = [synth.make_pcm(40 + b, n_calls * N / 16000 + 0.01)[:n_calls * N] for b in range(B)]
    pos, toks = [0] * B, [[] for _ in range(B)]
    for c in range(n_calls):
        idx = list(range(B)) if mixed and c % 3 == 0 else [0]
        out = eng.step([sts[b] for b in idx], [pcms[b][pos[b] * N:(pos[b] + 1) * N] for b in idx])
        for b, t in zip(idx, out):
            toks[b] += t
            pos[b] += 1
    for b, t in enumerate(eng.finalize(sts)):
        toks[b] += t
    caches = [sts[0].tap(tap, l, cap=70 * 1024).copy() for l in range(L) for tap in (capi.TAP_K_CACHE, capi.TAP_V_CACHE, capi.TAP_CONV_CACHE)]
    res = dict(tokens=toks, frames=[s.token_frames() for s in sts], caches=caches, cut_drains=eng.counter("cut_drains"),
               pipelined=eng.counter("pipelined_steps"))
    eng.close()
    return res


def test_family_change_while_steps_are_in_flight(W4):
    """80 calls: a mixed call of six rows (unfused layers, cut at whole layers), then two calls of stream 0 alone (fused layers, cut at
    launches), so steps of both forms are in flight at every switch.  pipe_step completes the steps in flight before a step of the other
    family; tokens and token frames of every stream and every layer's K / V ring and conv cache of stream 0 equal synchronous stepping bit
    for bit.  A population that stays in one family never drains."""
    sync, pipe = _mixed_run(W4, 0, 80, True), _mixed_run(W4, 4, 80, True)
    assert pipe["pipelined"] > 0 and pipe["cut_drains"] > 0, pipe["cut_drains"]
    assert sync["cut_drains"] == 0
    assert pipe["tokens"] == sync["tokens"] and sum(len(t) for t in sync["tokens"]) > 0
    assert pipe["frames"] == sync["frames"]
    assert len(pipe["caches"]) == 3 * L
    for a, b in zip(pipe["caches"], sync["caches"]):
        assert a.size > 0 and np.array_equal(a, b)
    fused_only = _mixed_run(W4, 4, 40, False)
    assert fused_only["pipelined"] > 0 and fused_only["cut_drains"] == 0


def test_default_budget_never_falls_back_on_quiet_audio():
    """The speech checkpoint (its joint is fitted to the 24-layer encoder) on make_speech_pcm(0): no frame emits more than two symbols, so 60
    pipelined steps with the default 3-iteration decode graph never take the fallback, and the tokens equal synchronous stepping."""
    W = synth.make_weights(n_layers=24, margins="speech")
    pcm = synth.make_speech_pcm(0, 60 * N / 16000 + 0.01)[0][:60 * N]
    sync, pipe = _one_stream(W, 24, pcm, 60, 0), _one_stream(W, 24, pcm, 60, 4)
    assert pipe["pipelined"] > 0 and pipe["fallbacks"] == 0 and pipe["cut_drains"] == 0
    assert pipe["tokens"] == sync["tokens"] and pipe["frames"] == sync["frames"]
    assert len(sync["tokens"]) > 0
