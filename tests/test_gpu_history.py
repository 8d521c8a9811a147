"""Frame history of live streams (engine option "frame_history") and the second-pass entries over it, through the C ABI on the MI355X.

Engines: the 2-layer synthetic model of the other GPU tests (the sharpened joint of tests/test_gpu_beam.py, GAIN = 30, where log-probabilities
are compared), and the 24-layer "speech" checkpoint for the greedy second pass.

Bound of a kept row.  A row is joint.enc applied to the encoder's f32 output row x: 640 f32 dot products of length 1024 plus the bias, in both
engines (the bf16 engine keeps the residual stream and this projection in f32: k_encproj reads f32 x and f32 weights, so the same bound holds
there and the test runs both dtypes).  Whatever the summation order, an f32 dot product of length n plus one addition satisfies
|err| <= (n + 1) * 2^-24 * (sum_k |x_k w_k| + |b|) to first order -- the standard forward bound, derived and not measured; n = 1024.
The reference is the float64 product of the engine's own tapped encoder rows (NASR_TAP_ENCODER_OUT) with the checkpoint's joint.enc.

Log-probabilities of two decode kernel forms over the same rows (the live decode's few-row joint, the offline decode's tiled joint) are
compared with LP_BOUND = 2e-4, the tolerance tests/test_gpu_logprobs.py uses between a stream alone (k_dec_joint) and in a batch of 64
(k_dec_joint_tiled): the line `assert d < LP_BOUND` that closes test_option_changes_nothing_but_adds_the_values_and_is_deterministic
(tests/test_gpu_logprobs.py:322).  loglik / best against the
float64 recursions use (T + U + 1) * LP_BOUND, the tolerance of tests/test_gpu_align.py.

Greedy second pass: tokens and frames must EQUAL the stream's own.  Rule for a near-tie: both decodes take the arg-max of the same joint
over the same rows from the same start state, through kernels that sum in different orders, so they can only part where the top-2 margin of
a decision is below the kernels' difference (2 * LP_BOUND in log-probability); the speech checkpoint's decisions have margins of 0.5 logits
and more on >= 99 % of frames (tests/test_gpu_speech.py).  Should a run ever differ, the comparison is to be made up to the first decision
whose float64 margin (tests/align_ref.py lattice of the tapped rows) is below 2 * LP_BOUND, as tests/test_gpu_beam.py does for its reference
search; until that happens the test demands equality outright.

Every figure is printed before it is asserted (run with -s)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi, gguf_io, synth
from oracle import binding as ob
from tests import align_ref as ar
from tests import beam_lm_ref as blr
from tests.test_gpu_beam import CachedOracle, check_invariants, sharpened

pytestmark = pytest.mark.gpu

GAIN = 30.0
LP_BOUND = 2e-4
ROW = 640
DTYPES = [capi.DTYPE_F32, capi.DTYPE_BF16]
IDS = ["f32", "bf16"]


@pytest.fixture(scope="module")
def W2():
    return synth.make_weights(n_layers=2)


@pytest.fixture(scope="module")
def WS(W2):
    return sharpened(W2, GAIN)


def engine(W, dtype, max_streams=1, N=2048, options=(), L=2, debug=False):
    eng = capi.Engine(W, n_layers=L, dtype=dtype, max_streams=max_streams)
    if N:
        eng.set_option("frame_history", N)
    for k, v in options:
        eng.set_option(k, v)
    if debug:
        eng.set_debug(True)
    return eng


def done_of(st):
    first, count = st.history_range()
    return first + count


def feed(eng, sts, pcms, n, enc=None, finalize=True):
    """steps the streams through their audio n samples per call (n: one number, or one per stream for ragged pushes), then the finalize tail;
    enc (a list per stream): the tapped encoder rows of the frames each call decodes are appended.  -> the token lists"""
    ns = [n] * len(sts) if np.isscalar(n) else list(n)
    toks = [[] for _ in sts]
    at = [0] * len(sts)
    while any(at[b] < pcms[b].size for b in range(len(sts))):
        before = [done_of(s) for s in sts] if enc is not None else None
        for b, t in enumerate(eng.step(sts, [pcms[b][at[b]:at[b] + ns[b]] for b in range(len(sts))])):
            toks[b] += t
        at = [a + k for a, k in zip(at, ns)]
        if enc is not None:
            for b, s in enumerate(sts):
                k = done_of(s) - before[b]
                if k > 0:
                    enc[b].append(s.tap(capi.TAP_ENCODER_OUT).reshape(-1, 1024)[:k])
    if finalize:
        before = [done_of(s) for s in sts] if enc is not None else None
        for b, t in enumerate(eng.finalize(sts)):
            toks[b] += t
        if enc is not None:
            for b, s in enumerate(sts):
                k = done_of(s) - before[b]
                if k > 0:
                    enc[b].append(s.tap(capi.TAP_ENCODER_OUT).reshape(-1, 1024)[:k])
    return toks


def row_bound(W, x):
    """(float64 product, the forward bound of its f32 evaluation) of encoder rows x [n][1024] with joint.enc"""
    x64 = np.asarray(x, np.float64)
    w, b = np.asarray(W["joint.enc.weight"], np.float64), np.asarray(W["joint.enc.bias"], np.float64)
    return x64 @ w.T + b, 1025 * 2.0 ** -24 * (np.abs(x64) @ np.abs(w).T + np.abs(b))


def check_rows(name, W, hist, enc):
    x = np.concatenate(enc) if enc else np.zeros((0, 1024), np.float32)
    assert hist.shape == (x.shape[0], ROW), (name, hist.shape, x.shape)
    ref, bound = row_bound(W, x)
    worst = float((np.abs(hist.astype(np.float64) - ref) / bound).max()) if x.size else 0.0
    print(f"history rows {name}: {x.shape[0]} frames, worst |err| / bound = {worst:.3f}")
    assert worst <= 1.0, (name, worst)


# ---- rows are right -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R", [0, 13])
def test_rows_are_the_projection_of_the_tapped_encoder_rows(W2, dtype, R):
    n = synth.shift_samples(R)
    seconds = 40 * 0.08 + 0.35                                    # about 40 frames and a tail for finalize
    for B in (1, 3):                                              # alone, and with two more streams of other audio in the same calls: the slots do not mix
        eng = engine(W2, dtype, max_streams=B, debug=True)
        sts = [eng.stream(R) for _ in range(B)]
        pcms = [synth.make_pcm(910 + 7 * b, seconds) for b in range(B)]
        enc = [[] for _ in range(B)]
        feed(eng, sts, pcms, n, enc)
        for b, s in enumerate(sts):
            first, count = s.history_range()
            assert first == 0 and count == sum(e.shape[0] for e in enc[b]) and count >= 38
            check_rows(f"R{R}-B{B}-stream{b}", W2, s.history(0, count), enc[b])
        if B == 3:
            assert not np.array_equal(sts[0].history(0, 8), sts[1].history(0, 8))
        eng.close()


# ---- every step form writes the same bits ---------------------------------------------------------------------------------------------------
def run_form(W, dtype, R, pcms, n, options=(), N=2048, finalize=True, L=2):
    eng = engine(W, dtype, max_streams=len(pcms), N=N, options=options, L=L)
    sts = [eng.stream(R) for _ in pcms]
    toks = feed(eng, sts, pcms, n, finalize=finalize)
    out = dict(tokens=toks, frames=[s.token_frames() for s in sts], range=[s.history_range() for s in sts],
               rows=[s.history(*s.history_range()) for s in sts], state=[s.tap(capi.TAP_DEC_STATE) for s in sts],
               last_enc=[s.tap(capi.TAP_ENCODER_OUT) for s in sts],
               counters={k: eng.counter(k) for k in ("graph_replays", "eager_steps", "pipelined_steps", "grouped_steps")})
    eng.close()
    return out


def same_history(a, b):
    return a["tokens"] == b["tokens"] and a["frames"] == b["frames"] and a["range"] == b["range"] and \
        all(x.tobytes() == y.tobytes() for x, y in zip(a["rows"], b["rows"])) and all(x.tobytes() == y.tobytes() for x, y in zip(a["state"], b["state"]))


@pytest.mark.parametrize("R", [0, 13])
def test_every_step_form_writes_the_same_bits(W2, R):
    n = synth.shift_samples(R)
    pcms = [synth.make_pcm(930, (24 if R == 0 else 42) * 0.08 + 0.35)]
    # Within each "fused" setting: eager against the synchronous graph and the pipelined steps.  Across the two settings the history is held
    # to the encoder's own output: "fused" picks the encoder's kernel family at few rows per step, and the test reads the encoder rows of
    # the last step (NASR_TAP_ENCODER_OUT, the input of the projection, which this feature does not touch) under both.  Where those rows
    # are bit-equal the histories must be bit-equal; where the encoder itself gives other bits (measured: R = 0, one row per step) the
    # kept rows cannot be equal and the comparison is of the ranges and row counts
    forms = {"graph": (("graph", 1),), "pipeline1": (("pipeline", 1),), "pipeline4": (("pipeline", 4),), "pipeline8": (("pipeline", 8),)}
    bases = {}
    for fused in (1, 0):
        base = bases[fused] = run_form(W2, capi.DTYPE_BF16, R, pcms, n, (("fused", fused), ("graph", 0)))
        assert base["range"][0][0] == 0 and base["range"][0][1] >= (22 if R == 0 else 40) and base["counters"]["eager_steps"] > 0
        for name, opts in forms.items():
            got = run_form(W2, capi.DTYPE_BF16, R, pcms, n, (("fused", fused),) + opts)
            print(f"history forms R{R} fused {fused} {name}: {got['counters']}")
            assert same_history(base, got), (fused, name)
            if name == "graph":
                assert got["counters"]["graph_replays"] > 0
            if name.startswith("pipeline"):
                assert got["counters"]["pipelined_steps"] > 0
    enc_equal = bases[0]["last_enc"][0].tobytes() == bases[1]["last_enc"][0].tobytes()
    d_enc = float(np.abs(bases[0]["last_enc"][0] - bases[1]["last_enc"][0]).max())
    print(f"history forms R{R}: encoder rows of the last step under fused 0 / 1 bit-equal: {enc_equal} (max |d| {d_enc:.3e})")
    assert bases[0]["range"] == bases[1]["range"] and bases[0]["rows"][0].shape == bases[1]["rows"][0].shape
    if enc_equal:
        assert same_history(bases[0], bases[1])
    if R == 13:                                                   # 14 rows per step: both settings run the same kernels
        assert enc_equal
    # the append's other grid (measurement option): the same bytes
    one = run_form(W2, capi.DTYPE_BF16, R, pcms, n, (("history_append_rows", 4),))
    graph = run_form(W2, capi.DTYPE_BF16, R, pcms, n)
    assert same_history(one, graph) and same_history(graph, bases[1])


def test_grouped_form_writes_the_same_bits():
    """"pipeline" = 8 takes the grouped form at one row per step on a model whose layer count is a multiple of 8: an 8-layer engine"""
    W8 = synth.make_weights(n_layers=8)
    n = synth.shift_samples(0)
    pcms = [synth.make_pcm(935, 24 * 0.08 + 0.35)]
    base = run_form(W8, capi.DTYPE_BF16, 0, pcms, n, (("graph", 0),), L=8)
    got = run_form(W8, capi.DTYPE_BF16, 0, pcms, n, (("pipeline", 8),), L=8)
    print(f"history forms grouped: {got['counters']}")
    assert got["counters"]["grouped_steps"] > 0 and base["range"][0][1] >= 22
    assert same_history(base, got)


@pytest.mark.parametrize("options", [(("graph", 1),), (("pipeline", 4),)], ids=["graph", "pipeline4"])
def test_multi_chunk_pushes_keep_the_same_frames(W2, options):
    """several chunks per call (G chunks x T frames in one launch sequence; the eager path has no such form, it runs chunk by chunk): done, the range, the tokens and the row count are those of chunk by
    chunk; the rows are within the bound of the float64 product of the rows THAT call's encoder produced (another row count: other GEMM shapes)"""
    R, per_call = 1, 5
    n = synth.shift_samples(R)
    pcm = synth.make_pcm(940, 20 * n / 16000 + 0.2)
    base = run_form(W2, capi.DTYPE_F32, R, [pcm], n, (("graph", 0),))
    eng = engine(W2, capi.DTYPE_F32, options=options)
    st = eng.stream(R)
    enc = [[]]
    toks = feed(eng, [st], [pcm], per_call * n, enc)          # without debug mode the tap reads the step's workspace rows
    assert toks == base["tokens"] and st.token_frames() == base["frames"][0] and st.history_range() == base["range"][0]
    assert max(e.shape[0] for e in enc[0]) == per_call * (1 + R)
    hist = st.history(*st.history_range())
    assert hist.shape == base["rows"][0].shape
    check_rows(f"multi-chunk {options}", W2, hist, enc[0])
    eng.close()


def test_ragged_batch_only_the_stream_that_completes_a_chunk_appends(W2):
    R = 0
    n = synth.shift_samples(R)
    pcms = [synth.make_pcm(950, 16 * n / 16000), synth.make_pcm(951, 16 * n / 16000)]
    for opts in ((("graph", 0),), (("graph", 1),), (("pipeline", 4),)):
        eng = engine(W2, capi.DTYPE_BF16, max_streams=2, options=opts)
        sts = [eng.stream(R) for _ in range(2)]
        done = [[], []]
        for k in range(10):                                       # stream 1 gets half a chunk per call: it completes one every other call
            eng.step(sts, [pcms[0][k * n:(k + 1) * n], pcms[1][k * n // 2:(k + 1) * n // 2]])
            for b in range(2):
                done[b].append(done_of(sts[b]))
        assert all(b - a in (0, 1) for a, b in zip(done[1], done[1][1:])) and done[1][-1] < done[0][-1] and 0 in np.diff(done[1])
        rows = [s.history(*s.history_range()) for s in sts]
        if opts == (("graph", 0),):
            base = rows
        assert all(a.tobytes() == b.tobytes() for a, b in zip(base, rows)), opts
        eng.close()


# ---- wrap, reset, recycled slots, the option's values -----------------------------------------------------------------------------------------
def test_wrap_reset_and_recycled_slot(W2):
    R = 13
    n = synth.shift_samples(R)
    pcm = synth.make_pcm(960, 10 * n / 16000 + 0.6)              # ten chunks of 14 frames and a tail: about 150 frames
    small, big = engine(W2, capi.DTYPE_BF16, N=64), engine(W2, capi.DTYPE_BF16, N=2048)
    s, b = small.stream(R), big.stream(R)
    assert feed(small, [s], [pcm], n) == feed(big, [b], [pcm], n)
    done = done_of(b)
    assert 140 <= done <= 160 and b.history_range() == (0, done) and s.history_range() == (done - 64, 64)
    assert s.history(done - 64, 64).tobytes() == b.history(done - 64, 64).tobytes()          # crosses the wrap unless done is a multiple of 64
    assert s.history(done - 10, 10).tobytes() == b.history(done - 10, 10).tobytes()
    assert s.history(done - 65, 64).shape == (0, ROW) and s.history(done - 64, 65).shape == (0, ROW)
    with pytest.raises(capi.NasrError, match=rf"window \[{done - 65}, {done - 1}\) of streams\[0\] is not wholly kept: the stream keeps frames \[{done - 64}, {done}\)"):
        small.history_transcribe([s], [(done - 65, 64)])
    with pytest.raises(capi.NasrError, match="NO_SYNC"):
        small.history_transcribe([s], [(done - 64, 64)], flags=capi.FLAG_NO_SYNC)
    assert small.history_transcribe([s], [(done - 64, 64)]) == big.history_transcribe([b], [(done - 64, 64)])
    assert small.history_transcribe([s], [(done - 3, 0)]) == ([[]], [[]])          # count = 0: what T = 0 gives offline
    assert small.counter("history_calls") == 2 and small.counter("history_frames") == 64
    for reference in (False, True):
        s.reset(reference=reference)
        assert s.history_range() == (0, 0) and s.history(0, 1).shape == (0, ROW)
        feed(small, [s], [pcm[:3 * n]], n, finalize=False)
        chunks = s.progress().chunks
        assert chunks >= 2 and s.history_range() == (0, 14 * chunks)
    s.destroy()
    fresh = small.stream(R)                                      # the recycled slot: nothing of its predecessor
    assert fresh.history_range() == (0, 0) and fresh.history(0, 1).shape == (0, ROW)
    with pytest.raises(capi.NasrError, match="not wholly kept"):
        small.history_transcribe([fresh], [(0, 1)])
    small.close()
    big.close()


def test_option_values_and_entries_without_the_option(W2):
    eng = capi.Engine(W2, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    for bad in (-64, 1, 63, 65, 100, 2047, 2112, 4096):
        with pytest.raises(capi.NasrError, match="frame_history must be 0 or"):
            eng.set_option("frame_history", bad)
    eng.set_option("frame_history", 0)
    st = eng.stream(0)
    n = synth.shift_samples(0)
    pcm = synth.make_pcm(970, 4 * n / 16000)
    for call in (st.history_range, lambda: st.history(0, 1), lambda: eng.history_transcribe([st], [(0, 1)]), lambda: eng.history_beam([st], [(0, 1)]),
                 lambda: eng.history_align([st], [(0, 1)], [[5]])):
        with pytest.raises(capi.NasrError, match='engine option "frame_history" is off'):
            call()
    assert len(eng.step([st], [pcm])) == 1                       # the engine is usable
    with pytest.raises(capi.NasrError, match="before the first step"):
        eng.set_option("frame_history", 64)
    eng.close()
    eng = capi.Engine(W2, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    for ok in (64, 0, 128, 2048, 0, 64):                          # until the first step another N replaces the rings and 0 frees them
        eng.set_option("frame_history", ok)
    st = eng.stream(0)
    eng.step([st], [synth.make_pcm(971, 4 * n / 16000)])
    assert st.history_range() == (0, done_of(st)) and 2 <= done_of(st) <= 4 and st.history(0, 2).shape == (2, ROW)
    with pytest.raises(capi.NasrError, match="null"):
        capi._chk(capi.lib().nasr_engine_history_transcribe(eng.h, None, 1, None, None, None, None, (C.c_int32 * 1)(), None, 0))
    with pytest.raises(capi.NasrError, match="null"):
        capi._chk(capi.lib().nasr_stream_get_history(st.h, 0, 1, None))
    eng.close()


# ---- option off is what it was ------------------------------------------------------------------------------------------------------------------
def test_option_off_launches_nothing_and_on_changes_no_bit(W2):
    R = 0
    n = synth.shift_samples(R)
    pcm = synth.make_pcm(980, 12 * n / 16000 + 0.3)
    results = {}
    for N in (0, 2048):
        eng = engine(W2, capi.DTYPE_BF16, N=N)
        st = eng.stream(R)
        toks = feed(eng, [st], [pcm], n)
        results[N] = (toks, st.token_frames(), st.tap(capi.TAP_DEC_STATE).tobytes(), st.progress().chunks)
        eng.close()
        eng = engine(W2, capi.DTYPE_BF16, N=N)                    # the same under the profiler (eager steps): launches by name
        eng.profile(True)
        st = eng.stream(R)
        assert feed(eng, [st], [pcm], n) == toks
        stats = {s["name"]: s["launches"] for s in eng.profile_read()}
        steps = st.progress().chunks
        print(f"frame_history = {N}: {steps} decoded steps, k_history_append launches {stats.get('k_history_append', 0)}")
        assert stats.get("k_history_append", 0) == (steps if N else 0) and steps >= 12
        eng.close()
    assert results[0] == results[2048]


# ---- fork and restore ------------------------------------------------------------------------------------------------------------------------
def test_fork_and_restore_start_with_an_empty_history(W2):
    R = 1
    n = synth.shift_samples(R)
    pcm = synth.make_pcm(990, 30 * n / 16000)
    eng = engine(W2, capi.DTYPE_BF16, max_streams=3, N=64)
    plain = engine(W2, capi.DTYPE_BF16, max_streams=1, N=0)
    src, twin = eng.stream(R), plain.stream(R)
    feed(eng, [src], [pcm[:14 * n]], n, finalize=False)
    feed(plain, [twin], [pcm[:14 * n]], n, finalize=False)
    done = done_of(src)
    assert 24 <= done <= 28
    before = src.history(0, done)
    fork, blob = src.fork(), src.save()
    # the blob has the size and the header it has on an engine without the option: everything the header states up to the checksums (bytes
    # 120 .. 127 and 136 .. 143 sum the device section and the head; the sections hold whole rings, whose never-written entries differ
    # between any two engines) and the reserved bytes
    other = twin.save()
    assert len(blob) == len(other) and blob[:120] == other[:120] and blob[128:136] == other[128:136] == bytes(8)
    back = eng.restore(blob)
    assert fork.history_range() == (done, 0) and back.history_range() == (done, 0) and fork.history(done - 1, 1).shape == (0, ROW)
    assert src.history_range() == (0, done) and src.history(0, done).tobytes() == before.tobytes()
    rest = pcm[14 * n:24 * n]
    toks = [feed(eng, [s], [rest], n, finalize=False) for s in (src, fork, back)]          # each in calls of its own
    assert toks[0] == toks[1] == toks[2]
    done2 = done_of(src)
    k = done2 - done
    assert 18 <= k <= 22 and fork.history_range() == (done, k) == back.history_range() and src.history_range() == (0, done2)
    later = src.history(done, k)
    assert later.shape == (k, ROW) and fork.history(done, k).tobytes() == later.tobytes() == back.history(done, k).tobytes()
    assert src.history(0, done).tobytes() == before.tobytes()
    with pytest.raises(capi.NasrError, match=rf"keeps frames \[{done}, {done2}\)"):
        eng.history_transcribe([fork], [(done - 1, 5)])
    assert eng.history_transcribe([fork], [(done, k)]) == eng.history_transcribe([src], [(done, k)])
    eng.close()
    plain.close()


# ---- the second passes ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=DTYPES, ids=IDS)
def world(request, WS):
    """one debug engine per dtype with three streams of other audio stepped chunk by chunk (R = 0, about 14 frames and the tail), their tapped
    encoder rows, and stream 0's twin that never sees a history call"""
    R = 0
    n = synth.shift_samples(R)
    eng = engine(WS, request.param, max_streams=4, debug=True, options=(("token_logprobs", 1), ("phrase_boost", 64)))
    sts = [eng.stream(R) for _ in range(3)]
    pcms = [synth.make_pcm(1000 + 3 * b, 13 * n / 16000 + 0.3) for b in range(3)]
    enc = [[] for _ in range(3)]
    toks = feed(eng, sts, pcms, n, enc)
    enc = [np.concatenate(e) for e in enc]
    yield dict(eng=eng, sts=sts, enc=enc, toks=toks, om=CachedOracle(ob.OracleModel(WS, 2)), W=WS, pcms=pcms, n=n)
    eng.close()


def own_lattices(eng, st, win, hyps):
    res = eng.history_align([st] * len(hyps), [win] * len(hyps), [h[1] for h in hyps])
    return [res[u] + eng.align_lattice(u, len(hyps[u][1])) for u in range(len(hyps))]


def hyp_bits(hyps):
    return [(h[0], h[1], h[2], h[3].tobytes()) for h in hyps]


def test_beam_second_pass_invariants_and_batches(world):
    eng, sts, enc, om = world["eng"], world["sts"], world["enc"], world["om"]
    done = [done_of(s) for s in sts]
    assert all(d == e.shape[0] and d >= 13 for d, e in zip(done, enc))
    for Wd, S in ((4, 3), (2, 3)):
        for first in (0, 5):                                      # a window from the stream's start, and one starting at a later frame
            win = (first, done[0] - first)
            hyps = eng.history_beam([sts[0]], [win], beam=Wd, max_symbols=S)[0]
            own = own_lattices(eng, sts[0], win, hyps)
            ref = [ar.lattice(om, enc[0][first:], h[1]) for h in hyps]          # the float64 lattice of THAT window's rows, fresh decoder state
            check_invariants(f"history W{Wd}-S{S}-first{first}", win[1], Wd, S, hyps, lambda r: own[r], lambda r: ref[r])
            wins = [win, (2, done[1] - 2), (0, done[2])]
            batch = eng.history_beam(sts, wins, beam=Wd, max_symbols=S)
            assert hyp_bits(batch[0]) == hyp_bits(hyps)                         # alone == in a batch of three streams' windows
            twice = eng.history_beam([sts[0], sts[1], sts[0]], [win, wins[1], win], beam=Wd, max_symbols=S)
            assert hyp_bits(twice[0]) == hyp_bits(twice[2]) == hyp_bits(hyps) and hyp_bits(twice[1]) == hyp_bits(batch[1])
    assert eng.offline_tap(capi.TAP_ENCODER_OUT, 0).size == 0          # no encoder ran: its taps are empty


def test_beam_second_pass_with_lm_and_boost(world):
    eng, st = world["eng"], world["sts"][0]
    win = (0, done_of(st))
    plain = eng.history_beam([st], [win], beam=4, max_symbols=3)[0]
    top = plain[0][1]
    assert len(top) >= 2
    weight, bonus = 0.5, 0.25
    eng.set_lm({(top[0],): -1.0, (top[1],): -2.0, (top[0], top[1]): -0.5}, order=2, weight=weight, token_bonus=bonus)
    for score, toks, frames, lps, lm, total, tok_lm in eng.history_beam([st], [win], beam=4, max_symbols=3, lm=True)[0]:
        assert total == blr.total_of(score, lm, len(toks), weight, bonus) and tok_lm.shape == (len(toks),)
    eng.set_lm(None)
    eng.set_boost_phrases([top[:2]], 2.0)
    boosted = eng.history_beam([st], [win], beam=4, max_symbols=3, boost=True)[0]
    totals = [h[5] for h in boosted]
    assert all(a >= b for a, b in zip(totals, totals[1:]))
    for score, toks, frames, lps, boost, total, bonuses in boosted:
        assert total == score + boost and boost == float(np.sum(bonuses.astype(np.float64))) and bonuses.shape == (len(toks),)
    assert any(h[4] > 0 for h in boosted)
    eng.set_boost_phrases(())
    assert hyp_bits(eng.history_beam([st], [win], beam=4, max_symbols=3)[0]) == hyp_bits(plain)


def test_align_second_pass_of_the_greedy_transcript(world):
    eng, sts, enc, om = world["eng"], world["sts"], world["enc"], world["om"]
    for b in (0, 1):
        st, toks = sts[b], world["toks"][b]
        T, U = done_of(st), len(toks)
        frames_g = st.token_frames()
        assert U >= 2 and len(frames_g) == U
        loglik, best, frames, lps = eng.history_align([st], [(0, T)], [toks])[0]
        lb, ly = eng.align_lattice(0, U)
        greedy_path = ar.path_score(lb.astype(np.float64), ly.astype(np.float64), frames_g)
        bound = (T + U + 1) * LP_BOUND
        rb, ry = ar.lattice(om, enc[b], toks)
        ref = ar.recursions(rb, ry)
        print(f"history align stream {b}: T {T} U {U} loglik {loglik:.4f} (float64 {ref['loglik']:.4f}) best {best:.4f} (float64 {ref['best']:.4f}) greedy path {greedy_path:.4f}")
        assert loglik >= best >= greedy_path - 1e-9
        assert all(0 <= f < T for f in frames) and all(x <= y for x, y in zip(frames, frames[1:]))
        assert abs(loglik - ref["loglik"]) <= bound and abs(best - ref["best"]) <= bound


def test_history_calls_leave_the_stream_as_it_was(world):
    """a twin of stream 0 (same audio, calls of its own, no history call) against stream 0 after greedy, beam and align calls over it"""
    eng, st, pcm, n = world["eng"], world["sts"][0], world["pcms"][0], world["n"]
    more = synth.make_pcm(1100, 6 * n / 16000 + 0.3)
    twin = eng.stream(0)
    feed(eng, [twin], [pcm], n)
    counters = {k: eng.counter(k) for k in ("graph_execs", "graph_shapes")}
    rng, rows = st.history_range(), st.history(*st.history_range())
    eng.history_transcribe([st], [(0, rng[1])])
    eng.history_beam([st], [(3, rng[1] - 3)])
    eng.history_align([st], [(0, rng[1])], [world["toks"][0]])
    assert st.history_range() == rng and st.history(*rng).tobytes() == rows.tobytes()
    assert {k: eng.counter(k) for k in counters} == counters
    assert st.tap(capi.TAP_DEC_STATE).tobytes() == twin.tap(capi.TAP_DEC_STATE).tobytes()
    a, b = feed(eng, [st], [more], n), feed(eng, [twin], [more], n)
    assert a == b and done_of(st) >= rng[1] + 6 and st.token_frames() == twin.token_frames()
    assert st.tap(capi.TAP_DEC_STATE).tobytes() == twin.tap(capi.TAP_DEC_STATE).tobytes()
    assert st.history(*st.history_range()).tobytes() == twin.history(*twin.history_range()).tobytes()
    twin.destroy()


@pytest.fixture(scope="module")
def W_speech():
    return synth.make_weights(24, margins="speech")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_greedy_second_pass_returns_the_streams_own_decode(W_speech, dtype):
    R = 13
    pcm = synth.make_speech_pcm(3, 4.0)[0]
    eng = engine(W_speech, dtype, L=24, options=(("token_logprobs", 1),))
    st = eng.stream(R)
    toks = feed(eng, [st], [pcm], synth.shift_samples(R))[0]
    T = done_of(st)
    frames, lps = st.token_frames(), st.token_logprobs()
    got_t, got_f = eng.history_transcribe([st], [(0, T)])
    d = float(np.abs(eng.offline_token_logprobs(0) - lps).max()) if toks else 0.0
    print(f"greedy second pass: {T} frames, {len(toks)} tokens, max |d lp| live vs second pass = {d:.3e}")
    assert T >= 45 and len(toks) >= 5
    assert got_t[0] == toks and got_f[0] == frames               # the rule for a near-tie: module docstring
    assert d < LP_BOUND
    eng.close()


# ---- the command-line tool -----------------------------------------------------------------------------------------------------------------
BIN = Path(__file__).resolve().parent.parent / "nemotron-asr.cpp_amd" / "bin"
HYP = re.compile(r"(\d) (-?\d+\.\d{6}) ?(.*)")


def run_cli(model, audio, *flags):
    r = subprocess.run([str(BIN / "nemotron-asr-amd"), str(model), str(audio), "80", "0", *flags], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    return r.stdout.splitlines(), r.stderr


def test_cli_second_pass_on_the_speech_checkpoint(W_speech, tmp_path):
    """nemotron-asr-amd --second-pass 4 --nbest 2 without endpointing: the whole input is one utterance, two hypotheses are printed before
    the transcript's line, and the best one's text is the greedy text"""
    model, audio = tmp_path / "speech.gguf", tmp_path / "a.pcm"
    gguf_io.write_gguf(model, W_speech, gguf_io.default_hparams(n_layers=24), gguf_io.synthetic_vocab())
    synth.make_speech_pcm(3, 4.0)[0].tofile(audio)
    plain, _ = run_cli(model, audio)
    got, _ = run_cli(model, audio, "--second-pass", "4", "--nbest", "2")
    assert len(got) == len(plain) + 2 and got[2:] == plain and plain[0].strip()
    hyps = [HYP.fullmatch(ln) for ln in got[:2]]
    assert all(hyps) and [int(h[1]) for h in hyps] == [0, 1] and float(hyps[0][2]) >= float(hyps[1][2])
    assert hyps[0][3].strip() == plain[0].strip()


def test_cli_second_pass_at_every_endpoint(WS, tmp_path):
    """with --endpoints: two hypotheses for every utterance the detector closes and for the one still open at the end, in the order of the
    `endpoint` lines; every other line is the output without --second-pass.  An utterance longer than the frames kept gets the notice and
    its greedy text"""
    model, audio = tmp_path / "model.gguf", tmp_path / "a.pcm"
    gguf_io.write_gguf(model, WS, gguf_io.default_hparams(n_layers=2), gguf_io.synthetic_vocab())
    synth.make_pcm(5, 6.0).tofile(audio)
    ep = ["--f32", "--endpoints", "--endpoint-idle", "0.48", "--endpoint-silence", "0.24", "--endpoint-max", "3.2"]
    plain, _ = run_cli(model, audio, *ep)
    utts = [re.fullmatch(r"endpoint (\d+\.\d\d) (\d+\.\d\d) rule (\d) tokens (\d+):(.*)", ln) for ln in plain]
    utts = [u for u in utts if u]
    assert len(utts) >= 2
    got, err = run_cli(model, audio, *ep, "--second-pass", "4", "--nbest", "2")
    n_hyp = len(got) - len(plain)
    assert got[n_hyp:] == plain and err.count("second pass: utterance") == len(utts)
    hyps = [HYP.fullmatch(ln) for ln in got[:n_hyp]]
    assert all(hyps)
    ranks = [int(h[1]) for h in hyps]
    assert ranks.count(0) == len(utts) and n_hyp <= 2 * len(utts) and ranks.count(1) >= 1
    assert all(b == 1 and a == 0 for a, b in zip(ranks, ranks[1:]) if b != 0)          # 0 [1] 0 [1] ...: at most two per utterance, best first
    # 64 frames kept, one utterance of the whole input (75 frames): the notice with the greedy text
    whole, _ = run_cli(model, audio, "--f32")
    short, _ = run_cli(model, audio, "--f32", "--second-pass", "4", "--history-frames", "64")
    m = re.fullmatch(r"second pass: the utterance's (\d+) frames are not all among the 64 kept; greedy:(.*)", short[0])
    assert m and int(m[1]) > 64 and m[2].strip() == whole[0].strip() and short[1:] == whole
