"""Stream fork (nasr_stream_fork: one k_stream_fork launch copies the live part of a slot into a free one) and the non-destructive tail
preview built on it (nasr_engine_preview), through the C ABI.

The reference of every comparison is a CONTROL: a stream of a second engine that was never forked and was fed the same audio in the same
pushes from its start.  For bit comparisons every stream is stepped in a call of its own (B = 1) on both sides, so that both run the same
launch shapes; a fork and its control then differ in nothing but the slot, and tokens, frames, token log-probabilities, the K = 3
alternatives and the per-frame blank log-probabilities are compared bit for bit over the whole stream from its create.

Before every fork the destination slot is dirtied: a stream that lands in it (the lowest free slot, as the fork will) is pushed other audio
with every option on and destroyed, so that a piece of state the fork forgot holds foreign data, not the zeros of a fresh engine."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi, gguf_io, synth

pytestmark = pytest.mark.gpu

LP_BOUND = 2e-4                      # tests/test_gpu_logprobs.py: two rows of one call
KVC = 326
ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "nemotron-asr.cpp_amd" / "bin"
OPTS = (("token_logprobs", 1), ("token_alternatives", 3), ("frame_blank_logprobs", 1))


@pytest.fixture(scope="module")
def W2():
    return synth.make_weights(n_layers=2)


def _engine(W, dtype, max_streams, options=OPTS):
    eng = capi.Engine(W, n_layers=2, dtype=dtype, max_streams=max_streams)
    for k, v in options:
        eng.set_option(k, v)
    return eng


@pytest.fixture(scope="module")
def pairs(W2):
    """dtype -> (engine under test, control engine), every read-out option on; the tests leave no stream behind"""
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = (_engine(W2, dtype, 4), _engine(W2, dtype, 4))
        return made[dtype]
    yield get
    for eng, ctl in made.values():
        eng.close()
        ctl.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).tolist()


def _readouts(st):
    ids, lps = st.token_alternatives()
    return dict(frames=st.token_frames(), lps=_bits(st.token_logprobs()), alt_ids=ids.tolist(), alt_lps=_bits(lps), fb=_bits(st.frame_blank_logprobs()),
                iterations=st.stats().decode_iterations)


def _feed(eng, st, pushes, audio=False):
    toks = []
    for p in pushes:
        toks += (eng.step_audio if audio else eng.step)([st], [p])[0]
    return toks


def _end(eng, st, toks):
    """finalize in a call of its own; (all tokens, read-outs over the whole stream)"""
    toks = toks + eng.finalize([st])[0]
    out = _readouts(st)
    out["tokens"] = toks
    assert len(out["frames"]) == len(toks)
    return out


def _dirty(eng, R, seed=4242):
    """a stream in the lowest free slot, pushed three chunks of other audio and flushed, then destroyed"""
    d = eng.stream(R)
    eng.step([d], [synth.make_pcm(seed, 3.2 * synth.shift_samples(R) / 16000)])
    eng.finalize([d])
    d.destroy()


def _cut(pcm, sizes, at=0):
    out = []
    for n in sizes:
        out.append(pcm[at:at + n])
        at += n
    assert at <= pcm.size
    return out, at


def _control(ctl, R, pushes, setup=None, audio=False):
    c = ctl.stream(R)
    try:
        if setup:
            setup(c)
        return _end(ctl, c, _feed(ctl, c, pushes, audio))
    finally:
        c.destroy()


def _same(got, want, what):
    for k in ("tokens", "frames", "iterations", "lps", "alt_ids", "alt_lps", "fb"):
        assert got[k] == want[k], (what, k)


# ---- twin --------------------------------------------------------------------------------------------------------------------------------
def _fork_point(point, R):
    """push sizes up to the fork, seconds of audio needed in all"""
    n = synth.shift_samples(R)
    if point == "fresh":
        return []
    if point == "one_chunk":
        return [2 * n]
    if point == "mid_chunk":
        return [7777] * 3
    if point == "kv_wrap":          # kv_head = chunks x T in 257 .. 325: 20 chunks of 14 frames, 264 of one
        return [4 * n] * 5 if R == 13 else [64 * n] * 4 + [8 * n]
    if point == "mel_wrap":         # more than 4096 mel frames pushed: the ring's window has wrapped; 5.12 s a push
        return [81920] * 9
    raise ValueError(point)


@pytest.mark.parametrize("R", [0, 13])
@pytest.mark.parametrize("dtype", [capi.DTYPE_F32, capi.DTYPE_BF16])
@pytest.mark.parametrize("point", ["fresh", "one_chunk", "mid_chunk", "kv_wrap", "mel_wrap"])
def test_twin(pairs, point, dtype, R):
    """source and fork, fed the same remaining audio and finalized, both equal the control bit for bit"""
    eng, ctl = pairs(dtype)
    n = synth.shift_samples(R)
    sizes = _fork_point(point, R)
    pcm = synth.make_pcm(11 + R, (sum(sizes) + 7777 + n + 5000) / 16000 + 0.4)
    prefix, at = _cut(pcm, sizes)
    suffix, at = _cut(pcm, [7777, n, 5000], at)
    suffix.append(pcm[at:])
    src = eng.stream(R)
    fork = None
    try:
        pre = _feed(eng, src, prefix)
        p = src.progress()
        if point == "one_chunk":
            assert p.chunks >= 1
        if point == "mid_chunk":
            assert p.mel_frames_buffered > 9
        if point == "kv_wrap":
            assert p.chunks * (1 + R) < KVC and 257 <= p.chunks * (1 + R) <= 325, p.chunks
        if point == "mel_wrap":
            assert p.samples_in // 160 > 4096 + 121
        _dirty(eng, R)
        forks0 = eng.counter("stream_forks")
        fork = src.fork()
        assert eng.counter("stream_forks") == forks0 + 1
        q = fork.progress()
        assert (q.samples_in, q.chunks, q.cache_valid_len, q.mel_frames_buffered) == (p.samples_in, p.chunks, p.cache_valid_len, p.mel_frames_buffered)
        got_src = _end(eng, src, pre + _feed(eng, src, suffix))
        got_fork = _end(eng, fork, pre + _feed(eng, fork, suffix))
    finally:
        src.destroy()
        if fork:
            fork.destroy()
    want = _control(ctl, R, prefix + suffix)
    print(f"twin {point} dtype {dtype} R {R}: {len(want['tokens'])} tokens, {len(want['fb'])} frames")
    assert len(want["tokens"]) >= 1
    _same(got_src, want, "source")
    _same(got_fork, want, "fork")


@pytest.mark.parametrize("dtype,R", [(capi.DTYPE_F32, 13), (capi.DTYPE_BF16, 0)])
def test_independence(pairs, dtype, R):
    """source and fork fed DIFFERENT audio each equal their own control (prefix + own suffix): the source is untouched, the fork is no alias"""
    eng, ctl = pairs(dtype)
    n = synth.shift_samples(R)
    prefix, _ = _cut(synth.make_pcm(21, 2.0), [7777] * 3)
    suf_a, _ = _cut(synth.make_pcm(22, (3 * n + 9000) / 16000), [7777, 2 * n, n + 1223])
    suf_b, _ = _cut(synth.make_pcm(23, (3 * n + 9000) / 16000), [7777, 2 * n, n + 1223])
    src = eng.stream(R)
    fork = None
    try:
        pre = _feed(eng, src, prefix)
        _dirty(eng, R)
        fork = src.fork()
        ta, tb = list(pre), list(pre)
        for a, b in zip(suf_a, suf_b):                                 # interleaved: each step of one lies between two steps of the other
            ta += eng.step([src], [a])[0]
            tb += eng.step([fork], [b])[0]
        got_b = _end(eng, fork, tb)
        got_a = _end(eng, src, ta)
    finally:
        src.destroy()
        if fork:
            fork.destroy()
    want_a, want_b = _control(ctl, R, prefix + suf_a), _control(ctl, R, prefix + suf_b)
    assert want_a["tokens"] != want_b["tokens"]
    _same(got_a, want_a, "source")
    _same(got_b, want_b, "fork")


# ---- carried decoder state ---------------------------------------------------------------------------------------------------------------
def _calls(eng, st, pcm, n):
    """one chunk per call at R = 0: the tokens of every call"""
    return [eng.step([st], [pcm[o:o + n]])[0] for o in range(0, pcm.size - n + 1, n)]


def _next_after(calls, i):
    """(the last token of call i, the first token of a later call)"""
    later = [t for c in calls[i + 1:] for t in c]
    return (calls[i][-1] if calls[i] else None, later[0] if later else None)


def test_boost_and_lm_state_travel(W2):
    """phrase_boost and lm_fusion on, non-zero weights, and a fork between the two tokens of a phrase.

    The phrase is picked from the control's own output: a call of the plain run ends with t1, the next token t2 comes in a later call, and X
    is the model's best other token where t2 was emitted, g = ln P(t2) - ln P(X) behind it.  The LM scores every token -6 (its bias
    0.5 x -6 + 3 = 0 exactly: it changes nothing) except X after t1, whose bias is g - 5e-5; the boost set is the phrase (t1, X) with bonus
    1e-4.  Neither alone lifts X over t2, both together do, by 5e-5 (fifty times the rounding of the f32 values involved): X follows t1
    only in a stream whose automaton stands inside the phrase AND whose LM history is t1.  The control confirms that before a candidate is
    taken (runs with both on, boost off, LM off; the output up to t1 unchanged).  The fork is made right after the call that emitted t1,
    into a slot that a boosted and fused stream of other audio has left"""
    R, n = 0, synth.shift_samples(0)
    opts = OPTS + (("phrase_boost", 64), ("lm_fusion", 1))
    eng, ctl = _engine(W2, capi.DTYPE_F32, 3, opts), _engine(W2, capi.DTYPE_F32, 3, opts)
    try:
        c = ctl.stream(R)

        def run(pcm, boost=True, lm=True):
            c.reset()
            c.set_boost(boost)
            c.set_lm(lm)
            return _calls(ctl, c, pcm, n)
        picked, tried = None, 0
        for seed in (31, 33, 35):
            pcm = synth.make_pcm(seed, 12.0)
            ctl.set_boost_phrases([], None)
            ctl.set_lm(None)
            plain = run(pcm)                                           # no phrases, no model: the unfused decode
            ids, lps = c.token_alternatives()
            cands, idx = [], 0
            for i, call in enumerate(plain[:-2]):
                idx += len(call)
                later = [t for c2 in plain[i + 1:] for t in c2]
                if i < 1 or not call or not later:
                    continue
                assert int(ids[idx][0]) == later[0]                    # unboosted, unfused: the token is the model's first
                for k in (1, 2):
                    X, g = int(ids[idx][k]), float(lps[idx][0]) - float(lps[idx][k])
                    if X not in (1024, call[-1]) and g >= 1e-3:
                        cands.append((i, call[-1], later[0], X, g))
                        break
            for i, t1, t2, X, g in cands:
                tried += 1
                for e in (eng, ctl):
                    e.set_boost_phrases([[t1, X]], 1e-4)
                    e.set_lm({(t1,): (-6.0, 0.0), (X,): (-6.0, 0.0), (t1, X): (-6.0 + 2.0 * (g - 5e-5), 0.0)}, order=2, unk_logprob=-6.0)
                    e.set_greedy_lm_weights(0.5, 3.0)
                no_boost, no_lm, both = run(pcm, boost=False), run(pcm, lm=False), run(pcm)
                if (_next_after(both, i) == (t1, X) and _next_after(no_boost, i) == (t1, t2) and _next_after(no_lm, i) == (t1, t2)
                        and both[:i + 1] == plain[:i + 1]):
                    picked = (i, t1, t2, X, g)
                    break
            if picked:
                break
        assert picked, f"none of {tried} call boundaries of the control's output gave a phrase that needs both states"
        i, t1, t2, X, g = picked
        print(f"carried state: after {t1} the model says {t2}, boost + LM say {X} (gap {g:.3e}); fork after call {i} of {len(both)}, candidate {tried}")
        want = _end(ctl, c, [t for call in both for t in call])
        src = eng.stream(R)
        calls = [pcm[o:o + n] for o in range(0, pcm.size - n + 1, n)]
        pre = _feed(eng, src, calls[:i + 1])
        assert pre[-1] == t1
        d = eng.stream(R)                                              # the dirty slot: boosted and fused, another history
        _feed(eng, d, [synth.make_pcm(32, 2.0)])
        d.destroy()
        fork = src.fork()
        got_fork = _end(eng, fork, pre + _feed(eng, fork, calls[i + 1:]))
        got_src = _end(eng, src, pre + _feed(eng, src, calls[i + 1:]))
        assert got_fork["tokens"][len(pre)] == X and got_src["tokens"][len(pre)] == X
        _same(got_src, want, "source")
        _same(got_fork, want, "fork")
    finally:
        eng.close()
        ctl.close()


def test_boost_off_and_an_audio_format_of_its_own(W2):
    """a stream with set_boost(False) forked keeps boosting off; a 48 kHz mu-law stream forked mid-push (the converter's history, counters
    and parity travel) goes on through step_audio"""
    opts = OPTS + (("phrase_boost", 64),)
    eng, ctl = _engine(W2, capi.DTYPE_BF16, 3, opts), _engine(W2, capi.DTYPE_BF16, 3, opts)
    try:
        R, n = 0, synth.shift_samples(0)
        pcm = synth.make_pcm(41, 4.0)
        pushes, _ = _cut(pcm, [7777] * 8)
        c = ctl.stream(R)
        plain = _end(ctl, c, _feed(ctl, c, pushes))
        c.destroy()
        for e in (eng, ctl):
            e.set_boost_phrases([[t] for t in sorted(set(plain["tokens"]))[:3]] + [[int(t) for t in range(5)]], 6.0)
        boosted = _control(ctl, R, pushes)
        assert boosted["tokens"] != plain["tokens"]                    # the set matters where it is on
        src = eng.stream(R)
        src.set_boost(False)
        pre = _feed(eng, src, pushes[:3])
        _dirty(eng, R)                                                 # a boosted stream in the slot
        fork = src.fork()
        got_fork = _end(eng, fork, pre + _feed(eng, fork, pushes[3:]))
        got_src = _end(eng, src, pre + _feed(eng, src, pushes[3:]))
        want = _control(ctl, R, pushes, setup=lambda s: s.set_boost(False))
        assert want["tokens"] == plain["tokens"]
        _same(got_src, want, "boost off: source")
        _same(got_fork, want, "boost off: fork")
        src.destroy()
        fork.destroy()
        # 48 kHz mu-law, pushes that are no multiple of anything
        raw = ((synth.make_pcm(42, 4.0 * 3).astype(np.int32) >> 8) + 128).astype(np.uint8)
        apush, _ = _cut(raw, [23333] * 8)
        fmt = lambda s: s.set_audio_format(48000, "mulaw")
        src = eng.stream(R)
        fmt(src)
        pre = _feed(eng, src, apush[:3], audio=True)
        _dirty(eng, R)
        fork = src.fork()
        got_fork = _end(eng, fork, pre + _feed(eng, fork, apush[3:], audio=True))
        got_src = _end(eng, src, pre + _feed(eng, src, apush[3:], audio=True))
        want = _control(ctl, R, apush, setup=fmt, audio=True)
        assert len(want["tokens"]) >= 1
        _same(got_src, want, "mu-law: source")
        _same(got_fork, want, "mu-law: fork")
    finally:
        eng.close()
        ctl.close()


# ---- same call, pipelined ----------------------------------------------------------------------------------------------------------------
def test_source_and_fork_in_one_call(pairs):
    """stepped together (B = 2) they give equal tokens and frames; two rows of a call are not promised equal bits, so the
    log-probabilities are held to LP_BOUND"""
    eng, _ = pairs(capi.DTYPE_BF16)
    R, n = 13, synth.shift_samples(13)
    pcm = synth.make_pcm(24, (6 * n + 7777) / 16000)
    prefix, at = _cut(pcm, [7777])                                     # the fork comes before the stream's first chunk: its tokens come after
    suffix, _ = _cut(pcm, [2 * n, n, 3 * n - 100], at)
    src = eng.stream(R)
    fork = None
    try:
        _feed(eng, src, prefix)
        _dirty(eng, R)
        fork = src.fork()
        ta, tb = [], []
        for p in suffix:
            a, b = eng.step([src, fork], [p, p])
            ta, tb = ta + a, tb + b
        a, b = eng.finalize([src, fork])
        assert ta + a == tb + b and len(ta + a) >= 1
        assert src.token_frames() == fork.token_frames()
        la, lb = src.token_logprobs(), fork.token_logprobs()
        assert la.shape == lb.shape and float(np.abs(la.astype(np.float64) - lb).max(initial=0.0)) < LP_BOUND
        fa, fb = src.frame_blank_logprobs(), fork.frame_blank_logprobs()
        assert fa.shape == fb.shape and float(np.abs(fa.astype(np.float64) - fb).max(initial=0.0)) < LP_BOUND
    finally:
        src.destroy()
        if fork:
            fork.destroy()


def test_fork_and_preview_with_pipelined_steps_in_flight(W2, pairs):
    """pipeline = 4: the destination slot is dirtied BEFORE the pipelined pushes, and the fork is made straight after the pipelined step of
    the stream's first chunk, while that step is in flight -- shown by its tokens, which the synchronous control has delivered by then and
    this engine has not.  The fork call completes it first: the tokens then wait on both streams.  The same, on a second stream, for a
    preview.  After the last collect every stream has the tokens and frames of the synchronous control"""
    _, ctl = pairs(capi.DTYPE_BF16)
    eng = _engine(W2, capi.DTYPE_BF16, 3)
    eng.set_option("pipeline", 4)
    try:
        R, n = 13, synth.shift_samples(13)
        pcm = synth.make_pcm(24, 12 * n / 16000 + 0.5)
        pushes = [pcm[o:o + n] for o in range(0, 12 * n, n)] + [pcm[12 * n:]]
        c = ctl.stream(R)                                              # the synchronous control after two pushes, and what finalize adds then
        sync2 = _feed(ctl, c, pushes[:2])
        tail2 = ctl.finalize([c])[0]
        tail2_frames = c.token_frames()[len(sync2):]
        c.destroy()
        want = _control(ctl, R, pushes)
        assert len(sync2) >= 1 and len(want["tokens"]) >= 1

        def rest(st, toks, k):
            toks = toks + _feed(eng, st, pushes[k:])
            return toks + eng.finalize([st])[0] + eng.collect([st])[0]
        src = eng.stream(R)
        _dirty(eng, R)                                                 # lands in the slot the fork will take; completes what it started itself
        pre = _feed(eng, src, pushes[:2])
        assert eng.counter("pipelined_steps") >= 1
        assert len(pre) < len(sync2) and src.progress().reserved == 0, "no step is in flight: nothing of the first chunk is outstanding"
        fork = src.fork()                                              # straight after a pipelined step
        assert fork.progress().reserved == src.progress().reserved == len(sync2) - len(pre)      # completed: its tokens wait on both streams
        tb = rest(fork, pre, 2)
        ta = rest(src, pre, 2)
        assert ta == want["tokens"] and tb == want["tokens"]
        assert src.token_frames() == want["frames"] and fork.token_frames() == want["frames"]
        fork.destroy()
        src.reset()                                                    # the same stream again, its twin's slot free and used
        pre = _feed(eng, src, pushes[:2])
        assert len(pre) < len(sync2) and src.progress().reserved == 0
        (ptoks, pframes), = eng.preview([src], frames=True)
        assert (ptoks, pframes) == (tail2, tail2_frames)
        assert src.progress().reserved == len(sync2) - len(pre)        # the preview completed the step; its tokens are the stream's, not the preview's
        ta = rest(src, pre, 2)
        assert ta == want["tokens"] and src.token_frames() == want["frames"]
    finally:
        eng.close()


# ---- preview -----------------------------------------------------------------------------------------------------------------------------
def test_preview(W2):
    """at 0.3 s, 0.6 s and 1.0 s into a chunk of a right_context 13 stream the preview is what finalize returns on a control fed the same
    prefix; the previewed stream ends bitwise equal to a control that was never previewed; the slots come back; a batch of three"""
    eng, ctl = _engine(W2, capi.DTYPE_BF16, 6), _engine(W2, capi.DTYPE_BF16, 6)
    try:
        R, n = 13, synth.shift_samples(13)
        pcm = synth.make_pcm(71, (4 * n + 16000) / 16000 + 0.3)
        sizes = [2 * n, 4800, 4800, 6400, 2 * n]
        pushes, at = _cut(pcm, sizes)
        pushes.append(pcm[at:])
        st = eng.stream(R)
        assert eng.preview([st]) == [[]]                               # nothing buffered but the nine start frames
        assert st.progress().mel_frames_buffered <= 9 and eng.counter("stream_previews") == 1
        toks, n_nonempty = [], 0
        for k, p in enumerate(pushes):
            toks += eng.step([st], [p])[0]
            if k in (1, 2, 3):
                before = (st.progress().samples_in, st.progress().mel_frames_buffered, st.stats().tokens)
                _dirty(eng, R, seed=900 + k)
                (ptoks, pframes), = eng.preview([st], frames=True)
                assert (st.progress().samples_in, st.progress().mel_frames_buffered, st.stats().tokens) == before
                c = ctl.stream(R)
                head = _feed(ctl, c, pushes[:k + 1])
                tail = ctl.finalize([c])[0]
                assert head == toks and ptoks == tail and pframes == c.token_frames()[len(head):], k
                c.destroy()
                n_nonempty += bool(ptoks)
                print(f"preview at push {k}: {len(ptoks)} tentative tokens")
        assert n_nonempty >= 1
        assert eng.counter("stream_previews") == 4 and eng.counter("stream_forks") == 4
        got = _end(eng, st, toks)
        _same(got, _control(ctl, R, pushes), "the previewed stream")
        # the slots were released: max_streams streams can exist again
        more = [eng.stream(R) for _ in range(5)]
        with pytest.raises(capi.NasrError, match=r"stream pool exhausted \(max_streams=6\)"):
            eng.stream(R)
        for s in more[2:]:
            s.destroy()
        # a batch of three previews (three free slots), each stream at another point of its chunk
        trio, ctrio = [st] + more[:2], [ctl.stream(R) for _ in range(3)]
        for s in trio + ctrio:
            s.reset()
        cuts = [pcm[:2 * n + 4000], pcm[:n + 9000], pcm[:3 * n + 15000]]
        assert eng.step(trio, cuts) == ctl.step(ctrio, cuts)
        prev = eng.preview(trio, frames=True)
        tails = ctl.finalize(ctrio)
        assert [t for t, _ in prev] == tails and sum(len(t) for t in tails) >= 1
        for (t, f), c in zip(prev, ctrio):
            assert f == c.token_frames()[len(c.token_frames()) - len(t):]
        assert eng.finalize(trio) == tails                             # ... and the streams themselves still have their tails to give
    finally:
        eng.close()
        ctl.close()


# ---- errors, graphs ----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_engine_usable(W2, pairs):
    _, ctl = pairs(capi.DTYPE_BF16)
    eng = _engine(W2, capi.DTYPE_BF16, 2)
    try:
        R, n = 0, synth.shift_samples(0)
        pcm = synth.make_pcm(81, 2.5)
        pushes, _ = _cut(pcm, [7777] * 5)
        a, b = eng.stream(R), eng.stream(R)
        toks = _feed(eng, a, pushes[:2])
        with pytest.raises(capi.NasrError, match=r"stream pool exhausted \(max_streams=2\)"):
            a.fork()
        with pytest.raises(capi.NasrError, match=r"1 free slot\(s\) missing"):
            eng.preview([a])
        with pytest.raises(capi.NasrError, match=r"2 free slot\(s\) missing"):
            eng.preview([a, b])
        out = C.c_void_p(1)
        assert capi.lib().nasr_stream_fork(None, C.byref(out)) < 0 and b"null" in capi.lib().nasr_last_error()
        assert capi.lib().nasr_stream_fork(a.h, None) < 0
        dead = C.c_void_p(b.h.value)                                   # a destroyed stream is refused, not read
        b.destroy()
        assert capi.lib().nasr_stream_fork(dead, C.byref(out)) < 0 and b"not a live stream" in capi.lib().nasr_last_error()
        assert out.value is None
        assert eng.counter("stream_forks") == 0 and eng.counter("stream_previews") == 0
        got = _end(eng, a, toks + _feed(eng, a, pushes[2:]))
        _same(got, _control(ctl, R, pushes), "after the refused calls")
    finally:
        eng.close()


def test_forks_between_graph_steps_keep_the_graphs(pairs):
    """20 forks between graph steps: every step is still a graph replay, nothing is evicted or captured anew"""
    eng, _ = pairs(capi.DTYPE_BF16)
    R, n = 0, synth.shift_samples(0)
    pcm = synth.make_pcm(91, 30 * n / 16000)
    st = eng.stream(R)
    try:
        for k in range(6):
            eng.step([st], [pcm[k * n:(k + 1) * n]])
        replays, evictions, shapes, forks = (eng.counter(k) for k in ("graph_replays", "graph_evictions", "graph_shapes", "stream_forks"))
        for k in range(6, 26):
            f = st.fork()
            eng.step([st], [pcm[k * n:(k + 1) * n]])
            assert eng.counter("graph_replays") == replays + (k - 5)
            f.destroy()
        assert eng.counter("graph_evictions") == evictions and eng.counter("graph_shapes") == shapes and eng.counter("stream_forks") == forks + 20
    finally:
        st.destroy()


def test_debug_taps(W2):
    """a fork's taps are empty until its own first call; a preview leaves the source's taps, the per-call staged ones included, as they were"""
    eng = _engine(W2, capi.DTYPE_BF16, 3)
    eng.set_debug(True)
    try:
        R, n = 13, synth.shift_samples(13)
        st = eng.stream(R)
        st.set_audio_format(48000, "mulaw")
        raw = ((synth.make_pcm(43, 13.0).astype(np.int32) >> 8) + 128).astype(np.uint8)
        eng.step_audio([st], [raw[:3 * (2 * n + 5000)]])
        which = (capi.TAP_MEL, capi.TAP_PCM16, capi.TAP_SUBSAMPLED, capi.TAP_ENCODER_OUT)
        before = [st.tap(w) for w in which]
        assert all(t.size > 0 for t in before)
        fork = st.fork()
        assert [fork.tap(w).size for w in which] == [0, 0, 0, 0]
        fork.destroy()
        _dirty(eng, R)
        eng.step_audio([st], [raw[3 * (2 * n + 5000):3 * (3 * n + 9000)]])
        before = [st.tap(w) for w in which]
        assert all(t.size > 0 for t in before)
        assert eng.preview([st]) is not None
        after = [st.tap(w) for w in which]
        for x, y in zip(before, after):
            assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))
    finally:
        eng.close()


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_preview_lines(W2, tmp_path):
    """nemotron-asr-amd --preview: the lines without `~ ` are the run without the flag, byte for byte; one `~ ` line per read, some with text"""
    gguf_io.write_gguf(tmp_path / "model.gguf", W2, gguf_io.default_hparams(n_layers=2), gguf_io.synthetic_vocab())
    synth.make_pcm(95, 8.0).tofile(tmp_path / "a.pcm")
    cli = [str(BIN / "nemotron-asr-amd"), str(tmp_path / "model.gguf"), str(tmp_path / "a.pcm"), "80", "13", "--print-tokens"]
    plain = subprocess.run(cli, capture_output=True, timeout=120)
    with_flag = subprocess.run(cli + ["--preview"], capture_output=True, timeout=120)
    assert plain.returncode == 0 and with_flag.returncode == 0, with_flag.stderr[-800:]
    lines = with_flag.stdout.split(b"\n")
    tilde = [ln for ln in lines if ln.startswith(b"~ ")]
    assert b"\n".join(ln for ln in lines if not ln.startswith(b"~ ")) == plain.stdout
    assert not any(ln.startswith(b"~ ") for ln in plain.stdout.split(b"\n"))
    assert len(plain.stdout.split(b"\n")[-2].split()) > 1              # TOKENS: and at least one id
    assert len(tilde) >= 5 and any(len(ln) > 2 for ln in tilde)
