"""Device-side audio input conversion (nasr_stream_set_audio_format / nasr_engine_step_audio / nasr_engine_convert_audio) through the C ABI.

The kernel is held against csrc/nasr_resample.h itself: tests/resample_ref.py compiles the header's host restatement into a stand-alone
program (g++, no FMA contraction), and every comparison of samples here is np.array_equal.  What the header computes is checked against a
float64 reference, under AddressSanitizer / UBSan, in tests/test_resample_math.py (CPU)."""
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi
from tests import resample_ref as rr

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_audio")
    return rr.build_driver(d, ROOT, sanitize=False), d


@pytest.fixture(scope="module")
def eng(weights2):
    e = capi.Engine(weights2, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=8)
    e.set_option("token_logprobs", 1)
    yield e
    e.close()


def _g711_encode(x, law):
    tab = rr.mulaw_table() if law == "mulaw" else rr.alaw_table()
    order = np.argsort(tab, kind="stable")
    idx = np.clip(np.searchsorted(tab[order], np.rint(x * 32767).astype(np.int64)), 0, 255)
    return order[idx].astype(np.uint8)


def _audio(fin, enc, channels, frames, seed):
    """[frames * channels] in the encoding's dtype: a tone per channel under a 3 Hz envelope, plus noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames) / fin
    cols = []
    for c in range(channels):
        f0 = 180.0 + 70.0 * c + 13.0 * (seed % 7)
        cols.append(0.35 * np.sin(2 * np.pi * f0 * t + c) * (0.55 - 0.45 * np.cos(2 * np.pi * 3.0 * t)) + 0.05 * rng.standard_normal(frames))
    x = np.stack(cols, axis=1).reshape(-1)
    if enc == "s16":
        return np.rint(np.clip(x, -1, 1) * 32767).astype(np.int16)
    if enc == "f32":
        return x.astype(np.float32)
    return _g711_encode(np.clip(x, -1, 1), enc)


def _frames_with_total(fin, want_mod, lo=3000, hi=6000):
    """an input length in [lo, hi] whose flushed output ends want_mod samples past a workgroup boundary (256 outputs per workgroup).  At
    8 kHz every total is even: 255 and 257 become 254 and 258 there."""
    for mod in (want_mod, want_mod + (1 if want_mod > 256 else -1)):
        for n in range(hi, lo - 1, -1):
            if rr.out_total(fin, n) % 256 == mod % 256 and rr.out_total(fin, n) > 256:
                return n, mod
    raise AssertionError((fin, want_mod))


def _kernel_cases():
    cases = []
    for fin in rr.RATES:
        for enc in ("s16", "f32", "mulaw", "alaw"):
            for mod in (255, 256, 257):
                cases.append((fin, enc, 1, 0, mod))
    for fin in (8000, 44100, 48000):
        for mod in (255, 256, 257):
            cases.append((fin, "f32", 2, (0, 1, -1)[mod - 255], mod))          # stereo: channel 0, channel 1, mix
        cases.append((fin, "s16", 3, -1, 256))                                   # three channels mixed
        cases.append((fin, "mulaw", 2, -1, 257))
    for fin in rr.RATES:
        L, _, half = rr.plan(fin)
        for n in (0, 1, 2 * half // L):
            cases.append((fin, "s16", 1, 0, -n))                                 # the length itself (negative marks it)
    return cases


def test_kernel_equals_the_header_bit_for_bit(eng, drv):
    prog, d = drv
    n_checked = 0
    for k, (fin, enc, channels, channel, mod) in enumerate(_kernel_cases()):
        frames, mod = (-mod, mod) if mod <= 0 else _frames_with_total(fin, mod)
        x = _audio(fin, enc, channels, frames, 100 + k)
        want = rr.convert(prog, d, x.tobytes(), fin, enc, channels, channel, tag="k")
        got = eng.convert_audio(capi.audio_format(fin, enc, channels, channel), x)
        assert got.dtype == np.int16 and got.size == rr.out_total(fin, frames) == want.size, (fin, enc, channels, channel, frames)
        assert np.array_equal(got, want), (fin, enc, channels, channel, frames, int(np.abs(got.astype(int) - want.astype(int)).max()))
        if mod > 0:
            assert got.size % 256 == mod % 256
        n_checked += 1
    assert n_checked == 96 + 15 + 24
    # non-finite f32 input reads as silence, on the device as in the header
    x = _audio(48000, "f32", 1, 3000, 5)
    x[[0, 7, 1500, 2999]] = [np.nan, np.inf, -np.inf, np.nan]
    assert np.array_equal(eng.convert_audio(capi.audio_format(48000, "f32"), x), rr.convert(prog, d, x.tobytes(), 48000, "f32", tag="nan"))


@pytest.mark.parametrize("lds", [0, 1])
def test_coefficients_from_lds_or_global_memory_give_the_same_bits(weights2, drv, lds):
    """engine option "audio_lds_table" (default 1): the rates whose table fits (L <= 2) read it from LDS; 44.1 kHz keeps the global table"""
    prog, d = drv
    e = capi.Engine(weights2, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    try:
        e.set_option("audio_lds_table", lds)
        for k, (fin, enc, channels, channel) in enumerate([(8000, "mulaw", 1, 0), (24000, "s16", 1, 0), (32000, "f32", 2, -1), (48000, "s16", 1, 0), (44100, "s16", 1, 0)]):
            x = _audio(fin, enc, channels, _frames_with_total(fin, 257)[0], 300 + k)
            want = rr.convert(prog, d, x.tobytes(), fin, enc, channels, channel, tag="lds")
            assert np.array_equal(e.convert_audio(capi.audio_format(fin, enc, channels, channel), x), want), fin
    finally:
        e.close()


def _random_pieces(rng, frames, hist):
    pieces, left = [], frames
    while left > 0:
        n = int(rng.choice([0, 1, 2, hist - 1, hist + 1, int(rng.integers(1, 900)), int(rng.integers(200, 2000))]))
        n = min(n, left)
        pieces.append(n)
        left -= n
    return pieces


@pytest.mark.parametrize("fin,enc,channels,channel", [(8000, "mulaw", 1, 0), (44100, "f32", 2, -1), (48000, "s16", 1, 0)])
def test_streaming_equals_one_shot(eng, fin, enc, channels, channel):
    fmt = capi.audio_format(fin, enc, channels, channel)
    frames = 6000
    x = _audio(fin, enc, channels, frames, fin)
    whole = eng.convert_audio(fmt, x)
    L, _, half = rr.plan(fin)
    rng = np.random.default_rng(fin)
    eng.set_debug(True)
    try:
        for trial in range(2):
            s = eng.stream(0)
            s.set_audio_format(fin, enc, channels, channel)
            got, at = [], 0
            pieces = _random_pieces(rng, frames, 2 * half // L + 1)
            for n in [0] + pieces:                                             # an empty push first
                eng.step_audio([s], [x[at * channels:(at + n) * channels]])
                tap = s.tap(capi.TAP_PCM16)
                assert tap.size == capi.audio_out_ready(fmt, at + n) - capi.audio_out_ready(fmt, at)
                got.append(tap)
                at += n
            assert s.progress().samples_in == capi.audio_out_ready(fmt, frames)
            eng.finalize([s])
            tail = s.tap(capi.TAP_PCM16)
            assert tail.size == capi.audio_out_total(fmt, frames) - capi.audio_out_ready(fmt, frames) > 0
            got.append(tail)
            assert s.progress().samples_in == whole.size
            assert np.array_equal(np.concatenate(got).astype(np.int16), whole), (trial, pieces[:12])
            eng.finalize([s])                                                  # nothing is left to flush
            assert s.tap(capi.TAP_PCM16).size == 0
            s.destroy()
    finally:
        eng.set_debug(False)


def _results(s):
    return dict(frames=s.token_frames(), lps=s.token_logprobs().tobytes(), dec=s.tap(capi.TAP_DEC_STATE).tobytes(), stats=(s.stats().tokens, s.stats().chunks, s.stats().samples_in))


def _run_pairs(e, specs, n_push, seed):
    """specs: (fin, enc, channels, channel, frames) per stream.  Streams A take their own format through step_audio, all in one call per
    push; streams B take the one-shot conversion through step, cut where audio_out_ready says A's pushes end; then both are finalized."""
    B = len(specs)
    fmts = [capi.audio_format(*sp[:4]) for sp in specs]
    xs = [_audio(sp[0], sp[1], sp[2], sp[4], seed + i) for i, sp in enumerate(specs)]
    wholes = [e.convert_audio(f, x) for f, x in zip(fmts, xs)]
    A, Bs = [e.stream(0) for _ in range(B)], [e.stream(0) for _ in range(B)]
    for s, sp in zip(A, specs):
        if sp[:4] != (16000, "s16", 1, 0):
            s.set_audio_format(*sp[:4])
    rng = np.random.default_rng(seed)
    cuts = []
    for sp in specs:                                                            # n_push cut points per stream, the last at the end
        c = np.sort(rng.integers(0, sp[4] + 1, n_push - 1)).tolist() + [sp[4]]
        cuts.append([0] + c)
    tokA, tokB = [[] for _ in range(B)], [[] for _ in range(B)]
    for k in range(n_push):
        for b, t in enumerate(e.step_audio(A, [xs[b][cuts[b][k] * specs[b][2]:cuts[b][k + 1] * specs[b][2]] for b in range(B)])):
            tokA[b] += t
        lo = [capi.audio_out_ready(fmts[b], cuts[b][k]) for b in range(B)]
        hi = [capi.audio_out_ready(fmts[b], cuts[b][k + 1]) for b in range(B)]
        for b, t in enumerate(e.step(Bs, [wholes[b][lo[b]:hi[b]] for b in range(B)])):
            tokB[b] += t
    tails = [wholes[b][capi.audio_out_ready(fmts[b], specs[b][4]):] for b in range(B)]
    for b, t in enumerate(e.step(Bs, tails)):                                   # what A's finalize flushes
        tokB[b] += t
    for b, t in enumerate(e.finalize(A)):
        tokA[b] += t
    for b, t in enumerate(e.finalize(Bs)):
        tokB[b] += t
    out = []
    for b in range(B):
        ra, rb = _results(A[b]), _results(Bs[b])
        assert tokA[b] == tokB[b], (specs[b], len(tokA[b]), len(tokB[b]))
        assert ra == rb, specs[b]
        out.append(len(tokA[b]))
    for s in A + Bs:
        s.destroy()
    return out


FOUR = [(48000, "s16", 1, 0, 6000), (8000, "mulaw", 1, 0, 6000), (44100, "f32", 2, -1, 6000), (16000, "s16", 1, 0, 3000)]


@pytest.mark.parametrize("pipeline", [0, 4])
def test_end_to_end_equals_stepping_the_converted_samples(weights2, pipeline):
    e = capi.Engine(weights2, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=8)
    try:
        e.set_option("token_logprobs", 1)
        e.set_option("pipeline", pipeline)
        n_tok = 0
        for i, sp in enumerate(FOUR[:3] + [(48000, "s16", 1, 0, 30000)]):      # one stream at a time
            n_tok += sum(_run_pairs(e, [sp], 5, 40 + i))
        n_tok += sum(_run_pairs(e, FOUR, 5, 50))                               # four formats in one call, one of them the default
        assert n_tok > 0
    finally:
        e.close()


@pytest.mark.parametrize("fin", [48000, 44100])
def test_whole_chunk_pushes_replay_graphs(weights2, fin):
    e = capi.Engine(weights2, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=2)
    try:
        e.set_option("token_logprobs", 1)
        fmt = capi.audio_format(fin)
        L, M, _ = rr.plan(fin)
        push = 1280 * M // L                                                    # one chunk (R = 0) of input frames
        n_push = 6
        x = _audio(fin, "s16", 1, push * n_push, 9)
        whole = e.convert_audio(fmt, x)
        a, b = e.stream(0), e.stream(0)
        a.set_audio_format(fin)
        for k in range(n_push):
            c0 = (e.counter("graph_replays"), e.counter("eager_steps"))
            e.step_audio([a], [x[k * push:(k + 1) * push]])
            c1 = (e.counter("graph_replays"), e.counter("eager_steps"))
            lo, hi = capi.audio_out_ready(fmt, k * push), capi.audio_out_ready(fmt, (k + 1) * push)
            e.step([b], [whole[lo:hi]])
            c2 = (e.counter("graph_replays"), e.counter("eager_steps"))
            da, db = (c1[0] - c0[0], c1[1] - c0[1]), (c2[0] - c1[0], c2[1] - c1[1])
            assert da == db, (k, da, db)
            if k >= 1:
                assert hi - lo == 1280 and da == (1, 0), (k, hi - lo, da)
        ra, rb = _results(a), _results(b)
        assert ra["stats"][:2] == rb["stats"][:2] and ra["frames"] == rb["frames"] and ra["lps"] == rb["lps"]
    finally:
        e.close()


def test_contract(eng):
    s = eng.stream(0)
    with pytest.raises(capi.NasrError):
        s.set_audio_format(12000)
    with pytest.raises(capi.NasrError):
        s.set_audio_format(48000, 7)
    with pytest.raises(capi.NasrError):
        s.set_audio_format(48000, "s16", 2, 2)
    s.set_audio_format(48000, "f32", 2, "mix")
    x = _audio(48000, "f32", 2, 6000, 3)
    with pytest.raises(capi.NasrError) as err:                                   # nasr_engine_step refuses the stream and names the other entry
        eng.step([s], [np.zeros(1280, np.int16)])
    assert "nasr_engine_step_audio" in str(err.value)
    first = eng.step_audio([s], [x]) + eng.finalize([s])                        # ... and the engine stays usable
    with pytest.raises(capi.NasrError):                                          # after audio: refused, the old format stays
        s.set_audio_format(8000, "mulaw")
    st1 = _results(s)
    # a reset keeps the format and restarts the converter's counters (k_stream_reset also zeroes the history buffer, which no output can
    # show: a stream that starts over reads zeros in front of its first frame whatever the buffer holds)
    s.reset()
    again = eng.step_audio([s], [x]) + eng.finalize([s])
    assert again == first and _results(s) == st1
    s.reset()
    s.set_audio_format(16000)                                                    # right after a reset the format may change
    eng.step([s], [np.zeros(1280, np.int16)])
    # 10 frames at 48 kHz complete no sample: a step of zero samples, no tokens; the format is then fixed
    t = eng.stream(0)
    t.set_audio_format(48000)
    assert eng.step_audio([t], [np.zeros(10, np.int16)]) == [[]] and t.progress().samples_in == 0
    with pytest.raises(capi.NasrError):
        t.set_audio_format(8000)
    # the profile classes
    eng.profile(True)
    eng.step_audio([t], [np.zeros(4000, np.int16)])
    names = {r["name"]: r for r in eng.profile_read()}
    eng.profile(False)
    assert names["audio_convert"]["launches"] == 1 and names["audio_convert"]["flops"] > 0 and names["h2d_pcm"]["bytes"] >= 8000
    s.destroy()
    t.destroy()


def test_a_default_stream_beside_a_48k_stream_gives_the_bits_of_step(eng):
    pcm = _audio(16000, "s16", 1, 6000, 21)
    x48 = _audio(48000, "s16", 1, 6000, 22)
    d1, d2, hi = eng.stream(0), eng.stream(0), eng.stream(0)
    hi.set_audio_format(48000)
    t1, t2 = [], []
    for o in range(0, 6000, 1500):
        t1 += eng.step_audio([d1, hi], [pcm[o:o + 1500], x48[o:o + 1500]])[0]
        t2 += eng.step([d2], [pcm[o:o + 1500]])[0]
    t1 += eng.finalize([d1, hi])[0]
    t2 += eng.finalize([d2])[0]
    assert t1 == t2 and _results(d1) == _results(d2)
    for s in (d1, d2, hi):
        s.destroy()
