"""Stream snapshots in host memory (nasr_stream_save: one k_stream_pack launch + one device-to-host copy; nasr_stream_restore: one
host-to-device copy + one k_stream_unpack launch into the lowest free slot; csrc/nasr_snapshot.h), through the C ABI.

As in tests/test_gpu_stream_fork.py the reference of every comparison is a CONTROL: a never-saved stream of another engine that was fed
the same pushes from its start; every stream is stepped in calls of its own (B = 1), so a restored stream and its control differ in nothing
but the engine and the slot, and tokens, frames, decode iterations, token log-probabilities, the K = 3 alternatives and the per-frame blank
log-probabilities are compared bit for bit over the whole stream.  No tolerance.  Before every restore the destination slot is dirtied
(_dirty): what a restore forgot then holds foreign data, not the zeros of a fresh engine.

Shapes: 2-layer synthetic weights (the per-layer loop runs twice), f32 and bf16, right_context 0 and 13, at the five points of the fork
tests -- fresh, one chunk, mid chunk (a partial 16-byte vector of samples), K/V head in 257 .. 325 (the window wraps), more than 4096 mel
frames pushed (the mel window wraps)."""
import ctypes as C
import re
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi, gguf_io, sharding, synth
from tests.test_gpu_stream_fork import KVC, OPTS, _calls, _control, _cut, _dirty, _end, _engine, _feed, _fork_point, _next_after, _same

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "nemotron-asr.cpp_amd" / "bin"
HEADER_BYTES = 144                   # csrc/nasr_snapshot.h; the fields read below: mirror_bytes at 104, device_bytes at 112, device_sum at 120


@pytest.fixture(scope="module")
def W2():
    return synth.make_weights(n_layers=2)


@pytest.fixture(scope="module")
def trios(W2):
    """dtype -> (engine A that saves, engine B that restores, control engine), same weights, every read-out option on; the tests leave no stream behind"""
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = tuple(_engine(W2, dtype, 4) for _ in range(3))
        return made[dtype]
    yield get
    for engines in made.values():
        for e in engines:
            e.close()


def _sections(blob):
    mirror_bytes, device_bytes, device_sum = struct.unpack_from("<QQQ", blob, 104)
    assert len(blob) == HEADER_BYTES + mirror_bytes + device_bytes
    return mirror_bytes, device_bytes, device_sum


def _device_checksum(payload):
    """csrc/nasr_snapshot.h restated: word w at index i adds fmix32(w ^ i * 0x9E3779B1) to a sum mod 2^64"""
    w = np.frombuffer(payload, "<u4").astype(np.uint64)
    h = (w ^ ((np.arange(w.size, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)))
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return int(h.sum(dtype=np.uint64))          # uint64 addition wraps: mod 2^64


# ---- twin across engines ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 13])
@pytest.mark.parametrize("dtype", [capi.DTYPE_F32, capi.DTYPE_BF16])
@pytest.mark.parametrize("point", ["fresh", "one_chunk", "mid_chunk", "kv_wrap", "mel_wrap"])
def test_twin_across_engines(trios, point, dtype, R):
    """saved on engine A, restored on engine B, both fed the same remaining audio and finalized: source and restored stream equal the control bit for bit"""
    a, b, ctl = trios(dtype)
    n = synth.shift_samples(R)
    sizes = _fork_point(point, R)
    pcm = synth.make_pcm(11 + R, (sum(sizes) + 7777 + n + 5000) / 16000 + 0.4)
    prefix, at = _cut(pcm, sizes)
    suffix, at = _cut(pcm, [7777, n, 5000], at)
    suffix.append(pcm[at:])
    src = a.stream(R)
    twin = None
    try:
        pre = _feed(a, src, prefix)
        p = src.progress()
        if point == "mid_chunk":
            assert p.mel_frames_buffered > 9
        if point == "kv_wrap":
            assert 257 <= p.chunks * (1 + R) <= 325 and p.chunks * (1 + R) < KVC, p.chunks
        if point == "mel_wrap":
            assert p.samples_in // 160 > 4096 + 121
        _dirty(b, R)
        saves0, restores0 = a.counter("stream_saves"), b.counter("stream_restores")
        blob = src.save()
        assert a.counter("stream_saves") == saves0 + 1 and len(blob) <= a.snapshot_bound()
        twin = b.restore(blob)
        assert b.counter("stream_restores") == restores0 + 1
        q, p2 = twin.progress(), src.progress()
        assert (q.samples_in, q.chunks, q.cache_valid_len, q.mel_frames_buffered) == (p.samples_in, p.chunks, p.cache_valid_len, p.mel_frames_buffered)
        assert (p2.samples_in, p2.chunks, p2.cache_valid_len, p2.mel_frames_buffered) == (p.samples_in, p.chunks, p.cache_valid_len, p.mel_frames_buffered)
        got_src = _end(a, src, pre + _feed(a, src, suffix))           # the source was not disturbed by the save
        got_twin = _end(b, twin, pre + _feed(b, twin, suffix))
    finally:
        src.destroy()
        if twin:
            twin.destroy()
    want = _control(ctl, R, prefix + suffix)
    print(f"snapshot twin {point} dtype {dtype} R {R}: {len(blob)} bytes, {len(want['tokens'])} tokens, {len(want['fb'])} frames")
    assert len(want["tokens"]) >= 1
    _same(got_src, want, "source")
    _same(got_twin, want, "restored")


# ---- blob identities, and the kernel's checksum ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,R,point", [(capi.DTYPE_BF16, 13, "mid_chunk"), (capi.DTYPE_F32, 0, "kv_wrap"), (capi.DTYPE_BF16, 0, "mel_wrap")])
def test_blob_identities_and_the_kernel_checksum(trios, dtype, R, point):
    """save(restore(blob)) == blob, save(fork(s)) == save(s), two saves of an untouched stream are equal, the size asked for with buf == NULL is
    the size written and within the bound -- and the checksum the pack launch left in the header (the sum of its workgroups' partials: wave
    reduction, then LDS) equals the host formula over the payload, as does the one the unpack launch compares on the way back"""
    a, b, _ = trios(dtype)
    prefix, _ = _cut(synth.make_pcm(51, sum(_fork_point(point, R)) / 16000 + 0.2), _fork_point(point, R))
    src = a.stream(R)
    made = []
    try:
        _feed(a, src, prefix)
        need = C.c_int64(-1)
        assert capi.lib().nasr_stream_save(src.h, None, 0, C.byref(need)) < 0
        assert f"needs {need.value} bytes".encode() in capi.lib().nasr_last_error()
        small = C.create_string_buffer(need.value - 1)
        need2 = C.c_int64(-1)
        assert capi.lib().nasr_stream_save(src.h, C.cast(small, C.c_void_p), need.value - 1, C.byref(need2)) < 0 and need2.value == need.value
        blob = src.save()
        assert len(blob) == need.value <= a.snapshot_bound() == b.snapshot_bound()
        assert src.save() == blob
        mirror_bytes, device_bytes, device_sum = _sections(blob)
        payload = blob[HEADER_BYTES + mirror_bytes:]
        assert device_bytes % 16 == 0 and device_bytes > 2 * 2 * 70 * 1024 * (2 if dtype == capi.DTYPE_BF16 else 4)
        assert _device_checksum(payload) == device_sum, "k_stream_pack's reduction disagrees with the host formula"
        _dirty(b, R)
        twin = b.restore(blob)                                         # k_stream_unpack's sum equalled the header's, or this would have failed
        made.append(twin)
        assert twin.save() == blob
        _dirty(a, R)
        fork = src.fork()
        made.append(fork)
        assert fork.save() == blob
        again = a.restore(blob)                                        # the engine that saved, another slot
        made.append(again)
        assert again.save() == blob
    finally:
        src.destroy()
        for s in made:
            s.destroy()


# ---- a reset stream against a new one --------------------------------------------------------------------------------------------------
MIRROR_NAMES = ("R", "prompt", "abuf_cnt", "abuf_par", "mel_start", "mel_count", "valid_len", "kv_head", "cc_par", "chunks", "tok_read", "samples_in", "boost_enabled", "lm_enabled",
                "sample_rate", "encoding", "channels", "channel", "aud_in", "aud_out", "aud_par", "n_queue")
MIRROR_FMT = "<11iqII4iqqiI"         # the mirror's fixed fields in wire order (tests/test_snapshot_format.py restates the whole format)
FRESH = dict(abuf_cnt=256, abuf_par=0, mel_start=0, mel_count=9, valid_len=0, kv_head=0, cc_par=0, chunks=0, tok_read=0, samples_in=0, aud_in=0, aud_out=0, aud_par=0, n_queue=0)


def _mirror(blob):
    return dict(zip(MIRROR_NAMES, struct.unpack_from(MIRROR_FMT, blob, HEADER_BYTES)))


def _segments(mirror, esz, n_layers=2, ks=9):
    """(name, bytes in the device section) of the fork plan's segments under OPTS for a mirror whose K/V and mel windows do not wrap (csrc/nasr_fork_plan.h
    and the per-slot buffers of csrc/nasr_decode_set.h restated)"""
    pad = lambda n: -(-n // 16) * 16
    assert mirror["kv_head"] + 70 <= KVC and mirror["mel_start"] + mirror["mel_count"] <= 4096
    segs = []
    for layer in range(n_layers):
        segs += [(f"kv[{layer}].K", 70 * 1024 * esz), (f"kv[{layer}].V", 70 * 1024 * esz), (f"cc[{layer}]", 2 * (ks - 1) * 1024 * 4)]
    segs += [("mel", mirror["mel_count"] * 128 * 4), ("abuf", pad(mirror["abuf_cnt"] * 4)), ("last_sample", 16), ("aud_hist", pad(2 * 193 * 4))]
    segs += [("ctrl", 48), ("h", 4 * 640 * 4), ("c", 4 * 640 * 4), ("predg", 640 * 4), ("tok_ring", 4096 * 4), ("tok_frame", 4096 * 4), ("tok_logprob", 4096 * 4),
             ("alt_id", 4096 * 3 * 4), ("alt_lp", 4096 * 3 * 4), ("frame_blank", 4096 * 4)]
    return [(name, n) for name, n in segs if n]


# what k_stream_reset leaves as it finds it, because the decode writes it before it reads it: the LSTM candidate (DecCtrl::dirty = 1) and the
# read-out rings (clipped to n_tok and frame0 + t, which it zeroes)
NOT_RESET = {"predg", "tok_ring", "tok_frame", "tok_logprob", "alt_id", "alt_lp", "frame_blank"}


def _differing(payload_a, payload_b, mirror, esz):
    """names of the device-section segments in which two payloads of the same plan differ"""
    at, out = 0, []
    for name, n in _segments(mirror, esz):
        if payload_a[at:at + n] != payload_b[at:at + n]:
            out.append(name)
        at += n
    assert at == len(payload_a) == len(payload_b)
    return out


@pytest.mark.parametrize("reference", [False, True])
def test_a_reset_stream_saves_what_a_new_stream_saves(trios, reference):
    """one engine, right_context 0: a stream that has decoded two chunks and more and is reset saves the header and mirror bytes of a stream just
    created with the same right_context and prompt (create and reset go through one function on the record), and every segment of the device
    section that k_stream_reset writes.  The device sections as a whole are NOT equal, before the record existed or since: the segments of
    NOT_RESET hold what the slot's earlier life left (all seven differed on the MI355X), so the device checksum and the head checksum over it
    are left out of the header comparison.
    reset(reference=True): abuf_cnt, abuf_par, kv_head and cc_par in the mirror are those from before the reset, the rest of it is a new
    stream's, and the device section has the size the fork plan gives that mirror"""
    eng, _, _ = trios(capi.DTYPE_BF16)
    R, n = 0, synth.shift_samples(0)
    used, new = eng.stream(R), None
    try:
        eng.step([used], [synth.make_pcm(17, (3 * n + 77) / 16000 + 0.01)[:3 * n + 77]])
        before = _mirror(used.save())
        assert before["chunks"] >= 2 and before["kv_head"] == before["chunks"] and before["samples_in"] == 3 * n + 77 and before["abuf_cnt"] != 256
        used.reset(reference=reference)
        blob_used = used.save()
        new = eng.stream(R)
        blob_new = new.save()
    finally:
        used.destroy()
        if new:
            new.destroy()
    got, fresh = _mirror(blob_used), _mirror(blob_new)
    assert fresh == dict(before, **FRESH) and _sections(blob_new)[0] == 112
    if reference:
        kept = {k: before[k] for k in ("abuf_cnt", "abuf_par", "kv_head", "cc_par")}
        assert got == dict(fresh, **kept), (got, fresh)
        pad = lambda v: -(-v // 16) * 16
        assert _sections(blob_used)[1] == _sections(blob_new)[1] - pad(256 * 4) + pad(kept["abuf_cnt"] * 4)
        return
    head = HEADER_BYTES + 112
    diff = _differing(blob_used[head:], blob_new[head:], fresh, 2)
    print(f"reset against create: device segments that differ: {diff or 'none'}")
    assert got == fresh
    assert blob_used[:120] == blob_new[:120] and blob_used[128:136] == blob_new[128:136] and blob_used[HEADER_BYTES:head] == blob_new[HEADER_BYTES:head]
    assert set(diff) <= NOT_RESET, diff


# ---- carried decoder state ----------------------------------------------------------------------------------------------------------------
def test_boost_and_lm_state_travel(W2):
    """tests/test_gpu_stream_fork.py::test_boost_and_lm_state_travel with a save on one engine and a restore on another that carries the
    same boost set and LM, between the two tokens of the phrase: X follows t1 only in a stream whose automaton stands inside the phrase AND
    whose LM history is t1.  Then: a restore where the boost set or the LM differs is refused with the message that names it"""
    R, n = 0, synth.shift_samples(0)
    opts = OPTS + (("phrase_boost", 64), ("lm_fusion", 1))
    eng, dst, ctl = (_engine(W2, capi.DTYPE_F32, 3, opts) for _ in range(3))
    try:
        c = ctl.stream(R)

        def run(pcm, boost=True, lm=True):
            c.reset()
            c.set_boost(boost)
            c.set_lm(lm)
            return _calls(ctl, c, pcm, n)

        def tables(e, t1, X, g):
            e.set_boost_phrases([[t1, X]], 1e-4)
            e.set_lm({(t1,): (-6.0, 0.0), (X,): (-6.0, 0.0), (t1, X): (-6.0 + 2.0 * (g - 5e-5), 0.0)}, order=2, unk_logprob=-6.0)
            e.set_greedy_lm_weights(0.5, 3.0)
        picked, tried = None, 0
        for seed in (31, 33, 35):
            pcm = synth.make_pcm(seed, 12.0)
            ctl.set_boost_phrases([], None)
            ctl.set_lm(None)
            plain = run(pcm)
            ids, lps = c.token_alternatives()
            cands, idx = [], 0
            for i, call in enumerate(plain[:-2]):
                idx += len(call)
                later = [t for c2 in plain[i + 1:] for t in c2]
                if i < 1 or not call or not later:
                    continue
                for k in (1, 2):
                    X, g = int(ids[idx][k]), float(lps[idx][0]) - float(lps[idx][k])
                    if X not in (1024, call[-1]) and g >= 1e-3:
                        cands.append((i, call[-1], later[0], X, g))
                        break
            for i, t1, t2, X, g in cands:
                tried += 1
                tables(ctl, t1, X, g)
                no_boost, no_lm, both = run(pcm, boost=False), run(pcm, lm=False), run(pcm)
                if (_next_after(both, i) == (t1, X) and _next_after(no_boost, i) == (t1, t2) and _next_after(no_lm, i) == (t1, t2)
                        and both[:i + 1] == plain[:i + 1]):
                    picked = (i, t1, t2, X, g)
                    break
            if picked:
                break
        assert picked, f"none of {tried} call boundaries of the control's output gave a phrase that needs both states"
        i, t1, t2, X, g = picked
        want = _end(ctl, c, [t for call in both for t in call])
        for e in (eng, dst):
            tables(e, t1, X, g)
        src = eng.stream(R)
        calls = [pcm[o:o + n] for o in range(0, pcm.size - n + 1, n)]
        pre = _feed(eng, src, calls[:i + 1])
        assert pre[-1] == t1
        d = dst.stream(R)                                              # the dirty slot: boosted and fused, another history
        _feed(dst, d, [synth.make_pcm(32, 2.0)])
        d.destroy()
        blob = src.save()
        twin = dst.restore(blob)
        got_twin = _end(dst, twin, pre + _feed(dst, twin, calls[i + 1:]))
        got_src = _end(eng, src, pre + _feed(eng, src, calls[i + 1:]))
        assert got_twin["tokens"][len(pre)] == X and got_src["tokens"][len(pre)] == X
        _same(got_src, want, "source")
        _same(got_twin, want, "restored")
        twin.destroy()
        # other tables: the states in the blob mean nothing against them
        dst.set_boost_phrases([[t1, X], [X, t1]], 1e-4)
        with pytest.raises(capi.NasrError, match=r"boost set mismatch: the snapshot's fingerprint is [0-9a-f]{16}, the engine's [0-9a-f]{16}"):
            dst.restore(blob)
        dst.set_boost_phrases([[t1, X]], 1e-4)
        dst.set_greedy_lm_weights(0.25, 3.0)
        with pytest.raises(capi.NasrError, match=r"language model mismatch: the snapshot's fingerprint is [0-9a-f]{16}, the engine's [0-9a-f]{16}"):
            dst.restore(blob)
        dst.set_lm(None)
        with pytest.raises(capi.NasrError, match=r"language model mismatch: .* the engine's 0{16}"):
            dst.restore(blob)
        tables(dst, t1, X, g)                                          # the same ones again: accepted, and still the twin
        twin = dst.restore(blob)
        _same(_end(dst, twin, pre + _feed(dst, twin, calls[i + 1:])), want, "restored after the refusals")
        assert dst.counter("stream_restores") == 2
    finally:
        for e in (eng, dst, ctl):
            e.close()


def test_converter_state_travels(trios):
    """a 44.1 kHz f32 stereo stream (mean of the channels) saved in the middle of a sequence of odd pushes: history, counters and parity of
    the audio converter travel, step_audio on the restored stream equals the control"""
    a, b, ctl = trios(capi.DTYPE_BF16)
    R = 13
    mono = synth.make_pcm(61, 4.0 * 44100 / 16000).astype(np.float32) / 32768.0
    raw = np.stack([mono * 0.75, mono * 1.25], axis=1).astype(np.float32)
    pushes = [raw[o:o + 23333] for o in range(0, raw.shape[0], 23333)]
    assert len(pushes) >= 6
    fmt = lambda s: s.set_audio_format(44100, "f32", 2, "mix")
    src = a.stream(R)
    twin = None
    try:
        fmt(src)
        pre = _feed(a, src, pushes[:3], audio=True)
        _dirty(b, R)
        twin = b.restore(src.save())
        assert (twin.fmt.sample_rate, twin.fmt.encoding, twin.fmt.channels, twin.fmt.channel) == (44100, capi.AUDIO_F32, 2, -1)
        got_twin = _end(b, twin, pre + _feed(b, twin, pushes[3:], audio=True))
        got_src = _end(a, src, pre + _feed(a, src, pushes[3:], audio=True))
    finally:
        src.destroy()
        if twin:
            twin.destroy()
    want = _control(ctl, R, pushes, setup=fmt, audio=True)
    assert len(want["tokens"]) >= 1
    _same(got_src, want, "44.1 kHz stereo: source")
    _same(got_twin, want, "44.1 kHz stereo: restored")


def test_undelivered_tokens_travel(W2, trios):
    """a save behind a NASR_FLAG_NO_SYNC step, before the collect: the tokens are in the source's device ring and in the blob, and the restored
    stream's collect returns what the source's does.  The same behind a pipelined step in flight (the save completes it: the tokens wait in
    the host queue of both)"""
    a, b, ctl = trios(capi.DTYPE_BF16)
    R, n = 13, synth.shift_samples(13)
    pcm = synth.make_pcm(24, 12 * n / 16000 + 0.5)
    pushes = [pcm[o:o + n] for o in range(0, 12 * n, n)] + [pcm[12 * n:]]
    want = _control(ctl, R, pushes)
    c = ctl.stream(R)
    sync2 = _feed(ctl, c, pushes[:2])
    c.destroy()
    assert len(sync2) >= 1
    piped = _engine(W2, capi.DTYPE_BF16, 3)
    piped.set_option("pipeline", 4)
    try:
        for eng, flags in ((a, capi.FLAG_NO_SYNC), (piped, 0)):
            src = eng.stream(R)
            pre = []
            for p in pushes[:2]:
                pre += eng.step([src], [p], flags=flags)[0]
            assert len(pre) < len(sync2), "nothing is outstanding: the step's tokens were delivered"
            _dirty(b, R)
            twin = b.restore(src.save())
            assert b.collect([twin])[0] == eng.collect([src])[0] == sync2[len(pre):]
            got_twin = _end(b, twin, sync2 + _feed(b, twin, pushes[2:]))
            src.destroy()
            twin.destroy()
            assert got_twin["tokens"] == want["tokens"] and got_twin["frames"] == want["frames"]
    finally:
        piped.close()


# ---- graphs, refusals ---------------------------------------------------------------------------------------------------------------------
def test_saves_and_restores_between_graph_steps_keep_the_graphs(trios):
    """ten saves and restores between graph steps: every step is still a graph replay, nothing is evicted or captured anew, the counters count"""
    eng, _, _ = trios(capi.DTYPE_BF16)
    R, n = 0, synth.shift_samples(0)
    pcm = synth.make_pcm(91, 20 * n / 16000)
    st = eng.stream(R)
    try:
        for k in range(6):
            eng.step([st], [pcm[k * n:(k + 1) * n]])
        replays, evictions, shapes, saves, restores = (eng.counter(k) for k in ("graph_replays", "graph_evictions", "graph_shapes", "stream_saves", "stream_restores"))
        for k in range(6, 16):
            t = eng.restore(st.save())
            eng.step([st], [pcm[k * n:(k + 1) * n]])
            assert eng.counter("graph_replays") == replays + (k - 5)
            t.destroy()
        assert eng.counter("graph_evictions") == evictions and eng.counter("graph_shapes") == shapes
        assert eng.counter("stream_saves") == saves + 10 and eng.counter("stream_restores") == restores + 10
    finally:
        st.destroy()


def test_refusals_leave_the_engine_usable(W2, trios):
    a, _, ctl = trios(capi.DTYPE_BF16)
    L = capi.lib()
    R = 0
    pcm = synth.make_pcm(81, 2.5)
    pushes, _ = _cut(pcm, [7777] * 5)
    want = _control(ctl, R, pushes)
    small = _engine(W2, capi.DTYPE_BF16, 2)
    other_dtype = _engine(W2, capi.DTYPE_F32, 2)
    fewer_options = _engine(W2, capi.DTYPE_BF16, 2, OPTS[:2])
    try:
        src = a.stream(R)
        pre = _feed(a, src, pushes[:2])
        blob = src.save()
        mirror_bytes, device_bytes, _ = _sections(blob)
        # one payload bit flipped: every host check passes, the sum k_stream_unpack leaves differs from the header's
        bad = bytearray(blob)
        bad[HEADER_BYTES + mirror_bytes + device_bytes // 3] ^= 0x10
        restores0 = small.counter("stream_restores")
        with pytest.raises(capi.NasrError, match="device section checksum mismatch"):
            small.restore(bytes(bad))
        with pytest.raises(capi.NasrError, match="header / mirror checksum mismatch"):
            small.restore(blob[:HEADER_BYTES + 3] + bytes([blob[HEADER_BYTES + 3] ^ 1]) + blob[HEADER_BYTES + 4:])
        with pytest.raises(capi.NasrError, match="truncated"):
            small.restore(blob[:-1])
        with pytest.raises(capi.NasrError, match="dtype mismatch: the snapshot has 1, the engine 0"):
            other_dtype.restore(blob)
        with pytest.raises(capi.NasrError, match="option frame_blank_logprobs mismatch: the snapshot has 1, the engine 0"):
            fewer_options.restore(blob)
        assert small.counter("stream_restores") == restores0
        s0, s1 = small.stream(R), small.stream(R)                      # both slots are free: the failed restores hold none
        s1.destroy()
        _dirty(small, R)
        twin = small.restore(blob)                                     # the good blob, into the slot the refused one was scattered into
        with pytest.raises(capi.NasrError, match=r"stream pool exhausted \(max_streams=2\)"):
            small.restore(blob)
        out = C.c_void_p(1)
        buf = C.create_string_buffer(blob, len(blob))
        n_out = C.c_int64()
        assert L.nasr_stream_restore(None, C.cast(buf, C.c_void_p), len(blob), C.byref(out)) < 0 and b"null" in L.nasr_last_error()
        assert L.nasr_stream_restore(small.h, None, len(blob), C.byref(out)) < 0 and out.value is None
        assert L.nasr_stream_restore(small.h, C.cast(buf, C.c_void_p), len(blob), None) < 0
        assert L.nasr_stream_save(None, C.cast(buf, C.c_void_p), len(blob), C.byref(n_out)) < 0 and b"null" in L.nasr_last_error()
        assert L.nasr_stream_save(src.h, C.cast(buf, C.c_void_p), len(blob), None) < 0
        assert L.nasr_engine_snapshot_bound(None, C.byref(n_out)) < 0
        dead = C.c_void_p(s0.h.value)                                  # a destroyed stream is refused, not read
        s0.destroy()
        assert L.nasr_stream_save(dead, C.cast(buf, C.c_void_p), len(blob), C.byref(n_out)) < 0 and b"not a live stream" in L.nasr_last_error()
        assert small.counter("stream_restores") == restores0 + 1 and small.counter("stream_saves") == 0
        got_twin = _end(small, twin, pre + _feed(small, twin, pushes[2:]))
        got_src = _end(a, src, pre + _feed(a, src, pushes[2:]))
        src.destroy()
        twin.destroy()
        _same(got_twin, want, "restored after the refused calls")
        _same(got_src, want, "source after the refused calls")
    finally:
        for e in (small, other_dtype, fewer_options):
            e.close()


# ---- migration, and a later process -------------------------------------------------------------------------------------------------------
def test_migrate_between_two_engines(trios):
    a, b, ctl = trios(capi.DTYPE_BF16)
    R = 13
    pcm = synth.make_pcm(71, 6.0)
    pushes, _ = _cut(pcm, [7777] * 12)
    src = a.stream(R)
    pre = _feed(a, src, pushes[:5])
    blockers = [b.stream(R) for _ in range(4)]                          # b is full: the migration fails and the source survives
    with pytest.raises(capi.NasrError, match="stream pool exhausted"):
        sharding.migrate(src, b)
    assert src.h is not None and src.progress().samples_in == 5 * 7777
    for s in blockers:
        s.destroy()
    _dirty(b, R)
    moved = sharding.migrate(src, b)
    assert src.h is None and moved.engine is b
    full = [a.stream(R) for _ in range(4)]                             # the source engine's slot is free again: all four can be taken
    for s in full:
        s.destroy()
    got = _end(b, moved, pre + _feed(b, moved, pushes[5:]))
    moved.destroy()
    _same(got, _control(ctl, R, pushes), "migrated")


def test_cli_two_runs_over_the_halves_of_a_file(W2, tmp_path):
    """nemotron-asr-amd --save-state over the first half (cut at a multiple of the read size), then a fresh process with --load-state over the
    second half: by the rule of the usage text -- first line of run 1 without its newline + first line of run 2 = first line of the whole run, the
    later lines of run 2 are the whole run's -- the two runs print what one run over the whole file prints"""
    gguf_io.write_gguf(tmp_path / "model.gguf", W2, gguf_io.default_hparams(n_layers=2), gguf_io.synthetic_vocab())
    pcm = synth.make_pcm(11, 16.0)
    read = (9 + 8) * 160                                               # samples per read at right_context 0 (the synthetic model goes on emitting there; at 13 it says all it has in its first chunks)
    pcm.tofile(tmp_path / "whole.pcm")

    def run(audio, *flags):
        r = subprocess.run([str(BIN / "nemotron-asr-amd"), str(tmp_path / "model.gguf"), str(tmp_path / audio), "80", "0", "--print-tokens", "--timestamps", *flags],
                           capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr[-800:]
        return r.stdout.split(b"\n")
    whole = run("whole.pcm")
    # the cut: the read boundary at the median word time of the whole run (its --timestamps line), so that both runs have something to say
    times = sorted(float(t) for t in re.findall(rb"\{([0-9.]+)\}", whole[1]))
    assert len(times) >= 4 and times[-1] > times[0], whole[1]
    cut = max(1, int(times[len(times) // 2] / 0.08)) * read
    pcm[:cut].tofile(tmp_path / "first.pcm")
    pcm[cut:].tofile(tmp_path / "second.pcm")
    first = run("first.pcm", "--save-state", str(tmp_path / "state.bin"))
    second = run("second.pcm", "--load-state", str(tmp_path / "state.bin"))
    assert (tmp_path / "state.bin").stat().st_size > 2 * 2 * 70 * 1024 * 2
    assert len(whole[-2].split()) > 3 and whole[-2].startswith(b"TOKENS:")
    assert first[0] + second[0] == whole[0]
    assert second[1:] == whole[1:]
    assert len(first[0]) > 0 and len(second[0]) > 0
