"""csrc/nasr_resample.h (the arithmetic of the device-side audio input conversion) and host/wav_header.h, compiled with g++ under
AddressSanitizer / UBSan without FMA contraction -- no GPU -- against tests/resample_ref.py, a float64 numpy reference written from the
formulae of the design:
(1) the coefficient table of all eight rates; L, M, half and the tap counts are pinned
(2) the frequency response of the float64 prototype: +-0.1 dB up to 0.87 of the lower Nyquist, <= -80 dB from 1.03 of it
(3) the converter's s16 output against the float64 sum: off by at most 1, and only where the exact value is within the rounding allowance
    of the sequential f32 sum of a half-integer
(4) out_ready / out_total against brute force, and their linearity in steady state
(5) the G.711 tables, all 256 codes                (6) any cut into pushes gives the one-shot output bit for bit
(7) the WAV header parser over damaged headers: never out of bounds, accepted / rejected as stated."""
import struct
from pathlib import Path

import numpy as np
import pytest

from tests import resample_ref as rr

ROOT = Path(__file__).resolve().parent.parent
PINNED = {8000: (2, 1, 64, 65), 11025: (640, 441, 20480, 65), 16000: (1, 1, 0, 1), 22050: (320, 441, 14112, 89),
          24000: (2, 3, 96, 97), 32000: (1, 2, 64, 129), 44100: (160, 441, 14112, 177), 48000: (1, 3, 96, 193)}      # L, M, half, taps


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    d = tmp_path_factory.mktemp("resample")
    return rr.build_driver(d, ROOT), d


@pytest.mark.parametrize("fin", rr.RATES)
def test_coefficient_table(drv, fin):
    prog, _ = drv
    lines = rr.run_driver(prog, "table", fin).split("\n")
    head = lines[0].split()
    L, M, half, hist, max_taps, max_span = (int(v) for v in head[:6])
    assert (int(head[6]), float(head[7]), float(head[8])) == (rr.Z, rr.BETA, rr.RHO)         # the header's design constants are the reference's
    assert (L, M, half, max_taps) == PINNED[fin] and (L, M, half) == rr.plan(fin)
    assert hist == 2 * half // L + 1 == max_taps and hist <= 193 and max_span <= 1024        # what the kernel's buffers are sized for
    got = np.array([float(v) for v in lines[1:] if v]).astype(np.float32).astype(np.float64)       # nine digits name an f32 exactly
    ref = rr.coefficients(fin)
    assert got.shape == ref.shape == (2 * half + 1,)
    assert np.all(np.abs(got - ref) <= np.maximum(2.0 ** -23 * np.abs(ref), 1e-9))
    if fin == 16000:
        assert got.tolist() == [1.0]


@pytest.mark.parametrize("fin", [r for r in rr.RATES if r != 16000])
def test_frequency_response_of_the_prototype(fin):
    L, M, half = rr.plan(fin)
    c = rr.coefficients(fin)
    fs = float(fin) * L                                        # the prototype's own sampling rate
    nfft = 1 << 21
    H = np.abs(np.fft.rfft(c, nfft)) / L
    f = np.arange(H.size) * fs / nfft
    db = 20 * np.log10(np.maximum(H, 1e-30))
    ny = min(fin, 16000) / 2
    assert np.all(np.abs(db[f <= 0.87 * ny]) <= 0.1), float(np.abs(db[f <= 0.87 * ny]).max())
    assert np.all(db[f >= 1.03 * ny] <= -80.0), float(db[f >= 1.03 * ny].max())


CASES = [(fin, "s16", 1, 0, kind) for fin in rr.RATES if fin != 16000 for kind in ("noise", "chirp", "square")] + [
    (44100, "f32", 2, -1, "noise"), (8000, "mulaw", 1, 0, "noise"), (8000, "alaw", 2, 1, "noise"), (48000, "f32", 3, -1, "square"),
    (16000, "f32", 1, 0, "square"), (16000, "mulaw", 2, -1, "noise")]


@pytest.mark.parametrize("fin,enc,channels,channel,kind", CASES)
def test_driver_against_the_float64_sum(drv, fin, enc, channels, channel, kind):
    prog, d = drv
    rng = np.random.default_rng(7)
    # the f32 sum's rounding error grows with the partial sums, which are largest around the edges of a full-scale square wave: there a
    # few per cent of the samples round the other way.  The square wave is long and has two edges, so that its share stays under the bound
    raw = rr.make_input(rng, enc, 4000 if kind == "square" else 1500, channels, kind, fin)
    got = rr.convert(prog, d, raw, fin, enc, channels, channel).astype(np.int64)
    y, mag, taps = rr.resample(rr.decode(raw, enc, channels, channel), fin)
    assert got.shape == y.shape
    ref = np.clip(np.rint(y), -32768, 32767).astype(np.int64)
    diff = got - ref
    assert np.abs(diff).max() <= 1
    # the sequential f32 sum of ntaps products is within ntaps * 2^-24 * sum |c| |x| of the exact one: only an exact value that close to a
    # half-integer may round the other way
    allow = taps * 2.0 ** -24 * mag
    to_half = np.abs(np.abs(y - np.floor(y)) - 0.5)
    used = diff != 0
    assert np.all(to_half[used] <= allow[used])
    print(f"{fin} {enc} {kind}: {used.sum()} of {used.size} samples round the other way ({100 * used.mean():.2f} %)")
    assert used.mean() <= 0.01, used.mean()
    if kind == "square" and fin != 16000:
        assert (got == 32767).any() and (got == -32768).any()                  # the overshoot saturates


@pytest.mark.parametrize("fin", rr.RATES)
def test_counts(drv, fin):
    prog, _ = drv
    ns = list(range(0, 2001))
    rows = [tuple(int(v) for v in ln.split()) for ln in rr.run_driver(prog, "counts", fin, *ns).strip().split("\n")]
    assert rows == [(rr.out_ready_brute(fin, n), rr.out_total_brute(fin, n)) for n in ns]
    assert rows == [(rr.out_ready(fin, n), rr.out_total(fin, n)) for n in ns]
    if fin == 16000:
        assert [r[0] for r in rows] == ns
    L, M, half = rr.plan(fin)
    for c in (1280, 17920):                                    # chunk sizes are multiples of 160, so c M / L input frames are whole
        assert (c * M) % L == 0
        step = c * M // L
        for n0 in (half // L + 2, 3000, 3001, 77777):
            pts = [n0 + step * k for k in range(6)]
            r = [int(ln.split()[0]) for ln in rr.run_driver(prog, "counts", fin, *pts).strip().split("\n")]
            assert [b - a for a, b in zip(r, r[1:])] == [c] * 5
    # whole-chunk pushes from the start: every push from the second on completes exactly one chunk's samples
    for c in (1280, 17920):
        step = c * M // L
        r = [int(ln.split()[0]) for ln in rr.run_driver(prog, "counts", fin, *[step * k for k in range(1, 6)]).strip().split("\n")]
        assert [b - a for a, b in zip(r, r[1:])] == [c] * 4


def test_g711_tables(drv):
    prog, _ = drv
    v = np.array([int(x) for x in rr.run_driver(prog, "g711").split()])
    assert v.shape == (512,)
    assert np.array_equal(v[:256], rr.mulaw_table()) and np.array_equal(v[256:], rr.alaw_table())
    assert v[:256].max() == 32124 and v[:256].min() == -32124 and v[256:].max() == 32256 and v[256:].min() == -32256
    try:
        import audioop
    except ImportError:
        return
    codes = bytes(range(256))
    assert np.array_equal(v[:256], np.frombuffer(audioop.ulaw2lin(codes, 2), dtype="<i2"))
    assert np.array_equal(v[256:], np.frombuffer(audioop.alaw2lin(codes, 2), dtype="<i2"))


@pytest.mark.parametrize("fin,enc,channels,channel", [(8000, "mulaw", 1, 0), (44100, "f32", 2, -1), (48000, "s16", 1, 0), (22050, "s16", 2, 1),
                                                      (11025, "alaw", 1, 0), (24000, "f32", 1, 0), (32000, "s16", 3, -1), (16000, "s16", 2, -1)])
def test_any_cut_into_pushes_gives_the_one_shot_output(drv, fin, enc, channels, channel):
    prog, d = drv
    rng = np.random.default_rng(fin + channels)
    frames = 2500
    raw = rr.make_input(rng, enc, frames, channels, "noise", fin)
    whole = rr.convert(prog, d, raw, fin, enc, channels, channel, tag="whole")
    assert whole.size == rr.out_total(fin, frames)
    L, _, half = rr.plan(fin)
    hist = 2 * half // L + 1
    for trial in range(4):
        pushes, left = [], frames
        while left > 0 and len(pushes) < 60:
            n = int(rng.choice([0, 1, 1, 2, hist - 1, hist, hist + 1, int(rng.integers(1, 3 * hist + 2)), int(rng.integers(1, 700))]))
            n = min(max(n, 0), left)
            pushes.append(n)
            left -= n
        if trial == 3:
            pushes = [1] * 300                                               # one frame at a time through the whole history span
        got = rr.convert(prog, d, raw, fin, enc, channels, channel, pushes=pushes, tag=f"p{trial}")
        assert np.array_equal(got, whole), (trial, pushes[:10])


def _wav(fmt_tag=1, channels=1, rate=16000, bits=16, extra=b"", data=b"\0" * 32, data_size=None, fmt_body=None, with_data=True):
    if fmt_body is None:
        fmt_body = struct.pack("<HHIIHH", fmt_tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt_body)) + fmt_body + (b"\0" if len(fmt_body) & 1 else b"") + extra
    if with_data:
        body += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


def test_wav_header_corpus(drv):
    prog, d = drv
    OK, NOT_WAV = 0, 1
    good = _wav()
    ext = struct.pack("<HHIIHH", 0xFFFE, 2, 48000, 48000 * 8, 8, 32) + struct.pack("<HHI", 22, 32, 3) + struct.pack("<H", 3) + b"\0" * 14
    odd_list = b"LIST" + struct.pack("<I", 5) + b"abcde" + b"\0"
    corpus = [
        (good, OK, dict(tag=1, ch=1, rate=16000, enc=0, off=44)),
        (_wav(3, 2, 44100, 32), OK, dict(tag=3, ch=2, rate=44100, enc=1, off=44)),
        (_wav(7, 1, 8000, 8), OK, dict(tag=7, ch=1, rate=8000, enc=2, off=44)),
        (_wav(6, 1, 8000, 8), OK, dict(tag=6, ch=1, rate=8000, enc=3, off=44)),
        (_wav(fmt_body=ext), OK, dict(tag=3, ch=2, rate=48000, enc=1, off=68)),
        (_wav(extra=odd_list), OK, dict(off=44 + 14)),                                              # odd chunk, padded
        (_wav(extra=b"LIST" + struct.pack("<I", 5) + b"abcde"), "err", {}),                        # odd chunk WITHOUT its pad byte: 'data' is not where a chunk starts
        (_wav(data_size=0xFFFFFFFF), OK, dict(off=44, bytes=0xFFFFFFFF)),                           # a writer that could not seek back
        (_wav(data=b"", data_size=1 << 31), OK, dict(off=44)),                                      # data "larger" than the file
        (_wav(extra=b"junk" + struct.pack("<I", 0xFFFFFFF0) + b"xx"), "err", {}),                  # huge chunk in front of data
        (_wav(extra=b"junk" + struct.pack("<I", 0xFFFFFFFF)), "err", {}),
        (_wav(with_data=False), "err", {}),                                                         # no data chunk
        (b"RIFF" + struct.pack("<I", 4) + b"WAVE", "err", {}),                                      # no chunks at all
        (b"RIFF" + struct.pack("<I", 20) + b"WAVE" + b"data" + struct.pack("<I", 8) + b"\0" * 8, "err", {}),      # data before fmt
        (_wav(2, 1, 16000, 4), "err", {"msg": "format tag 2"}),                                    # ADPCM
        (_wav(1, 1, 16000, 24), "err", {"msg": "format tag 1"}),                                   # 24-bit PCM
        (_wav(0x55, 2, 44100, 0), "err", {"msg": "format tag 85"}),                                # MP3 in a WAVE container
        (_wav(1, 0, 16000, 16), "err", {}), (_wav(1, 9, 16000, 16), "err", {}),                    # channel counts
        (_wav(fmt_body=struct.pack("<HHIIH", 1, 1, 16000, 32000, 2)), "err", {}),                  # fmt chunk of 14 bytes
        (_wav(fmt_body=ext[:30]), "err", {}),                                                       # extensible cut short
        (b"", NOT_WAV, {}), (b"RIFF", NOT_WAV, {}), (b"\0" * 64, NOT_WAV, {}), (b"RIFX" + good[4:], NOT_WAV, {}), (good[:8] + b"AVI " + good[12:], NOT_WAV, {}),
    ]
    for n in range(len(good)):                                                                      # every truncation of a good header
        corpus.append((good[:n], NOT_WAV if n < 12 else ("err" if n < 44 else OK), {}))
    for n in range(12, 68):
        corpus.append((_wav(fmt_body=ext)[:n], "err", {}))
    rng = np.random.default_rng(5)
    fuzz = []
    for _ in range(400):                                                                            # random damage: any verdict, never out of bounds
        b = bytearray(_wav(fmt_body=ext, extra=odd_list) if rng.integers(2) else good)
        for _ in range(int(rng.integers(1, 5))):
            b[int(rng.integers(len(b)))] = int(rng.integers(256))
        fuzz.append(bytes(b[:int(rng.integers(len(b) + 1))]))
    path = d / "wav.bin"
    with open(path, "wb") as f:
        for rec in [c[0] for c in corpus] + fuzz:
            f.write(struct.pack("<I", len(rec)) + rec)
    lines = rr.run_driver(prog, "wav", path).strip("\n").split("\n")
    assert len(lines) == len(corpus) + len(fuzz)
    for (rec, want, facts), ln in zip(corpus, lines):
        head, msg = ln.split("|", 1)
        rc, tag, ch, rate, bits, enc, off, nbytes = (int(v) for v in head.split())
        if want == "err":
            assert rc < 0 and msg, (rec[:64], ln)
        else:
            assert rc == want, (rec[:64], ln)
        if rc == 0:
            assert 0 < off <= len(rec)
        got = dict(tag=tag, ch=ch, rate=rate, enc=enc, off=off, bytes=nbytes)
        for k, v in facts.items():
            if k == "msg":
                assert v in msg, ln
            else:
                assert got[k] == v, (k, ln)
    for rec, ln in zip(fuzz, lines[len(corpus):]):
        rc, off = int(ln.split()[0]), int(ln.split("|")[0].split()[6])
        assert rc in (0, 1, -1, -2, -3, -4) and (rc != 0 or off <= len(rec))
