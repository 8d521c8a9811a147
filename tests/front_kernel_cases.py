"""The cases of tests/test_gpu_front_kernels.py, numpy only (no GPU, no library): operands, the float32 restatements' expectations, the float64 references and
the bounds.  tests/test_front_kernel_ref.py checks them without a GPU: every restatement lies inside its bound, and every listed wrong variant leaves the bound or
breaks the `==`.

Exact    a float32 restatement of the kernel's documented order (tests/front_ref.py), compared with `==`.  The log-mel kernels are exact up to the sum s; the
         output is then compared with log_f64(float32(s + 2^-24)) within LOGF_REL |log|, the one measured constant (the device's logf against float64 on the
         harness's own k_libm, 4 x the largest relative error seen: profiles/front_kernels.md).  sqrtf and the division are IEEE operations in this build.
Bounded  the float64 reference of the operation, |got - ref| <= bound, the bound assembled from unit-roundoff terms: front_ref.mel_bound, front_ref.featnorm_bound,
         and for the convolutions the construction of tests/offline_kernel_cases.py (10 u sum |w x| through both stages)."""
from __future__ import annotations

import zlib

import numpy as np

from nemotron_asr_amd import synth
from tests import front_ref as R
from tests import offline_kernel_cases as OK
from tests import offline_kernel_ref as OR
from tests.front_ref import ABUF_CAP, F32, HOP, MEL_RING, NFFT, NMEL, SUBC, U24

SENT = 0xFFC5
SENT_F32 = np.array([SENT, SENT], np.uint16).view(np.float32)[0]
LOUD = F32(64.0)
LOGF_MEASURED = 1.84e-7         # largest |logf(x) - log(x)| / |log(x)| of the device over 200 001 points (profiles/front_kernels.md)
LOGF_REL = 4 * LOGF_MEASURED


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def sent_f32(shape):
    return np.full(shape, SENT_F32, np.float32)


def stale(n_rows, cols):
    """rows alternating loud / sentinel, loud first"""
    a = sent_f32((n_rows, cols))
    a[0::2] = LOUD
    return a


# ==== streaming log-mel ================================================================================================================================
def stream_tables(zero_row=None):
    fb = synth.mel_filterbank().astype(F32)
    if zero_row is not None:
        fb = fb.copy()
        fb[zero_row] = 0
    cos_t, sin_t = R.twiddles()
    return (R.padded_window(synth.hann_window()), np.ascontiguousarray(fb.T), R.bands(fb), cos_t, sin_t), fb


def pcm_signal(key, n):
    """noise plus tones, full scale at both ends of the s16 range: no mel sum is dominated by cancellation"""
    rng = rng_of("pcm", key)
    t = np.arange(n)
    x = 6000 * rng.standard_normal(n) + 5000 * np.sin(2 * np.pi * 440 / 16000 * t) + 3000 * np.sin(2 * np.pi * 3100 / 16000 * t + 1) + 2000 * np.sin(2 * np.pi * 7100 / 16000 * t)
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    x[3], x[n - 2], x[n // 2] = -32768, 32767, -32768
    return x


MEL_SLOTS, MEL_POOL, MEL_PUSHES = (2, 0, 3), 4, (1000, 2049)
MEL_START = {2: dict(last=0.0, wpos=MEL_RING - 2), 3: dict(last=0.25, wpos=100)}          # slot 0's descriptor is empty (n = 0, n_frames = 0), slot 1 is not named
MEL_VARIANTS = {"exact-max_n": dict(upper=False, tap_cap=0, zero_row=None), "graph-upper-bound-tap": dict(upper=True, tap_cap=3, zero_row=None),
                "empty-filter": dict(upper=False, tap_cap=0, zero_row=5)}
GRAPH_MAX_FRAMES = 16


def stream_reference(pcm, last, n_frames, tables, fb, coeff=R.PRE):
    """float64 log-mel of the first n_frames frames of a stream that starts with 256 zero samples in its buffer -> (ref [F][128], bound [F][128] without logf's term,
    as a function of logf_rel)"""
    window = tables[0]
    x = pcm.astype(np.float64) / 32768.0
    xp = np.concatenate([[float(F32(last))], x[:-1]])
    y = x - float(coeff) * xp
    buf, xa, xpa = (np.concatenate([np.zeros(256), a]) for a in (y, np.abs(x), np.abs(xp)))
    fr = lambda a: np.stack([a[t * HOP:t * HOP + NFFT] for t in range(n_frames)])  # noqa: E731
    v64 = fr(buf) * window.astype(np.float64)[None, :]
    ref, X = R.mel_f64(v64, fb)
    return ref, (lambda logf_rel: R.mel_bound(v64, R.stream_dv(fr(xa), fr(xpa), window), X, fb, tables[2], logf_rel))


def mel_case(variant, pushes=MEL_PUSHES, **wrong):
    """-> dict: tables, per push the descriptor rows and pcm, the expected images of abuf / last_sample after each push, s per push and slot, the float64 reference"""
    v = MEL_VARIANTS[variant]
    tables, fb = stream_tables(v["zero_row"])
    states = {s: R.StreamState(last=MEL_START[s]["last"], wpos=MEL_START[s]["wpos"]) for s in MEL_START}
    pcm_all = {s: pcm_signal((variant, s), sum(pushes)) for s in MEL_START}
    abuf, last = sent_f32((MEL_POOL, 2, ABUF_CAP)), sent_f32(MEL_POOL)
    for s in MEL_START:
        abuf[s, 0, :256], last[s] = 0, MEL_START[s]["last"]
    abuf[0, 0, :256], last[0] = 0, 0.5                                       # the empty descriptor's slot: as after a reset, must stay as it is
    out = dict(tables=tables, fb=fb, abuf0=abuf.copy(), last0=last.copy(), pushes=[], pcm_all=pcm_all)
    done = 0
    for n in pushes:
        descs, pcm, s_of = [], [], {}
        for slot in MEL_SLOTS:
            if slot not in states:
                descs.append([0, slot, 0, 256, 0, 0, 7, 0])
                continue
            st = states[slot]
            x = pcm_all[slot][done:done + n]
            d, s = st.push(x, tables, **wrong)
            descs.append([sum(len(p) for p in pcm), slot, d["n"], d["cnt"], d["par"], d["n_frames"], d["mel_wpos"], d["consumed"]])
            pcm.append(x)
            s_of[slot] = s
            abuf[slot, d["par"], d["cnt"]:d["cnt"] + n] = st.abuf[d["par"], d["cnt"]:d["cnt"] + n]
            if d["n_frames"]:
                left = d["cnt"] + n - d["consumed"]
                abuf[slot, d["par"] ^ 1, :left] = st.abuf[d["par"] ^ 1, :left]
            last[slot] = st.last
        nf = max(d[5] for d in descs)
        max_frames = GRAPH_MAX_FRAMES if v["upper"] else nf
        max_n = max_frames * HOP + NFFT if v["upper"] else max(d[2] for d in descs)
        out["pushes"].append(dict(desc=np.array(descs, np.int32), pcm=np.concatenate(pcm), s=s_of, abuf=abuf.copy(), last=last.copy(), max_frames=max_frames, max_n=max_n,
                                  tap_cap=v["tap_cap"]))
        done += n
    return out


def mel_case_reference(case):
    """slot -> (ref [F][128] over the frames of all pushes, bound(logf_rel))"""
    return {s: stream_reference(case["pcm_all"][s], MEL_START[s]["last"], sum(len(p["s"][s]) for p in case["pushes"]), case["tables"], case["fb"]) for s in MEL_START}


def logf_expect(s):
    """-> (float64 log of the float32 argument, its LOGF bound)"""
    want = np.log(R.log_arg_f32(s).astype(np.float64))
    return want, LOGF_REL * np.abs(want)


# ==== k_mel_put / k_mel_zero ===============================================================================================================================
def mel_ring_case():
    """B = 2 on a pool of 3: slot 2 writes 3 of max_frames = 4 frames across the ring's end, slot 0 writes 4 in the middle -> (desc [B][3], staged, expected mask)"""
    desc = np.array([[2, 3, MEL_RING - 2], [0, 4, 1000]], np.int32)
    staged = rng_of("mel_put").standard_normal((2, 4, NMEL)).astype(F32)
    return desc, staged, 4, 3


# ==== k_sub_conv0_dw =======================================================================================================================================
CONV0_COMBOS = ((0, 100), (1, 0), (2, MEL_RING - 25), (0, MEL_RING - 3), (1, 500), (2, 2000), (0, 200), (1, 1000))          # (slot, mel_start); one wraps 3 frames before the end
CONV0_B = {0: (12, 13, 102, 103), 1: (9, 10, 73, 74), "even": (12, 13, 102, 103)}          # H2 = 5 / 7 / 5: H2 B = 60, 65, 510, 515 / 63, 70, 511, 518
CONV0_EVEN = 16
# "even": the encoder's chunks hold 9 + 8 (1 + R) = 8 k + 1 mel rows, and then the last output row's patch ends on mel row 8 k, the chunk's last: the
# `ih < chunk_mel` mask of the staging never decides anything.  With 16 rows (H1 = 9, H2 = 5 by the same rule) output row 4 reaches mel row 16, the conv's one
# row of padding behind the image, where the ring holds the loud row that follows the chunk.


def conv0_dims(Rc):
    chunk_mel = CONV0_EVEN if Rc == "even" else R.PRE_CACHE + 8 * (1 + Rc)
    H1 = chunk_mel // 2 + 1
    return chunk_mel, H1, H1 // 2 + 1


def conv0_fz(H2, B):
    return 11 if H2 * B <= 64 else (3 if H2 * B <= 512 else 1)


class _Chunk:
    """adapter: tests/offline_kernel_cases.SubSetup.reference on one chunk"""

    def __init__(self, mel, w):
        self.mel, (self.w0, self.b0, self.w2, self.b2) = mel, w

    def utterance(self, k):
        return self.mel

    wt = OK.SubSetup.wt


def conv0_case(Rc):
    """-> ring [3][4096][128] (sentinel but the chunks and their loud / sentinel neighbours), weights, per combo the chunk as the kernel sees it"""
    chunk_mel, H1, H2 = conv0_dims(Rc)
    rng = rng_of("front-conv0", Rc)
    ring = sent_f32((3, MEL_RING, NMEL))
    chunks = []
    for slot, ms in CONV0_COMBOS:
        mel = (2.0 * rng.standard_normal((chunk_mel, NMEL))).astype(F32)
        rows = (ms + np.arange(-2, chunk_mel + 2)) % MEL_RING
        ring[slot, rows[:2]] = stale(2, NMEL)[::-1]
        ring[slot, rows[-2:]] = stale(2, NMEL)
        ring[slot, rows[2:-2]] = mel
        chunks.append(mel)
    w = ((rng.standard_normal((SUBC, 3, 3)) / 3).astype(F32), (0.3 * rng.standard_normal(SUBC)).astype(F32),
         (rng.standard_normal((SUBC, 3, 3)) / 3).astype(F32), (0.3 * rng.standard_normal(SUBC)).astype(F32))
    return dict(ring=ring, w=w, chunks=chunks, chunk_mel=chunk_mel, H1=H1, H2=H2)


def conv0_expect(case, k):
    """combo k -> (float32 restatement [H2][33][256], float64 reference, bound before the output's type)"""
    c = _Chunk(case["chunks"][k], case["w"])
    f32 = OK.conv_front_f32(c.mel, c.wt(c.w0), c.b0, c.wt(c.w2), c.b2)
    ref, bound = OK.SubSetup.reference(c, k)
    return f32, ref, bound


# ==== k_sub_dw / k_sub_dw_row ==============================================================================================================================
DW_WIN = 33
DW_CASES = {5: (170, 171), 14: (63, 64)}          # Hin -> (B with Hout B <= 511, B with Hout B >= 512): 510 / 513 and 504 / 512


def dw_kernel(Hin, B, bf16):
    return f"{'k_sub_dw_row' if (Hin // 2 + 1) * B >= 512 else 'k_sub_dw'}<{'true' if bf16 else 'false'}>"


def dw_case(Hin):
    """-> x [B_large][Hin][33][256] (odd batch entries loud), wt [9][256], bias; w as [256][3][3] for the float64 reference"""
    B = DW_CASES[Hin][1]
    rng = rng_of("front-dw", Hin)
    x = rng.standard_normal((B, Hin, DW_WIN, SUBC)).astype(F32)
    x[1::2] = LOUD * rng.choice([-1.0, 1.0], x[1::2].shape).astype(F32)
    w = (rng.standard_normal((SUBC, 3, 3)) / 3).astype(F32)
    bias = (0.3 * rng.standard_normal(SUBC)).astype(F32)
    return x, np.ascontiguousarray(w.reshape(SUBC, 9).T), bias, w


def dw_reference(x, w, bias, entries):
    """float64 conv3x3_s2 and 10 u (sum |w x| + |bias|) for the batch entries named"""
    zero = np.zeros(SUBC)
    ref = np.stack([OR.conv3x3_s2(x[b], w, bias, True) for b in entries])
    bound = np.stack([OK.G10 * (OR.conv3x3_s2(np.abs(x[b]), np.abs(w), zero, True) + np.abs(bias.astype(np.float64))) for b in entries])
    return ref, bound


# ==== diarization mel ======================================================================================================================================
DIAR_SHAPES = {"vad": dict(n_win=10080, T_pad=64, t_valid=63, cpitch=80), "spk": dict(n_win=24000, T_pad=160, t_valid=150, cpitch=96)}
DIAR_W = 3
DIAR_BASE = 48          # the first window's offset into the audio buffer


def diar_tables(shape):
    fb = (synth.mel_filterbank_n(80) if shape == "vad" else synth.slaney_filterbank(80)).astype(F32)
    cos_t, sin_t = R.twiddles()
    return (R.padded_window(synth.hann_window()), np.ascontiguousarray(fb.T), R.bands(fb), cos_t, sin_t), fb


def diar_audio(shape, s16):
    n = DIAR_BASE + DIAR_SHAPES[shape]["n_win"] + HOP * (DIAR_W - 1) + 32
    x = pcm_signal(("diar", shape, s16), n)
    return x if s16 else (x.astype(F32) / F32(32768.0) * F32(0.9)).astype(F32)


def diar_offsets():
    return DIAR_BASE + HOP * np.arange(DIAR_W, dtype=np.int64)


def diar_reference(x, n_win, ts, tables, fb, s16):
    """float64 log-mel of the frames ts of the window x[:n_win] -> (ref [len][80], bound(logf_rel))"""
    window = tables[0]
    parts = [R.diar_windowed(x, n_win, t, window, s16, f64=True) for t in ts]
    v64 = np.stack([p[0] for p in parts])
    xa, xpa = np.stack([p[1][0] for p in parts]).astype(np.float64), np.stack([p[1][1] for p in parts]).astype(np.float64)
    ref, X = R.mel_f64(v64, fb)
    return ref, (lambda logf_rel: R.mel_bound(v64, R.stream_dv(xa, xpa, window), X, fb, tables[2], logf_rel))


def diar_interior(n_win, t_valid):
    """the frames whose 512 samples, and the sample in front of them, lie inside the window: neither the zero padding nor the restart of the pre-emphasis shows"""
    return [t for t in range(t_valid) if t * HOP - NFFT // 2 >= 1 and t * HOP + NFFT // 2 <= n_win]


DIAR_FRAME_T = (0, 1, 30, 62)          # t = 0, t = 1, an interior t, the last valid t of the VAD shape


# ==== stream state: fork, pack, unpack =====================================================================================================================
VEC_PIECES = (1, 255, 256, 1023, 1024, 1025, 2051)          # 16-byte vectors
WORD_PIECES = ((4, 4, 0), (12, 0, 4), (20, 0, 0), (1028, 8, 12))          # (bytes, src misalignment, dst misalignment); (20, 0, 0): aligned, bytes % 16 != 0


def piece_plan():
    """-> (pieces [n][4] = src offset, dst offset, bytes, pad = dst offset / 4; src bytes; dst bytes): every piece 64 bytes of slack apart in both buffers, in another
    order in the destination"""
    sizes = [(16 * v, 0, 0) for v in VEC_PIECES] + list(WORD_PIECES)
    order = rng_of("pieces").permutation(len(sizes))
    so, src_at = 64, {}
    for i, (b, ms, _) in enumerate(sizes):
        src_at[i] = so + ms
        so += (b + ms + 15) // 16 * 16 + 64
    do, pieces = 64, [None] * len(sizes)
    for i in order:
        b, _, md = sizes[i]
        pieces[i] = (src_at[i], do + md, b, (do + md) // 4)
        do += (b + md + 15) // 16 * 16 + 16 + 64
    return np.array(pieces, np.int64), so, do


def piece_is_words(p):
    return bool((p[0] | p[1] | p[2]) & 15)


def pieces_expect(pieces, src, dst_bytes, which):
    """which 0 fork, 1 pack, 2 unpack: -> (expected dst image as uint8, sentinel elsewhere; sums)"""
    dst = np.full(dst_bytes // 2, SENT, np.uint16).view(np.uint8).copy()
    sums = []
    for so, do, b, pad in pieces:
        data = src[so:so + b]
        dst[do:do + b] = data
        padded = (b + 15) // 16 * 16 if piece_is_words((so, do, b)) else b
        tail = np.zeros(padded - b, np.uint8) if which != 2 else src[so + b:so + padded]
        if which == 1:
            dst[do + b:do + padded] = 0
        sums.append(R.checksum(np.concatenate([data, tail]).view(np.uint32), pad))
    return dst, sums


# ==== k_stream_reset =======================================================================================================================================
RESET = dict(n_layers=2, n_slots=3, slot=1, kv_head=R.KVC - 10, cc_slot_floats=2 * 8 * R.D)
RESET_CASES = [dict(esz=2, keep=0, aud=True, boost=True, lm=(0, 0, 1)), dict(esz=4, keep=1, aud=False, boost=False, lm=None), dict(esz=4, keep=0, aud=True, boost=False, lm=(0, 0, 0)),
               dict(esz=2, keep=1, aud=False, boost=True, lm=(1, 77, 1))]          # lm: (attached, start, enabled)


def reset_window_rows(kv_head):
    return (kv_head + np.arange(R.LCTX)) % R.KVC
