"""References of the front-end kernels' operations (nemotron-asr.cpp_amd/csrc/kernels_front.hip), numpy only, no GPU.

Two kinds, as in tests/spk_ref.py + tests/spk_kernel_cases.py:

  * float64 references of the OPERATION -- pre-emphasis, window, DFT (np.fft.rfft), power, filterbank, log; per-feature normalisation -- that know nothing about
    butterflies, bit reversal, bands or accumulation order, with the bound of a float32 radix-2 implementation against them (`mel_bound`, `featnorm_bound`:
    every term is written out there);
  * float32 restatements of the kernels' documented order, operation for operation, for `==` (`stream_frames_f32`, `diar_frames_f32`, `featnorm_f32`, `preemph_f32`,
    `dw_f32`).  numpy's float32 arithmetic rounds every multiply and add on its own, as the kernels do (the file is compiled without FMA contraction).

The tables -- padded window, twiddles, transposed filterbank, band table -- are built as nasr_engine.hip builds them and are shared operands: kernel, restatement
and float64 reference read the same float32 values.  The snapshot checksum (`word_term`) and the start state of the greedy LM fusion are restated here too."""
from __future__ import annotations

import numpy as np

NMEL, NBINS, NFFT, HOP, WIN, DIAR_NMEL = 128, 257, 512, 160, 400, 80
MEL_RING, MAX_PUSH = 4096, 1280 * 256
ABUF_CAP = MAX_PUSH + NFFT + 64
KVC, LCTX, D, HID, PRE_CACHE, SUBC, HIST_MAX, BLANK = 326, 70, 1024, 640, 9, 256, 193, 1024
U24 = 2.0 ** -24
F32 = np.float32
GUARD_F32 = F32(5.960464477539063e-8)          # the 2^-24 under the log
PRE = F32(0.97)
S16_SCALE = F32(1.0) / F32(32768.0)


# ---- the tables ------------------------------------------------------------------------------------------------------------------------------------
def padded_window(hann400):
    w = np.zeros(NFFT, F32)
    w[(NFFT - WIN) // 2:(NFFT - WIN) // 2 + WIN] = hann400
    return w


def twiddles():
    """float32 sin / cos of the float32 angle (2 pi_f32 * i) / 512, as nasr_engine.hip"""
    theta = (F32(2.0) * F32(np.pi) * np.arange(NFFT, dtype=F32)) / F32(NFFT)
    assert theta.dtype == F32
    return np.cos(theta).astype(F32), np.sin(theta).astype(F32)


def bands(fb):
    """fb [M][257] -> [M][2]: first and one-past-last bin with a non-zero weight; lo = hi = 0 for an empty filter"""
    out = np.zeros((fb.shape[0], 2), np.int32)
    for m, row in enumerate(fb):
        nz = np.flatnonzero(row != 0)
        if nz.size:
            out[m] = nz[0], nz[-1] + 1
    return out


BITREV = np.array([int(f"{i:09b}"[::-1], 2) for i in range(NFFT)])


# ---- float32 restatements -----------------------------------------------------------------------------------------------------------------------------
def preemph_f32(pcm, last, coeff=PRE):
    """k_preemph: y[i] = x[i] - 0.97 x[i - 1], x = s16 / 32768, x[-1] = last_sample -> (y, new last_sample)"""
    x = pcm.astype(F32) * S16_SCALE
    prev = np.concatenate([[F32(last)], x[:-1]]).astype(F32)
    return x - F32(coeff) * prev, x[-1]


def fft_power_f32(v, cos_t, sin_t, sqrt_trip, twiddle_stride=True, rev_bits=9):
    """v [F][512] windowed frames -> power [F][257]: 9-bit reversal, radix-2 DIT stages m = 2 .. 512, butterfly bf of a stage on (k + j, k + j + m / 2) with
    k = (bf / (m / 2)) m, j = bf % (m / 2), twiddle (cos, -sin)[j * 512 / m]; power = sqrt(re^2 + im^2)^2 (sqrt_trip) or re^2 + im^2"""
    rev = BITREV if rev_bits == 9 else BITREV >> 1
    re, im = np.zeros(v.shape, F32), np.zeros(v.shape, F32)
    re[:, rev] = v
    m = 2
    while m <= NFFT:
        m2, step = m // 2, NFFT // m
        bf = np.arange(NFFT // 2)
        k, j = (bf // m2) * m, bf % m2
        wr, wi = cos_t[j * step if twiddle_stride else j], -sin_t[j * step if twiddle_stride else j]
        i1, i2 = k + j, k + j + m2
        r1, q1, r2, q2 = re[:, i1], im[:, i1], re[:, i2], im[:, i2]
        tr, ti = wr * r2 - wi * q2, wr * q2 + wi * r2
        re[:, i2], im[:, i2], re[:, i1], im[:, i1] = r1 - tr, q1 - ti, r1 + tr, q1 + ti
        m *= 2
    re, im = re[:, :NBINS], im[:, :NBINS]
    p = re * re + im * im
    if sqrt_trip:
        mag = np.sqrt(p)
        p = mag * mag
    assert p.dtype == F32
    return p


def band_sum_f32(pw, fbT, band):
    """sum over the filter's band, k ascending, from 0: pw [F][257], fbT [257][M], band [M][2] -> s [F][M]"""
    s = np.zeros((pw.shape[0], fbT.shape[1]), F32)
    for k in range(int(band[:, 0].min()), int(band[:, 1].max())):
        on = (band[:, 0] <= k) & (k < band[:, 1])
        s[:, on] = s[:, on] + fbT[k, on][None, :] * pw[:, k:k + 1]
    return s


def log_arg_f32(s):
    """the float32 argument of the kernels' logf"""
    return (s + GUARD_F32).astype(F32)


def stream_frames_f32(buf, n_frames, tables, **wrong):
    """k_melframes up to the sum: buf = the slot's audio buffer (float32), frame t = buf[t * 160 : t * 160 + 512] -> s [n_frames][128]"""
    window, fbT, band, cos_t, sin_t = tables
    if n_frames == 0:
        return np.zeros((0, fbT.shape[1]), F32)
    v = np.stack([buf[t * HOP:t * HOP + NFFT] for t in range(n_frames)]) * window[None, :]
    fft_kw = {k: wrong[k] for k in ("twiddle_stride", "rev_bits") if k in wrong}
    pw = fft_power_f32(v.astype(F32), cos_t, sin_t, wrong.get("sqrt_trip", True), **fft_kw)
    b = band.copy()
    b[:, 1] = np.maximum(b[:, 1] + wrong.get("band_end", 0), b[:, 0])
    return band_sum_f32(pw, fbT, b)


class StreamState:
    """the host's and the device's view of one stream's audio buffer, restated: what launch_mel must leave behind after every push"""

    def __init__(self, last=0.0, cnt=256, wpos=0):
        self.abuf = np.zeros((2, ABUF_CAP), F32)          # what a reset leaves: 256 zero samples in parity 0
        self.cnt, self.par, self.last, self.wpos = cnt, 0, F32(last), wpos

    def plan(self, n):
        """-> (n_frames, consumed) of a push of n samples, as the host counts them"""
        have = self.cnt + n
        nf = 0 if have < NFFT else (have - NFFT) // HOP + 1
        return nf, nf * HOP

    def push(self, pcm, tables, coeff=PRE, **wrong):
        """-> dict of what the launch writes: abuf range [cnt, cnt + n) of the parity, the shifted tail [0, left) of the other, last_sample, s [n_frames][128]"""
        n = len(pcm)
        nf, consumed = self.plan(n)
        desc = dict(n=n, cnt=self.cnt, par=self.par, n_frames=nf, mel_wpos=self.wpos, consumed=consumed)
        if n:
            y, self.last = preemph_f32(pcm, self.last, coeff)
            self.abuf[self.par, self.cnt:self.cnt + n] = y
        s = stream_frames_f32(self.abuf[self.par], nf, tables, **wrong)
        left = self.cnt + n - consumed
        if nf > 0:
            self.abuf[self.par ^ 1, :left] = self.abuf[self.par, consumed:consumed + left]
            self.par ^= 1
            self.cnt = left
            self.wpos = (self.wpos + nf) % MEL_RING
        else:
            self.cnt += n
        return desc, s


def diar_windowed(x, n_win, t, window, s16, f64=False, before=None, coeff=PRE):
    """frame t of the window x[:n_win]: centred (start t * 160 - 256), zero outside the window, pre-emphasis restarting at sample 0 (y[0] = x[0])"""
    ty = np.float64 if f64 else F32
    xs = (x[:n_win].astype(F32) / F32(32768.0)) if s16 else x[:n_win].astype(F32)
    xs = xs.astype(ty)
    y = xs.copy()
    y[1:] = xs[1:] - ty(coeff) * xs[:-1]
    if before is not None:                                # a wrong variant: no restart, the sample in front of the window reaches y[0]
        y[0] = xs[0] - ty(coeff) * ty(before)
    idx = t * HOP - NFFT // 2 + np.arange(NFFT)
    ok = (idx >= 0) & (idx < n_win)
    v = np.zeros(NFFT, ty)
    v[ok] = y[idx[ok]]
    return v * window.astype(ty), (np.abs(xs[np.clip(idx, 0, n_win - 1)]) * ok, np.abs(np.where(idx >= 1, xs[np.clip(idx - 1, 0, n_win - 1)], 0)) * ok)


def diar_frames_f32(x, n_win, ts, tables, s16, **wrong):
    """diar_frame up to the sum for the frames ts of one window -> s [len(ts)][80]"""
    window, fbT, band, cos_t, sin_t = tables
    v = np.stack([diar_windowed(x, n_win, t, window, s16, before=wrong.get("before"))[0] for t in ts]).astype(F32)
    pw = fft_power_f32(v, cos_t, sin_t, False)
    return band_sum_f32(pw, fbT, band)


def featnorm_f32(x, denom_wrong=False):
    """k_diar_featnorm step by step on x [n][80] float32: sequential double sum, float mean, double sum of squared float differences, sqrtf, + 1e-5f, IEEE
    reciprocal, float multiply"""
    n = x.shape[0]
    denom = n if denom_wrong else max(n - 1, 1)
    s = np.zeros(x.shape[1], np.float64)
    for t in range(n):
        s = s + x[t].astype(np.float64)
    mean = (s / n).astype(F32)
    var = np.zeros(x.shape[1], np.float64)
    for t in range(n):
        d = (x[t] - mean).astype(F32)
        var = var + d.astype(np.float64) * d.astype(np.float64)
    std = np.sqrt((var / denom).astype(F32)).astype(F32) + F32(1e-5)
    inv = (F32(1.0) / std).astype(F32)
    return ((x - mean[None, :]).astype(F32) * inv[None, :]).astype(F32)


def dw_f32(x, wt, bias, swap_taps=False, w_out=None):
    """k_sub_dw: x [B][Hin][Win][256], wt [9][256] -> [B][Hout][Wout][256]; taps in (kh, kw) order from 0, taps outside the image skipped, multiply and add
    separate, bias last"""
    B, Hin, Win, C = x.shape
    Ho, Wo = Hin // 2 + 1, Win // 2 + 1
    xp = np.zeros((B, Hin + 3, Win + 3, C), F32)
    xp[:, 2:2 + Hin, 2:2 + Win] = x
    inside = np.zeros((Hin + 3, Win + 3), bool)
    inside[2:2 + Hin, 2:2 + Win] = True
    acc = np.zeros((B, Ho, Wo, C), F32)
    order = [(kh, kw) for kh in range(3) for kw in range(3)]
    if swap_taps:
        order = [(kh, kw) for kw in range(3) for kh in range(3)]
    for kh, kw in order:
        ins = inside[kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2][None, :, :, None]
        acc = np.where(ins, acc + wt[kh * 3 + kw][None, None, None, :] * xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2], acc)
    out = acc + bias[None, None, None, :]
    if w_out is not None:
        out[:, :, w_out:] = np.nan
    return out.astype(F32)


# ---- float64 references of the operations and their bounds ------------------------------------------------------------------------------------------------
FFT_STAGES = 9
TWIDDLE_ABS = 15 * U24          # |table - true|: the float32 angle (2 pi_f32, the product with i: 2 u theta <= 12.6 u) and a sinf / cosf within 1 ulp (2 u)
FFT_ETA = TWIDDLE_ABS + 4 * U24 * (np.sqrt(2.0) + TWIDDLE_ABS) / (1 - 4 * U24)          # Higham, ASNA thm 24.2: eta = mu + gamma_4 (sqrt 2 + mu)
POWER_REL = 6 * U24             # re^2, im^2, their sum (2 u), sqrtf (u), the square (2 u + u)


def mel_f64(v64, fb):
    """windowed frames v64 [F][512] float64 -> (log(fb . |rfft|^2 + 2^-24) [F][M], |X| [F][257])"""
    X = np.abs(np.fft.rfft(v64, axis=1))
    return np.log((X * X) @ fb.astype(np.float64).T + 2.0 ** -24), X


def mel_bound(v64, dv, X, fb, band, logf_rel):
    """|float32 radix-2 log-mel - mel_f64|, per frame and filter.  v64 [F][512] the exact windowed frames, dv [F][512] the bound of the float32 pre-emphasis and
    window on each sample (see `stream_dv`), X = |rfft(v64)|, fb [M][257] the weights (>= 0).

      d   = sqrt(512) (g ||v||_2 + (1 + g) ||dv||_2), g = 9 eta / (1 - 9 eta)      every |X_k - fl(X_k)|: log2(512) stages on the frame's 2-norm + table rounding,
                                                                                   the input error through the (unitary up to sqrt 512) transform
      dP  = 2 |X_k| d + d^2 + POWER_REL (|X_k| + d)^2                              the power
      dS  = sum_k w_k dP_k + (nb + 1) u sum_k w_k (P_k + dP_k) + u (S + 2^-24)     product and sequential sum over the nb bins of the band; the add of 2^-24
      r   = dS / (S + 2^-24) < 1/2;  bound = r / (1 - r) + logf_rel |log|          |log(a (1 + x))| <= |x| / (1 - |x|)"""
    g = FFT_STAGES * FFT_ETA / (1 - FFT_STAGES * FFT_ETA)
    nv, ndv = np.linalg.norm(v64, axis=1), np.linalg.norm(dv, axis=1)
    d = (np.sqrt(float(NFFT)) * (g * nv + (1 + g) * ndv))[:, None]
    P = X * X
    dP = 2 * X * d + d * d + POWER_REL * (X + d) ** 2
    w = fb.astype(np.float64).T
    nb = (band[:, 1] - band[:, 0]).astype(np.float64)[None, :]
    S = P @ w
    dS = dP @ w + (nb + 1) * U24 * ((P + dP) @ w) + U24 * (S + 2.0 ** -24)
    r = dS / (S + 2.0 ** -24)
    assert float(r.max()) < 0.5, f"a mel sum dominated by cancellation: r = {r.max()}"
    return r / (1 - r) + logf_rel * np.abs(np.log(S + 2.0 ** -24))


def stream_dv(xa, xpa, window):
    """bound of the float32 pre-emphasis and window product: |x| and |x_prev| [F][512] -> u (0.97 |x_prev| + |y|) w (1 + u) + u |v|, with |y| <= |x| + 0.97 |x_prev|"""
    w = window.astype(np.float64)[None, :]
    ya = xa + 0.97 * xpa
    return U24 * (0.97 * xpa + ya) * w * (1 + U24) + U24 * ya * w


def featnorm_f64(x):
    """x [n][M] -> (x - mean) / (std + 1e-5), std Bessel-corrected with max(n - 1, 1)"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    mean = x.mean(0)
    std = np.sqrt(((x - mean) ** 2).sum(0) / max(n - 1, 1)) + 1e-5
    return (x - mean) / std, mean, std


def featnorm_bound(x64, e):
    """|k_diar_featnorm(x) - featnorm_f64(x64)| where |x - x64| <= e [n][M] elementwise.
      e_mean = mean_t e + 2 u max|x|                the mean of perturbed values; the double sum is exact to 2^-53 n, the float mean rounds once
      e_diff = e + e_mean + u |x - mean|            the float difference
      e_std  = ||e_diff||_2 / sqrt(denom) + 3 u std + u 1e-5        ||.||_2 is 1-Lipschitz; float var, sqrtf, the add
      bound  = e_diff / std + |x - mean| e_std / std^2 (1 - e_std / std)^-1 + 3 u |ref|      reciprocal, product; inf where e_std >= std / 2, 0 where n = 1"""
    ref, mean, std = featnorm_f64(x64)
    n = x64.shape[0]
    denom = max(n - 1, 1)
    e_mean = e.mean(0) + 2 * U24 * np.abs(x64).max(0)
    diff = np.abs(x64 - mean)
    e_diff = e + e_mean[None, :] + U24 * diff
    e_std = np.linalg.norm(e_diff, axis=0) / np.sqrt(denom) + 3 * U24 * std + U24 * 1e-5
    if n == 1:
        return np.zeros_like(ref)          # x - mean is exactly 0 in any arithmetic: the result is exactly 0
    q = e_std / std
    ok = q < 0.5                           # no statement where the perturbation of std is comparable with std itself (two nearly equal frames): inf
    qs = np.where(ok, q, 0.0)
    return np.where(ok[None, :], e_diff / std + diff * (qs / std) / (1 - qs) + 3 * U24 * np.abs(ref) + 1e-30, np.inf)


# ---- stream state ----------------------------------------------------------------------------------------------------------------------------------------
def fmix32(h):
    h = np.asarray(h, np.uint32)
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def checksum(words, word0):
    """nasr_snap::checksum: sum over the words of fmix32(w ^ (index * 0x9E3779B1)) mod 2^64, index = word0 + position"""
    words = np.asarray(words, np.uint32)
    with np.errstate(over="ignore"):
        idx = (np.uint32(word0) + np.arange(words.size, dtype=np.uint32)) * np.uint32(0x9E3779B1)
        return int(fmix32(words ^ idx).astype(np.uint64).sum(dtype=np.uint64))


def greedy_start(attached, start, enabled):
    """nasr_lm::greedy_start"""
    return -1 if not enabled else (start if attached else 0)


DECCTRL_FIELDS = ("t", "n_frames", "symbols", "prev_token", "cur", "n_tok", "active", "iterations", "row", "dirty", "frame0", "frame_next")
DECCTRL_RESET = dict(t=0, n_frames=0, symbols=0, prev_token=BLANK, cur=0, n_tok=0, active=0, iterations=0, row=0, dirty=1, frame0=0, frame_next=0)
