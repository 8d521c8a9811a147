// nasr_resample.h -- the arithmetic of the device-side audio input conversion (other rates, encodings, channel counts -> the 16 kHz s16
// mono the front end reads), pure code without HIP so that the CPU suite compiles it with g++ under sanitizers
// (tests/test_resample_math.py), like nasr_align.h / nasr_logprob.h / nasr_topk.h.  kernels_audio.hip includes it and runs the same
// functions on the device: device and host agree bit for bit.
//
// Rational resampler fin -> 16 000 Hz, g = gcd(fin, 16000), L = 16000 / g, M = fin / g, s = min(1, L / M).  Prototype: Kaiser-windowed
// sinc with Z = 32 zero crossings per side at the lower of the two rates, beta = 9, roll-off rho = 0.94, sampled at 1 / L input sample:
//   half = Z * max(L, M)  (= ceil(Z / s * L)),  j in [-half, half],  tau = j / L,  x = tau * s / Z
//   h[j] = s rho sinc(s rho tau) I0(beta sqrt(1 - x^2)) / I0(beta)  for |x| < 1, else 0;    c[j] = (float)(h[j] L / sum h)
// computed in double on the host, rounded once.  Output n sits at n * M (units of 1 / L input sample):
//   acc = 0;  for k ascending with |n M - k L| <= half:  acc = fadd_rn(acc, fmul_rn(c[n M - k L], x[k]));   never an FMA
//   y[n] = clamp(rintf(acc * 32768), -32768, 32767)
// x[k] = 0 for k < 0 and for k at or past the end of the stream.  The table is stored linearly, c[j] at index j + half: the lanes of a
// wave (consecutive n) read, at the same loop trip, indices that lie within one window of L floats -- the [tap][phase] layout.
// A stream keeps the last hist = 2 half / L + 1 decoded input frames: output n is produced once (n_in - 1) L - half >= n M, and then the
// oldest frame an output not yet produced can need is n_in - hist.
#pragma once
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <vector>

#if defined(__HIPCC__)
#define NASR_RS_HD __host__ __device__ __forceinline__
#else
#define NASR_RS_HD inline
#endif

namespace nasr_rs {

constexpr int ZEROS = 32;              // zero crossings per side
constexpr double BETA = 9.0, ROLLOFF = 0.94;
constexpr int ENC_S16 = 0, ENC_F32 = 1, ENC_MULAW = 2, ENC_ALAW = 3;      // = NASR_AUDIO_*
constexpr int MAX_CHANNELS = 8;
constexpr int BLOCK = 256;             // outputs per workgroup
constexpr int SPAN_CAP = 1024;         // input frames a workgroup stages at most (48 kHz: 255 * 3 + 193 = 958)
constexpr int HIST_MAX = 193;          // largest hist of the supported rates (48 kHz)
constexpr int N_RATES = 8;

struct Plan { int fin, L, M, half, hist; };

NASR_RS_HD int rate_at(int i) {
    switch (i) { case 0: return 8000; case 1: return 11025; case 2: return 16000; case 3: return 22050;
                 case 4: return 24000; case 5: return 32000; case 6: return 44100; case 7: return 48000; }
    return 0;
}
NASR_RS_HD bool make_plan(int fin, Plan *p) {
    bool ok = false;
    for (int i = 0; i < N_RATES; i++) ok = ok || rate_at(i) == fin;
    if (!ok) return false;
    int a = fin, b = 16000;
    while (b) { const int t = a % b; a = b; b = t; }
    p->fin = fin; p->L = 16000 / a; p->M = fin / a;
    p->half = p->L == p->M ? 0 : ZEROS * (p->L > p->M ? p->L : p->M);
    p->hist = 2 * p->half / p->L + 1;
    return true;
}
NASR_RS_HD bool valid_format(int fin, int enc, int channels, int channel) {
    Plan p;
    return make_plan(fin, &p) && enc >= ENC_S16 && enc <= ENC_ALAW && channels >= 1 && channels <= MAX_CHANNELS && channel >= -1 && channel < channels;
}
NASR_RS_HD int bytes_per_sample(int enc) { return enc == ENC_S16 ? 2 : enc == ENC_F32 ? 4 : 1; }

NASR_RS_HD long long floor_div(long long a, long long b) { const long long q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }   // b > 0
NASR_RS_HD long long ceil_div(long long a, long long b) { return -floor_div(-a, b); }

// 16 kHz samples available after n_in input frames / in all once the stream has ended
NASR_RS_HD long long out_ready(const Plan &p, long long n_in) {
    const long long r = floor_div((n_in - 1) * p.L - p.half, p.M) + 1;
    return r > 0 ? r : 0;
}
NASR_RS_HD long long out_total(const Plan &p, long long n_in) { return n_in > 0 ? ceil_div(n_in * p.L, p.M) : 0; }
// first and last input frame output n reads
NASR_RS_HD long long k_first(const Plan &p, long long n) { return ceil_div(n * p.M - p.half, p.L); }
NASR_RS_HD long long k_last(const Plan &p, long long n) { return floor_div(n * p.M + p.half, p.L); }
NASR_RS_HD int taps_of(const Plan &p, long long n) { return (int)(k_last(p, n) - k_first(p, n) + 1); }
// input frames the outputs [n, n + BLOCK) read: what a workgroup stages
NASR_RS_HD long long block_span(const Plan &p, long long n) { return k_last(p, n + BLOCK - 1) - k_first(p, n) + 1; }

// ---- ITU-T G.711 expansion to 16-bit linear -------------------------------------------------------------------------------------
NASR_RS_HD int mulaw_expand(int code) {
    const int u = ~code & 0xff, t = (((u & 0x0f) << 3) + 0x84) << ((u >> 4) & 7);
    return (u & 0x80) ? 0x84 - t : t - 0x84;
}
NASR_RS_HD int alaw_expand(int code) {
    const int a = (code ^ 0x55) & 0xff, e = (a >> 4) & 7, m = a & 0x0f;
    const int t = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
    return (a & 0x80) ? t : -t;
}

NASR_RS_HD float rs_fmul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    const float r = a * b;
    return r;
#endif
}
NASR_RS_HD float rs_fadd(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    const float r = a + b;
    return r;
#endif
}

// sample `idx` (frame * channels + channel) of an interleaved buffer as f32
NASR_RS_HD float decode_sample(const void *in, int enc, long long idx) {
    if (enc == ENC_S16) return (float)((const int16_t *)in)[idx] / 32768.0f;
    if (enc == ENC_F32) {
        uint32_t u;
        memcpy(&u, (const char *)in + idx * 4, 4);
        if ((u & 0x7f800000u) == 0x7f800000u) return 0.0f;            // Inf / NaN read as silence
        float v;
        memcpy(&v, &u, 4);
        return v;
    }
    const int c = ((const uint8_t *)in)[idx];
    return (float)(enc == ENC_MULAW ? mulaw_expand(c) : alaw_expand(c)) / 32768.0f;
}
// one input frame: a channel, or (channel = -1) the mean of the channels: f32 sum in channel order times (float)(1 / channels)
NASR_RS_HD float decode_frame(const void *in, int enc, int channels, int channel, long long frame) {
    if (channel >= 0) return decode_sample(in, enc, frame * channels + channel);
    float sum = decode_sample(in, enc, frame * channels);
    for (int c = 1; c < channels; c++) sum = rs_fadd(sum, decode_sample(in, enc, frame * channels + c));
    return rs_fmul(sum, (float)(1.0 / (double)channels));
}

// where the input frames of a launch come from: the stream's history (frames [n_before - hist_len, n_before)), the push itself
// (frames [n_before, n_before + n_push)), silence before the stream's start and after its end
struct Source {
    const void *in; const float *hist;       // hist may be null (one-shot conversion: nothing precedes the buffer)
    long long n_before, n_push;
    int enc, channels, channel, hist_len;
    NASR_RS_HD float at(long long k) const {
        if (k < 0 || k >= n_before + n_push) return 0.0f;
        if (k >= n_before) return decode_frame(in, enc, channels, channel, k - n_before);
        const long long i = k - (n_before - hist_len);
        return hist && i >= 0 ? hist[i] : 0.0f;
    }
    // entry i of the history the NEXT launch finds
    NASR_RS_HD float hist_next(int i) const { return at(n_before + n_push - hist_len + i); }
};

// the tap loop of output n; x(k0, i) = input frame k0 + i as f32, k0 = the first frame the output reads; c = the table, c[j + half].
// The positions are 64-bit, the loop itself walks a pointer and a 32-bit counter (one output has at most 193 taps)
template <typename X>
NASR_RS_HD float accumulate(const Plan &p, const float *c, long long n, X x) {
    const long long pos = n * p.M, k0 = ceil_div(pos - p.half, p.L), k1 = floor_div(pos + p.half, p.L);
    const int taps = (int)(k1 - k0 + 1), step = p.L;
    const float *cj = c + (int)(pos - k0 * p.L + p.half);
    float acc = 0.0f;
    for (int i = 0; i < taps; i++, cj -= step) acc = rs_fadd(acc, rs_fmul(*cj, x(k0, i)));
    return acc;
}
NASR_RS_HD int16_t quantize(float acc) {
    float r = rintf(acc * 32768.0f);         // ties to even
    if (r != r) r = 0.0f;
    return (int16_t)(r < -32768.0f ? -32768.0f : r > 32767.0f ? 32767.0f : r);
}

// ---- host only: the coefficient table, and the streaming converter restated (what the kernel does launch by launch) ----------------
inline double bessel_i0(double x) {         // power series sum ((x / 2)^k / k!)^2
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}
inline void build_table(const Plan &p, std::vector<float> &c) {
    const int n = 2 * p.half + 1;
    c.assign((size_t)n, 1.0f);
    if (p.half == 0) return;
    const double pi = 3.14159265358979323846, s = p.L < p.M ? (double)p.L / (double)p.M : 1.0, i0b = bessel_i0(BETA);
    std::vector<double> h((size_t)n);
    double sum = 0.0;
    for (int j = -p.half; j <= p.half; j++) {
        const double tau = (double)j / (double)p.L, x = tau * s / (double)ZEROS, t = s * ROLLOFF * tau;
        double v = 0.0;
        if (fabs(x) < 1.0) v = s * ROLLOFF * (t == 0.0 ? 1.0 : sin(pi * t) / (pi * t)) * bessel_i0(BETA * sqrt(1.0 - x * x)) / i0b;
        h[(size_t)(j + p.half)] = v;
        sum += v;
    }
    for (int i = 0; i < n; i++) c[(size_t)i] = (float)(h[(size_t)i] * (double)p.L / sum);
}

struct HostStream {
    Plan p; int enc = ENC_S16, channels = 1, channel = 0;
    long long n_in = 0, n_out = 0;
    std::vector<float> table, hist;
    bool init(int fin, int enc_, int channels_, int channel_) {
        if (!valid_format(fin, enc_, channels_, channel_)) return false;
        make_plan(fin, &p); enc = enc_; channels = channels_; channel = channel_;
        build_table(p, table);
        reset();
        return true;
    }
    void reset() { n_in = n_out = 0; hist.assign((size_t)p.hist, 0.0f); }
    Source source(const void *in, long long n) const {
        Source s;
        s.in = in; s.hist = hist.data(); s.n_before = n_in; s.n_push = n; s.enc = enc; s.channels = channels; s.channel = channel; s.hist_len = p.hist;
        return s;
    }
    void produce(const Source &s, long long upto, std::vector<int16_t> &out) {
        for (long long n = n_out; n < upto; n++) out.push_back(quantize(accumulate(p, table.data(), n, [&](long long k0, int i) { return s.at(k0 + i); })));
        if (upto > n_out) n_out = upto;
    }
    // n more input frames: appends the samples they complete
    void push(const void *in, long long n, std::vector<int16_t> &out) {
        const Source s = source(in, n);
        produce(s, out_ready(p, n_in + n), out);
        if (n > 0) {
            std::vector<float> next((size_t)p.hist);
            for (int i = 0; i < p.hist; i++) next[(size_t)i] = s.hist_next(i);
            hist.swap(next);
        }
        n_in += n;
    }
    // the stream has ended: the samples that waited for input which will not come
    void flush(std::vector<int16_t> &out) { produce(source(nullptr, 0), out_total(p, n_in), out); }
};

}  // namespace nasr_rs
