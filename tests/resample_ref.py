"""float64 numpy reference of the audio input conversion, written from the formulae of include/nemotron_asr_amd.h / DESIGN.md section 12
(not from csrc/nasr_resample.h), and the stand-alone C++ driver through which the CPU suite and the GPU suite run the header itself.

Resampler fin -> 16 kHz: g = gcd(fin, 16000), L = 16000 / g, M = fin / g, s = min(1, L / M); Kaiser-windowed sinc, Z = 32 zero crossings per
side at the lower rate, beta = 9, roll-off rho = 0.94, sampled at 1 / L input sample; output n at n M / L input samples."""
import shutil
import subprocess
from fractions import Fraction
from math import ceil, gcd

import numpy as np

RATES = [8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000]
ENCODINGS = {"s16": 0, "f32": 1, "mulaw": 2, "alaw": 3}
Z, BETA, RHO = 32, 9.0, 0.94


def plan(fin):
    g = gcd(fin, 16000)
    L, M = 16000 // g, fin // g
    s = min(Fraction(1), Fraction(L, M))
    half = 0 if L == M else ceil(Fraction(Z) / s * L)
    return L, M, half


def prototype(fin):
    """h[j], j = -half .. half, float64 (not yet normalised)"""
    L, M, half = plan(fin)
    if half == 0:
        return np.ones(1)
    s = min(1.0, L / M)
    j = np.arange(-half, half + 1, dtype=np.float64)
    tau = j / L
    x = tau * s / Z
    w = np.where(np.abs(x) < 1.0, np.i0(BETA * np.sqrt(np.clip(1.0 - x * x, 0.0, None))) / np.i0(BETA), 0.0)
    return s * RHO * np.sinc(s * RHO * tau) * w


def coefficients(fin):
    L, _, _ = plan(fin)
    h = prototype(fin)
    return h * L / h.sum()


def out_ready(fin, n_in):
    L, M, half = plan(fin)
    return max(0, ((n_in - 1) * L - half) // M + 1)


def out_total(fin, n_in):
    L, M, _ = plan(fin)
    return -((-n_in * L) // M)


def out_ready_brute(fin, n_in):
    """outputs n whose last tap (the largest k with |n M - k L| <= half) and, by the rule of the design, position n M + half itself lie
    at or before input frame n_in - 1"""
    L, M, half = plan(fin)
    n = 0
    while n * M + half <= (n_in - 1) * L:
        n += 1
    return n


def out_total_brute(fin, n_in):
    L, M, _ = plan(fin)
    n = 0
    while n * M < n_in * L:
        n += 1
    return n


def mulaw_table():
    c = np.arange(256)
    u = ~c & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int64)


def alaw_table():
    c = np.arange(256) ^ 0x55
    e, m = (c >> 4) & 7, c & 0x0F
    t = np.where(e == 0, (m << 4) + 8, ((m << 4) + 0x108) << np.maximum(e - 1, 0))
    return np.where(c & 0x80, t, -t).astype(np.int64)


def decode(raw, encoding, channels, channel):
    """bytes -> float64 mono, the decode and down-mix of the design (f32 arithmetic where it says f32)"""
    if encoding == "s16":
        v = np.frombuffer(raw, dtype="<i2").astype(np.float32) / np.float32(32768)
    elif encoding == "f32":
        v = np.frombuffer(raw, dtype="<f4").copy()
        v[~np.isfinite(v)] = 0
    else:
        tab = mulaw_table() if encoding == "mulaw" else alaw_table()
        v = tab[np.frombuffer(raw, dtype=np.uint8)].astype(np.float32) / np.float32(32768)
    v = v.reshape(-1, channels)
    if channel >= 0:
        return v[:, channel].astype(np.float64)
    acc = v[:, 0].astype(np.float32)
    for c in range(1, channels):
        acc = (acc + v[:, c]).astype(np.float32)
    return (acc * np.float32(1.0 / channels)).astype(np.float32).astype(np.float64)


def resample(x, fin):
    """float64 value of every output before rounding, and sum |c| |x| over its taps; the coefficients are the f32-rounded table (that
    rounding is part of the design), the sum is float64"""
    L, M, half = plan(fin)
    c = coefficients(fin).astype(np.float32).astype(np.float64)
    n_in = len(x)
    n_out = out_total(fin, n_in)
    y, mag, taps = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out, dtype=np.int64)
    xp = np.concatenate([x, [0.0]])                        # index n_in (and -1) reads the zero
    for n in range(n_out):
        pos = n * M
        k0, k1 = -((half - pos) // L), (pos + half) // L
        k = np.arange(k0, k1 + 1)
        cj = c[pos - k * L + half]
        xv = xp[np.where((k >= 0) & (k < n_in), k, n_in)]
        y[n] = np.dot(cj, xv)
        mag[n] = np.dot(np.abs(cj), np.abs(xv))
        taps[n] = k1 - k0 + 1
    return y * 32768.0, mag * 32768.0, taps


DRIVER = r"""
#include "nasr_resample.h"
#include "wav_header.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace nasr_rs;
static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}
// table <fin>                 : "L M half hist max_taps max_span Z beta rho" then the 2 half + 1 coefficients
// counts <fin> n ..           : out_ready out_total per n
// g711                        : 256 mu-law then 256 A-law values
// conv <fin> <enc> <channels> <channel> <in> <out> [push ..] : the streaming converter over the file's frames in pushes of the given
//                               sizes (what is left goes in one last push), flushed; s16 to <out>; prints the frames out
// wav <corpus>                : records (u32 n, n bytes) -> "rc tag channels rate bits encoding offset bytes" per record
int main(int argc, char **argv) {
    if (argc < 2) return 1;
    if (!strcmp(argv[1], "table") && argc == 3) {
        Plan p;
        if (!make_plan(atoi(argv[2]), &p)) return 3;
        std::vector<float> c;
        build_table(p, c);
        int max_taps = 0; long long max_span = 0;
        for (long long n = 0; n < 4LL * p.M * BLOCK; n++) { if (taps_of(p, n) > max_taps) max_taps = taps_of(p, n); }
        for (long long n = 0; n < 4LL * p.M * BLOCK; n += BLOCK) if (block_span(p, n) > max_span) max_span = block_span(p, n);
        printf("%d %d %d %d %d %lld %d %.17g %.17g\n", p.L, p.M, p.half, p.hist, max_taps, max_span, ZEROS, BETA, ROLLOFF);
        for (float v : c) printf("%.9g\n", (double)v);
        return (int)c.size() == 2 * p.half + 1 ? 0 : 4;
    }
    if (!strcmp(argv[1], "counts") && argc >= 3) {
        Plan p;
        if (!make_plan(atoi(argv[2]), &p)) return 3;
        for (int i = 3; i < argc; i++) printf("%lld %lld\n", out_ready(p, atoll(argv[i])), out_total(p, atoll(argv[i])));
        return 0;
    }
    if (!strcmp(argv[1], "g711")) {
        for (int c = 0; c < 256; c++) printf("%d\n", mulaw_expand(c));
        for (int c = 0; c < 256; c++) printf("%d\n", alaw_expand(c));
        return 0;
    }
    if (!strcmp(argv[1], "conv") && argc >= 8) {
        HostStream hs;
        if (!hs.init(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]))) return 3;
        const std::vector<uint8_t> raw = slurp(argv[6]);
        const size_t fb = (size_t)hs.channels * bytes_per_sample(hs.enc);
        const long long frames = (long long)(raw.size() / fb);
        std::vector<int16_t> out;
        long long at = 0;
        for (int i = 8; i <= argc; i++) {
            long long n = i < argc ? atoll(argv[i]) : frames - at;
            if (n > frames - at) n = frames - at;
            // every push is its own exactly-sized heap block: a read outside the push is an AddressSanitizer report
            std::vector<uint8_t> piece(raw.begin() + (size_t)at * fb, raw.begin() + (size_t)(at + n) * fb);
            const long long before = (long long)out.size();
            hs.push(piece.data(), n, out);
            if ((long long)out.size() - before != out_ready(hs.p, at + n) - out_ready(hs.p, at)) return 5;
            at += n;
        }
        hs.flush(out);
        if ((long long)out.size() != out_total(hs.p, frames)) return 6;
        FILE *f = fopen(argv[7], "wb");
        if (!f) return 2;
        if (!out.empty() && fwrite(out.data(), 2, out.size(), f) != out.size()) return 2;
        fclose(f);
        printf("%zu\n", out.size());
        return 0;
    }
    if (!strcmp(argv[1], "wav") && argc == 3) {
        const std::vector<uint8_t> all = slurp(argv[2]);
        size_t at = 0;
        while (at + 4 <= all.size()) {
            const uint32_t n = wav_header::rd32(&all[at]);
            at += 4;
            if (n > all.size() - at) return 7;
            uint8_t *rec = (uint8_t *)malloc(n ? n : 1);                  // exactly n bytes: one read past them is a report
            memcpy(rec, all.data() + at, n);
            at += n;
            wav_header::Info w;
            memset(&w, 0, sizeof(w));
            char err[160];
            const int rc = wav_header::parse(rec, n, &w, err, sizeof(err));
            if (rc == wav_header::OK && w.data_offset > n) return 8;
            printf("%d %d %d %d %d %d %zu %u|%s\n", rc, w.format_tag, w.channels, w.sample_rate, w.bits, w.encoding, w.data_offset, w.data_bytes, err);
            free(rec);
        }
        return 0;
    }
    return 1;
}
"""


def build_driver(directory, root, sanitize=True):
    """compiles the driver without FMA contraction, under AddressSanitizer / UBSan unless sanitize is False (the GPU suite wants the
    header's values only); returns the program's path"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        raise RuntimeError("no host C++ compiler")
    src, out = directory / "resample_drv.cpp", directory / "resample_drv"
    src.write_text(DRIVER)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", *san, "-ffp-contract=off",
                           f"-I{root / 'nemotron-asr.cpp_amd' / 'csrc'}", f"-I{root / 'nemotron-asr.cpp_amd' / 'host'}", str(src), "-o", str(out)])
    return out


def run_driver(prog, *args, timeout=300):
    r = subprocess.run([str(prog)] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and not r.stderr, (args[:6], r.returncode, r.stderr[-2000:])
    return r.stdout


def convert(prog, directory, raw, fin, encoding, channels=1, channel=0, pushes=(), tag="c"):
    """the header's streaming converter over `raw` (bytes) -> int16 array"""
    src, dst = directory / f"{tag}.raw", directory / f"{tag}.s16"
    src.write_bytes(raw)
    run_driver(prog, "conv", fin, ENCODINGS[encoding], channels, channel, src, dst, *pushes)
    return np.fromfile(dst, dtype="<i2")


def make_input(rng, encoding, frames, channels=1, kind="noise", fin=16000):
    """test audio as raw bytes in the given encoding"""
    n = frames * channels
    if kind == "noise":
        x = rng.uniform(-0.9, 0.9, n)
    elif kind == "chirp":
        t = np.arange(frames) / fin
        f1 = 0.49 * fin
        x = np.repeat(0.8 * np.sin(2 * np.pi * (50.0 * t + 0.5 * (f1 - 50.0) / max(t[-1], 1e-9) * t * t)), channels)
    else:                                                        # full-scale square wave: overshoots past full scale and saturates
        x = np.repeat(np.where((np.arange(frames) // 1500) % 2 == 0, 1.0, -1.0), channels)
    if encoding == "s16":
        return np.clip(np.rint(x * 32768), -32768, 32767).astype("<i2").tobytes()
    if encoding == "f32":
        return x.astype("<f4").tobytes()
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes() if kind == "noise" else (np.clip(x * 127 + 128, 0, 255)).astype(np.uint8).tobytes()
