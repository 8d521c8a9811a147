"""The host arithmetic of a push (nemotron-asr.cpp_amd/csrc/nasr_step_plan.h): frames of a push, graph-step eligibility, the cut of a long push.
No GPU: the header is plain C++ and is compiled with the host compiler under AddressSanitizer and UBSan into a stand-alone program, like
tests/test_gemm_plan.py (the same stub of <hip/hip_runtime.h> lets the program read nasr_internal.h beside it).  The program answers one
case per input line; the expected values come from models written here:

  * framing: a literal run of the reference preprocessor's buffer (src/preprocessor.cpp:320-328) -- the samples waiting plus the samples
    pushed, a 512-sample frame taken while 512 are there, 160 samples dropped per frame; a fresh stream's buffer holds 256 zeros.
  * graph_step_chunks: a transcription of the loop it replaced in try_graph_step (nasr_abi.hip before this header existed):

        const int chunk_mel = PRE_CACHE + 8 * T, shift = 8 * T;
        int G = -1;
        for (int b = 0; b < B; b++) {
            const int n = n_samples[b];
            if (n <= 0 || n > MAX_PUSH) return 0;
            const int avail = s->abuf_cnt + n;
            const int nf = avail < NFFT ? 0 : (avail - NFFT + HOP) / HOP;
            const int mc = s->mel_count + nf;
            if (mc < chunk_mel) return 0;
            const int g = (mc - chunk_mel) / shift + 1;               // chunks this push completes
            if (G < 0) G = g;
            if (g != G) return 0;                                     // every stream must complete the same number
            if (nf > max_frames_per_push(T * G)) return 0;            // 8 * T * G + 16
        }
        if (G > 1) {
            if (!e->opt_multichunk || B * G * T > e->w_rows || G * T > MAXNEW) return 0;
        }

    with nf from the framing model above, not from the closed form.
"""
import shutil
import subprocess
from pathlib import Path

import pytest

from tests.test_gemm_plan import HIP_STUB

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"

NFFT, HOP, PRE_CACHE, MAXNEW = 512, 160, 9, 256
MAX_PUSH = 1280 * MAXNEW

DRIVER = r"""
#include "nasr_internal.h"
#include "nasr_step_plan.h"
#include "nasr_offline_plan.h"
#include <cstdio>
#include <vector>
static_assert(nasr::NFFT == 512 && nasr::HOP == 160 && nasr::PRE_CACHE == 9 && nasr::MAXNEW == 256 && nasr::MAX_PUSH == 1280 * 256, "the test's constants");
// one case per line of stdin, one answer per line of stdout:
//   F cnt n par                        -> n_frames consumed cnt' par' mel_count' mel_wpos    (fill_pcm_counts + apply_pcm_counts; mel window (4090, 10))
//   M n                                -> mel_frames(n) push_frames(256, n)
//   C mel_count T                      -> chunks_completed
//   G T B w_rows multichunk (cnt mel n) x B -> graph_step_chunks
//   S T B w_rows                       -> piece_samples
//   W first count have cap             -> ring_window (cap 0: nasr::TOK_CAP)
int main() {
    char op;
    while (scanf(" %c", &op) == 1) {
        if (op == 'F') {
            int cnt, n, par;
            if (scanf("%d %d %d", &cnt, &n, &par) != 3) return 2;
            nasr::PcmDesc d;
            memset(&d, 0, sizeof(d));
            nasr_step::fill_pcm_counts(d, n, cnt, par, 4090, 10);
            int c = cnt, p = par, mc = 10;
            nasr_step::apply_pcm_counts(d, c, p, mc);
            if (d.n != n || d.cnt != cnt || d.par != par || d.n_frames != nasr_step::push_frames(cnt, n)) return 3;
            printf("%d %d %d %d %d %d\n", d.n_frames, d.consumed, c, p, mc, d.mel_wpos);
        } else if (op == 'M') {
            long long n;
            if (scanf("%lld", &n) != 1) return 2;
            printf("%d %d\n", nasr_plan::mel_frames(n), nasr_step::push_frames(256, n));
        } else if (op == 'C') {
            int mc, T;
            if (scanf("%d %d", &mc, &T) != 2) return 2;
            printf("%d\n", nasr_step::chunks_completed(mc, T));
        } else if (op == 'G') {
            int T, B, w_rows, multi;
            if (scanf("%d %d %d %d", &T, &B, &w_rows, &multi) != 4) return 2;
            std::vector<int> cnt(B), mel(B);
            std::vector<int32_t> n(B);
            for (int b = 0; b < B; b++) if (scanf("%d %d %d", &cnt[b], &mel[b], &n[b]) != 3) return 2;
            printf("%d\n", nasr_step::graph_step_chunks(cnt.data(), mel.data(), n.data(), B, T, w_rows, multi != 0));
        } else if (op == 'S') {
            int T, B, w_rows;
            if (scanf("%d %d %d", &T, &B, &w_rows) != 3) return 2;
            printf("%lld\n", (long long)nasr_step::piece_samples(T, B, w_rows));
        } else if (op == 'W') {
            long long first, have;
            int count, cap;
            if (scanf("%lld %d %lld %d", &first, &count, &have, &cap) != 4) return 2;
            printf("%d\n", nasr_step::ring_window(first, count, have, cap ? cap : nasr::TOK_CAP));
        } else return 2;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("step_plan")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(HIP_STUB)
    (d / "drv.cpp").write_text(DRIVER)
    exe = d / "step_plan"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{d}", f"-I{CSRC}", f"-I{ROOT / 'include'}", str(d / "drv.cpp"), "-o", str(exe)])

    def run(cases):
        """cases: tuples (op, ints...) -> one list of ints per case"""
        text = "".join(" ".join(str(v) for v in c) + "\n" for c in cases)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
        out = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return run


def framing(waiting, pushed):
    """(frames, samples left) of the reference's buffer: a 512-sample frame while 512 samples are there, every 160 samples"""
    have, frames = waiting + pushed, 0
    while have >= NFFT:
        frames += 1
        have -= HOP
    return frames, have


def test_push_frames_and_the_counts_after_a_push(plan):
    ns = sorted(set(range(0, 1301)) | {MAX_PUSH - 1, MAX_PUSH})          # cnt + n = 511, 512, 671, 672 lie within 0 .. 1300 for every cnt
    cases, want = [], []
    for cnt in range(0, NFFT):
        for n in ns:
            par = (cnt + n) & 1
            f, left = framing(cnt, n)
            cases.append(("F", cnt, n, par))
            # n_frames, consumed, cnt', par' (flips exactly when frames were taken), mel_count', mel_wpos = (4090 + 10) mod 4096
            want.append([f, f * HOP, left, par ^ (1 if f > 0 else 0), 10 + f, 4])
    for total, f in ((511, 0), (512, 1), (671, 1), (672, 2)):          # the first and the second frame's edge, from every cnt
        assert all(want[cases.index(("F", c, total - c, total & 1))][0] == f for c in (0, 256, 511))
    got = plan(cases)
    bad = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, bad[:10]
    assert all(0 <= w[2] < NFFT for w in want)          # what is left is again a valid cnt


def test_a_stream_of_pushes_from_256_zeros(plan):
    """the counts carried from push to push, as the engine's mirror carries them"""
    import random
    rng = random.Random(5)
    cnt, par, cases, want = 256, 0, [], []
    for _ in range(400):
        n = rng.choice([0, 1, 159, 160, 161, 1280, 2560, rng.randrange(0, 20000)])
        f, left = framing(cnt, n)
        cases.append(("F", cnt, n, par))
        want.append([f, f * HOP, left, par ^ (1 if f > 0 else 0), 10 + f, 4])
        cnt, par = left, par ^ (1 if f > 0 else 0)
    assert plan(cases) == want


def test_mel_frames_is_push_frames_from_256_zeros(plan):
    ns = list(range(0, 1301)) + [MAX_PUSH - 1, MAX_PUSH, 16000 * 60, -5]
    got = plan([("M", n) for n in ns])
    assert got == [[framing(256, max(n, 0))[0]] * 2 for n in ns]
    assert got[0] == [0, 0] and got[255] == [0, 0] and got[256] == [1, 1] and got[416] == [2, 2]


def graph_step_chunks_model(T, B, w_rows, multichunk, streams):
    """the parent's loop (module docstring); streams = [(abuf_cnt, mel_count, n)] * B"""
    chunk_mel, shift = PRE_CACHE + 8 * T, 8 * T
    G = -1
    for cnt, mel, n in streams:
        if n <= 0 or n > MAX_PUSH:
            return 0
        nf = framing(cnt, n)[0]
        mc = mel + nf
        if mc < chunk_mel:
            return 0
        g = (mc - chunk_mel) // shift + 1
        if G < 0:
            G = g
        if g != G:
            return 0
        if nf > 8 * T * G + 16:
            return 0
    if G > 1 and (not multichunk or B * G * T > w_rows or G * T > MAXNEW):
        return 0
    return G


def samples_for(frames, cnt):
    """fewest samples that complete `frames` frames on a buffer holding cnt"""
    return NFFT + (frames - 1) * HOP - cnt


def test_graph_step_chunks(plan):
    cases, want, stated = [], [], []          # stated: the value the case was built for (None: the model's word alone)

    def add(T, B, w_rows, multi, streams, expect=None):
        cases.append(("G", T, B, w_rows, int(multi)) + tuple(v for s in streams for v in s))
        want.append([graph_step_chunks_model(T, B, w_rows, multi, streams)])
        stated.append(expect)

    BIG = 1 << 20
    for T in (1, 2, 7, 14):
        shift = 8 * T
        for B in (1, 2, 3):
            cnt, mel = 352, PRE_CACHE                                   # the steady state: a chunk's samples leave 352 waiting, 9 frames stay buffered
            one = (cnt, mel, samples_for(shift, cnt))
            add(T, B, BIG, True, [one] * B, 1)                          # streams in step
            add(T, B, BIG, True, [(cnt, mel, one[2] + HOP - 1)] * B, 1)  # ... with samples to spare, short of another frame
            ahead = (cnt, mel + shift, one[2])                          # one stream a chunk ahead
            add(T, B, BIG, True, [ahead] + [one] * (B - 1), 0 if B > 1 else 2)
            add(T, B, BIG, True, [one] * (B - 1) + [ahead], 0 if B > 1 else 2)
            add(T, B, BIG, True, [one] * (B - 1) + [(cnt, mel, one[2] - 1)], 0)          # one frame short of a chunk
            add(T, B, BIG, True, [(cnt, mel - 1, one[2])] * B, 0)
            for G in (2, 3):                                            # a push that completes G chunks
                many = (cnt, mel, samples_for(G * shift, cnt))
                add(T, B, BIG, True, [many] * B, G)
                add(T, B, BIG, False, [many] * B, 0)                    # "multichunk" off
                add(T, B, B * G * T, True, [many] * B, G)               # the rows exactly fill the workspace
                add(T, B, B * G * T - 1, True, [many] * B, 0)           # ... one row more than it has
                add(T, B, BIG, True, [many] * (B - 1) + [(cnt, mel, samples_for((G - 1) * shift, cnt))], 0 if B > 1 else G - 1)
            # G = MAXNEW / T and MAXNEW / T + 1 chunks: two of them buffered already, so that the push stays within MAX_PUSH
            gmax = MAXNEW // T
            for G, expect in ((gmax, gmax), (gmax + 1, 0)):
                s = (cnt, mel + 2 * shift, samples_for((G - 2) * shift, cnt))
                assert 0 < s[2] <= MAX_PUSH
                add(T, B, BIG, True, [s] * B, expect)
            add(T, B, BIG, True, [(cnt, mel, samples_for((gmax + 1) * shift, cnt))] * B, 0)      # the same from nothing buffered: more than MAX_PUSH samples
            # 16 and 17 frames beyond the chunk: at T = 7 and 14 still one chunk, and 17 are more than the captured front end takes
            add(T, B, BIG, True, [(cnt, mel, samples_for(shift + 16, cnt))] * B, 1 if T >= 7 else 3 if T == 1 else 2)
            add(T, B, BIG, True, [(cnt, mel, samples_for(shift + 17, cnt))] * B, 0 if T >= 7 else 3 if T == 1 else 2)
            add(T, B, BIG, True, [one] * (B - 1) + [(cnt, mel, 0)], 0)                          # n = 0
            add(T, B, BIG, True, [one] * (B - 1) + [(cnt, mel + 2 * MAXNEW * 8, MAX_PUSH + 1)], 0)  # n = MAX_PUSH + 1
            add(T, B, BIG, True, [(0, mel, MAX_PUSH)] * B)                                      # n = MAX_PUSH on an empty buffer
    assert all(w == [s] for w, s in zip(want, stated) if s is not None), [(c, w, s) for c, w, s in zip(cases, want, stated) if s is not None and w != [s]][:5]
    got = plan(cases)
    bad = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, bad[:10]


def test_chunks_completed(plan):
    cases = [("C", mc, T) for T in (1, 2, 7, 14) for mc in range(0, PRE_CACHE + 8 * T * 4 + 2)]
    want = []
    for _, mc, T in cases:              # chunks taken one at a time: 9 + 8 T frames needed, 8 T leave the buffer
        g = 0
        while mc >= PRE_CACHE + 8 * T:
            g, mc = g + 1, mc - 8 * T
        want.append([g])
    assert plan(cases) == want


def test_piece_samples(plan):
    # (T, B, w_rows) -> whole chunks per piece: min(MAXNEW / T, w_rows / (B T)), at least one
    table = [((1, 1, 4096), 256), ((1, 8, 4096), 256), ((1, 32, 4096), 128), ((1, 3, 4), 1), ((1, 5, 4), 1),      # the last: B T above w_rows, clamped to 1
             ((14, 1, 4096), 18), ((14, 3, 14 * 3 * 18), 18), ((14, 3, 14 * 3 * 18 - 1), 17), ((14, 3, 42), 1), ((14, 4, 42), 1), ((14, 512, 7168), 1)]
    got = plan([("S",) + k for k, _ in table])
    assert got == [[g * 8 * k[0] * HOP] for k, g in table]
    assert all(v[0] <= MAX_PUSH for v in got)


def ring_model(first, count, have, cap):
    """brute force: the device has written items 0 .. have - 1, item i to place i % cap; of the items asked for, those that exist are handed over,
    each read from its place -- and the answer is "too old" (-1) when there are some and the place of the first of them holds a later item"""
    ring = {}
    for i in range(have):
        ring[i % cap] = i
    asked = [i for i in range(first, first + count) if i < have]
    if asked and ring[asked[0] % cap] != asked[0]:
        return -1
    assert all(ring[i % cap] == i for i in asked)                      # the first is there: so are the rest
    return len(asked)


@pytest.mark.parametrize("cap,label", [(8, 8), (4096, 0)])
def test_ring_window_against_a_brute_force_ring(plan, cap, label):
    """the range the four read-out getters of nasr_abi.hip hand over (nasr_step::ring_window): first in {0, 1, have - cap - 1, have - cap,
    have - cap + 1, have - 1, have, have + 1}, count in {0, 1, cap, cap + 1}, have in {0, 1, cap - 1, cap, cap + 1, 3 cap + 5}, at cap = 8 and at
    TOK_CAP.  A negative first (have - cap - 1 and its neighbours while have <= cap) is no case: every getter refuses it before it gets here"""
    assert plan([("W", 0, 1, 1, 0)]) == [[1]] and plan([("W", 0, 4097, 5000, 0)]) == [[-1]] and plan([("W", 904, 4097, 5000, 0)]) == [[4096]]      # cap 0 is TOK_CAP = 4096
    cases, want = [], []
    for have in (0, 1, cap - 1, cap, cap + 1, 3 * cap + 5):
        for first in sorted({0, 1, have - cap - 1, have - cap, have - cap + 1, have - 1, have, have + 1}):
            for count in (0, 1, cap, cap + 1):
                if first < 0:
                    continue
                cases.append(("W", first, count, have, label))
                want.append([ring_model(first, count, have, cap)])
    assert len(cases) >= 100 and [-1] in want and [cap] in want and [0] in want
    assert plan(cases) == want
