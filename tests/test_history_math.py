"""The arithmetic of the frame-history ring (nemotron-asr.cpp_amd/csrc/nasr_history.h; engine option "frame_history").  No GPU: the header
is compiled with the host compiler under AddressSanitizer and UBSan into a stand-alone program, run as a child process, and its three
functions are compared with a brute-force restatement over a grid of (valid_from, done, N, first, count).

The restatement does not read the header.  A stream that has decoded `done` frames keeps frame f iff valid_from <= f < done and
f >= done - N; frame f lives in ring row f mod N; a window is kept iff every frame of it is kept (a window without a frame names no row
and is kept); the rows of a window, in frame order, are one ascending run of ring rows, or two where the window crosses row N - 1 -> 0."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"

DRIVER = r"""
#include "nasr_history.h"
#include <cstdio>
#include <initializer_list>
// one case per line of stdin: valid_from done N first count -> "range_first range_count kept row0 n0 n1 | row of every frame" (the runs and
// rows only where the window is kept and fits the ring: the engine asks for no other)
int main() {
    long long vf, done, first;
    int N, count;
    while (scanf("%lld %lld %d %lld %d", &vf, &done, &N, &first, &count) == 5) {
        const nasr_hist::Range r = nasr_hist::retained(vf, done, N);
        const bool kept = nasr_hist::window_kept(r, first, count);
        printf("%lld %d %d", (long long)r.first, (int)r.count, kept ? 1 : 0);
        if (kept && count <= N) {
            const nasr_hist::Runs u = nasr_hist::ring_runs(first, count, N);
            printf(" %d %d %d |", u.row0, u.n0, u.n1);
            for (int j = 0; j < count; j++) printf(" %d", nasr_hist::run_row(u, j));
            for (int j = 0; j < count; j++) if (nasr_hist::ring_row(first + j, N) != nasr_hist::run_row(u, j)) return 3;      // the append's row is the gather's
        }
        printf("\n");
    }
    for (int n : {0, 64, 128, 2048}) if (!nasr_hist::valid_frames(n)) return 4;
    for (int n : {-64, 1, 63, 65, 100, 2047, 2112, 4096}) if (nasr_hist::valid_frames(n)) return 5;
    if (nasr_hist::ring_bytes(512, 2048) != 512ll * 2048 * 2560 || nasr_hist::ROW_VECS != 160) return 6;
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("history_math")
    (d / "driver.cpp").write_text(DRIVER)
    out = d / "driver"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
                           str(d / "driver.cpp"), "-o", str(out)])
    return out


def kept_frames(valid_from, done, N):
    return [f for f in range(max(done - 2 * N, 0), done + 2) if valid_from <= f < done and f >= done - N]


def grid():
    cases = []
    for N in (64, 128):
        # done: nothing decoded, less than a ring, exactly a ring, a ring and a bit, several rings, a multiple of N
        for done in (0, 1, N - 1, N, N + 1, N + 37, 2 * N, 2 * N + 22, 5 * N - 1):
            for valid_from in sorted({0, 1, max(done - N, 0), max(done - 5, 0), done}):          # create / reset, and forks at several points (done: an empty history)
                lo = max(valid_from, done - N, 0)
                wrap = (done // N) * N                       # the frame in ring row 0 nearest below done
                firsts = sorted({0, lo - 1, lo, lo + 1, wrap - 3, wrap - 1, wrap, wrap + 1, done - 1, done, done + 1} - {-1, -2, -3, -4})
                for first in firsts:
                    if first < 0:
                        continue
                    counts = sorted({0, 1, 2, 3, wrap - first, wrap - first + 1, done - first, done - first + 1, N, N - 1, N + 1})
                    cases += [(valid_from, done, N, first, c) for c in counts if c >= 0]
    return cases


def test_range_window_and_runs_against_brute_force(exe):
    cases = grid()
    r = subprocess.run([str(exe)], input="".join("%d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    n_kept = n_wrapped = n_end_at_wrap = n_start_at_wrap = n_full = n_empty_hist = 0
    for (vf, done, N, first, count), line in zip(cases, lines):
        head, _, rows = line.partition("|")
        t = [int(x) for x in head.split()]
        frames = kept_frames(vf, done, N)
        want_first = frames[0] if frames else done
        assert (t[0], t[1]) == (max(vf, done - N) if frames else t[0], len(frames)), (vf, done, N, line)
        if frames:
            assert t[0] == want_first
        else:
            assert t[1] == 0 and t[0] <= done
            n_empty_hist += 1
        kept = all(f in frames for f in range(first, first + count))
        assert t[2] == int(kept), (vf, done, N, first, count, line)
        if not (kept and count <= N):
            assert len(t) == 3
            continue
        n_kept += 1
        want_rows = [(first + j) % N for j in range(count)]
        assert [int(x) for x in rows.split()] == want_rows
        row0, n0, n1 = t[3:]
        assert n0 + n1 == count and 0 <= row0 < N and row0 + n0 <= N
        assert want_rows == list(range(row0, row0 + n0)) + list(range(n1))
        n_wrapped += n1 > 0
        n_end_at_wrap += count > 0 and n1 == 0 and row0 + n0 == N
        n_start_at_wrap += count > 0 and row0 == 0
        n_full += count == N
    print(f"history math: {len(cases)} cases, {n_kept} kept windows, {n_wrapped} cross the wrap, {n_end_at_wrap} end at it, {n_start_at_wrap} start at it, "
          f"{n_full} of N frames, {n_empty_hist} on an empty history")
    assert min(n_wrapped, n_end_at_wrap, n_start_at_wrap, n_full, n_empty_hist) > 0 and any(c[4] == 0 for c in cases)


def test_empty_history_after_create_reset_and_fork(exe):
    """create and reset: valid_from = 0 and nothing decoded; fork / restore: valid_from = done of the source.  Nothing is kept, every window
    with a frame is refused, and the fork's range then grows with its own frames only"""
    cases = [(0, 0, 64, 0, 1), (0, 0, 64, 0, 0), (150, 150, 64, 149, 1), (150, 150, 64, 150, 1), (150, 150, 64, 100, 50),
             (150, 170, 64, 150, 20), (150, 170, 64, 149, 21), (150, 300, 64, 236, 64), (150, 300, 64, 235, 64)]
    r = subprocess.run([str(exe)], input="".join("%d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [[int(x) for x in line.partition("|")[0].split()][:3] for line in r.stdout.splitlines()]
    assert got == [[0, 0, 0], [0, 0, 1], [150, 0, 0], [150, 0, 0], [150, 0, 0], [150, 20, 1], [150, 20, 0], [236, 64, 1], [236, 64, 0]]


def test_header_is_pure_code():
    src = (CSRC / "nasr_history.h").read_text()
    assert "hip_runtime" not in src and "hipMemcpy" not in src and "#include <stdint.h>" in src
