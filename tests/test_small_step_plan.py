"""The decode-graph budget and the fused family's lane cut (nemotron-asr.cpp_amd/csrc/nasr_step_plan.h: pipe_decode_iterations, fused_cut).
No GPU: the header is compiled with the host compiler under AddressSanitizer and UBSan into a stand-alone program, like
tests/test_step_plan.py.  Expected values come from the rules written here:

  * blind(frames) = 2 for one frame, else min(frames / 2 + 4, 16)         (the synchronous step graph's iterations)
  * an explicit cap:  max(blind(frames), min(10 frames + 1, cap))          (the formula before "auto" existed)
  * auto (cap 0):     3 for a one-frame step of the fused family (1 .. 4 rows), else the explicit formula at cap 12
"""
import shutil
import subprocess
from pathlib import Path

import pytest

from tests.test_gemm_plan import HIP_STUB

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"

# the built-in four-piece cut of the 24-layer model (profiles/small_step_decode.md)
CUT4_24 = [46, 98, 150]

DRIVER = r"""
#include "nasr_internal.h"
#include "nasr_step_plan.h"
#include <cstdio>
// one case per line of stdin, one answer per line of stdout:
//   I rows frames cap   -> pipe_decode_iterations blind_iterations
//   C L E               -> fused_cut(L, E, 0 .. E)
//   P packed L          -> valid_cut4 and the three unpacked indices
int main() {
    char op;
    while (scanf(" %c", &op) == 1) {
        if (op == 'I') {
            int rows, frames, cap;
            if (scanf("%d %d %d", &rows, &frames, &cap) != 3) return 2;
            printf("%d %d\n", nasr_step::pipe_decode_iterations(rows, frames, cap), nasr_step::blind_iterations(frames));
        } else if (op == 'C') {
            int L, E;
            if (scanf("%d %d", &L, &E) != 2) return 2;
            for (int k = 0; k <= E; k++) printf("%d ", nasr_step::fused_cut(L, E, k));
            printf("\n");
        } else if (op == 'P') {
            int packed, L, c[3];
            if (scanf("%d %d", &packed, &L) != 2) return 2;
            nasr_step::unpack_cut4(packed, c);
            printf("%d %d %d %d\n", nasr_step::valid_cut4(c, L) ? 1 : 0, c[0], c[1], c[2]);
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
    d = tmp_path_factory.mktemp("small_step_plan")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(HIP_STUB)
    (d / "drv.cpp").write_text(DRIVER)
    exe = d / "small_step_plan"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{d}", f"-I{CSRC}", f"-I{ROOT / 'include'}", str(d / "drv.cpp"), "-o", str(exe)])

    def run(cases):
        text = "".join(" ".join(str(v) for v in c) + "\n" for c in cases)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
        out = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return run


def blind(frames):
    return 2 if frames <= 1 else min(frames // 2 + 4, 16)


def explicit(frames, cap):
    return max(blind(frames), min(frames * 10 + 1, cap))


def test_decode_graph_budget(plan):
    AUTO = 0
    cases = [("I", rows, frames, cap) for rows in range(1, 9) for frames in range(1, 15) for cap in (AUTO, 1, 2, 12)]
    got = plan(cases)
    for (_, rows, frames, cap), (iters, bl) in zip(cases, got):
        assert bl == blind(frames)
        assert iters >= bl, (rows, frames, cap)
        if cap != AUTO:
            assert iters == explicit(frames, cap), (rows, frames, cap)
        elif frames == 1 and rows <= 4:
            assert iters == 3, (rows, frames)
        else:
            assert iters == explicit(frames, 12), (rows, frames)
    by = {c[1:]: g[0] for c, g in zip(cases, got)}
    assert by[(1, 1, 1)] == 2 and by[(1, 2, 1)] == 5          # what the fallback tests set: R = 0 and R = 1 at "decode_graph_iterations" = 1
    assert by[(1, 1, 12)] == 11 and by[(5, 1, AUTO)] == 11 and by[(4, 1, AUTO)] == 3
    # a step outside the fused family is passed as 0 rows: never the short graph
    assert plan([("I", 0, 1, AUTO), ("I", 0, 14, AUTO)]) == [[11, 2], [12, 11]]


def test_fused_cut(plan):
    cases = [("C", L, E) for L in (2, 4, 8, 24) for E in (1, 2, 3, 4)]
    for (_, L, E), b in zip(cases, plan(cases)):
        assert len(b) == E + 1 and b[0] == 0 and b[-1] == 8 * L, (L, E, b)
        assert all(hi > lo for lo, hi in zip(b, b[1:])), (L, E, b)          # strictly increasing: every piece has launches
    assert plan([("C", 24, 4)]) == [[0] + CUT4_24 + [192]]
    assert plan([("C", 24, 3)]) == [[0, 57, 126, 192]]                       # the three-piece cut is the one measured before


def test_fused_cuts_option_packing(plan):
    def pack(c):
        return c[0] | (c[1] << 10) | (c[2] << 20)
    got = plan([("P", pack([48, 104, 162]), 24), ("P", pack([48, 48, 162]), 24), ("P", pack([48, 104, 192]), 24), ("P", pack([0, 104, 162]), 24),
                ("P", pack([46, 98, 150]), 8), ("P", pack([1, 2, 3]), 8)])
    assert got == [[1, 48, 104, 162], [0, 48, 48, 162], [0, 48, 104, 192], [0, 0, 104, 162], [1, 46, 98, 150], [0, 1, 2, 3]]
