"""nasr_lp::blank_lp (nasr_logprob.h, engine option "frame_blank_logprobs"), compiled with g++ under AddressSanitizer / UBSan into a
stand-alone program -- no GPU.
(a) blank_lp (f64 arithmetic over the kernels' f32 parts; the ring keeps its nearest f32) over the parts of a row, in both layouts (65 parts of 16 entries as k_dec_joint writes them, 17 parts of 64 as
    k_dec_joint_tiled does), is within 2e-6 of x[1024] - logsumexp(x) taken in float64;
(b) the last part's m has the bits of logits[1024]: blank is alone in it, for both widths."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"
V = 1025
BOUND = 2e-6

DRIVER = r"""
#include "nasr_logprob.h"
#include <cstdio>
#include <vector>
using namespace nasr_lp;
// <file> : f32 rows of 1025 logits -> per row "blank_lp16 blank_lp64 last_m16_bits last_m64_bits logit1024_bits"
int main(int argc, char **argv) {
    if (argc < 2) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<float> x(LP_VOCAB);
    while (fread(x.data(), 4, LP_VOCAB, f) == (size_t)LP_VOCAB) {
        double lp[2];
        unsigned mb[2];
        const int widths[2] = {TILE_W, WG_W};
        for (int w = 0; w < 2; w++) {
            std::vector<Part> parts((size_t)parts_of_width(widths[w]));      // exactly n parts: ASan guards parts[n - 1]
            row_parts(x.data(), widths[w], parts.data());
            lp[w] = blank_lp(parts.data(), (int)parts.size());
            mb[w] = f32_bits(parts.back().m);
        }
        printf("%.17g %.17g %u %u %u\n", lp[0], lp[1], mb[0], mb[1], f32_bits(x[LP_VOCAB - 1]));
    }
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("fb")
    (d / "drv.cpp").write_text(DRIVER)
    out = d / "fb"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{CSRC}", str(d / "drv.cpp"), "-o", str(out)])
    return out, d


def run_rows(exe, rows):
    prog, d = exe
    rows = np.ascontiguousarray(rows, np.float32)
    assert rows.shape[1] == V
    path = d / "rows.f32"
    rows.tofile(path)
    r = subprocess.run([str(prog), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr
    out = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert len(out) == rows.shape[0]
    lp = np.array([[float(o[0]), float(o[1])] for o in out])
    bits = np.array([[int(o[2]), int(o[3]), int(o[4])] for o in out], np.uint64)
    return lp, bits


def reference(rows):
    x = rows.astype(np.float64)
    return x[:, V - 1] - np.logaddexp.reduce(x, axis=1)


def check(rows, lp, bits):
    ref = reference(rows)
    err = np.abs(lp - ref[:, None]).max(axis=0)
    print(f"max |blank_lp - ref| per part width (16, 64) = {err}")
    assert (err < BOUND).all(), err
    assert (lp <= 0).all() and np.isfinite(lp).all()
    want = np.ascontiguousarray(rows[:, V - 1], np.float32).view(np.uint32)
    assert (bits[:, 0] == want).all() and (bits[:, 1] == want).all() and (bits[:, 2] == want).all()


@pytest.mark.parametrize("s", [0.1, 3.0, 30.0])
def test_blank_lp_matches_float64_and_last_part_is_blank(exe, s):
    rng = np.random.default_rng(int(s * 10) + 1)
    rows = (rng.standard_normal((200, V)) * s).astype(np.float32)
    for i in range(0, 200, 4):                                   # blank wins on a quarter of the rows, as on most frames of a stream
        rows[i, V - 1] = rows[i].max() + np.float32(2 * s)
    lp, bits = run_rows(exe, rows)
    check(rows, lp, bits)


def test_special_rows(exe):
    rows = np.zeros((6, V), np.float32)
    rows[0, :] = 3.25                                   # all equal: lp = -log 1025
    rows[1, :] = -40.0; rows[1, 517] = 30.0             # one dominant logit elsewhere: lp(blank) = -70
    rows[2, :] = -5.0; rows[2, 1024] = 2.0              # the 1025th entry, alone in its tile, wins
    rows[3, :] = 1.0; rows[3, 1024] = -60.0             # ... or is negligible
    rows[4, :] = -1e4; rows[4, 0] = -9990.0             # large negative logits: nothing underflows to log(0)
    rows[5, :] = 80.0; rows[5, 1000] = 88.0             # large positive ones: nothing overflows
    lp, bits = run_rows(exe, rows)
    check(rows, lp, bits)
    assert np.abs(lp[0] + np.log(1025.0)).max() < BOUND
    assert np.abs(lp[1] + 70.0).max() < 1e-5
