"""nasr_logprob.h (the arithmetic and the index maps of engine option "token_logprobs"), compiled with g++ under
AddressSanitizer / UBSan -- no GPU.
(a) the parts of a row (per 16-entry tile as k_dec_joint writes them, per 64-entry workgroup as k_dec_joint_tiled does) merged
    in ascending part index give log-sum-exp over the 1025 logits within 5e-6 of numpy.logaddexp.reduce in float64.  The bound
    is the f32 rounding of this scheme: about 70 adds of terms <= 1 at 6e-8 relative each, one exp / log pair, and the final
    m + log(s) at |lse| <= 16 (ulp 1e-6); an f32 restatement in numpy stays within 1.2e-6 for the distributions below.
(b) the arg-max key's high word gives back the winning logit bit for bit.
(c) every (row, part) slot of the rows in the row map is written exactly once by each kernel's grid."""
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"
V = 1025

DRIVER = r"""
#include "nasr_logprob.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace nasr_lp;
// lse <file> : f32 rows of 1025 logits -> per row "lse16 lse64 lp16 lp64 argmax key_logit_bits logit_bits"
// map <n_rows> <T> : grids of both kernels over a row map of n_rows entries -> JSON counts
int main(int argc, char **argv) {
    if (!strcmp(argv[1], "lse")) {
        FILE *f = fopen(argv[2], "rb");
        if (!f) return 2;
        std::vector<float> x(LP_VOCAB);
        while (fread(x.data(), 4, LP_VOCAB, f) == (size_t)LP_VOCAB) {
            unsigned long long best = 0;
            for (int v = 0; v < LP_VOCAB; v++) { const unsigned long long k = pack_key(x[v], v); if (k > best) best = k; }
            const int tok = key_index_of(best);
            const float lg = key_logit(best);
            float lp[2];
            const int widths[2] = {TILE_W, WG_W};
            for (int w = 0; w < 2; w++) {
                std::vector<Part> parts((size_t)parts_of_width(widths[w]));
                row_parts(x.data(), widths[w], parts.data());
                lp[w] = finish(lg, parts.data(), (int)parts.size());
            }
            printf("%.9g %.9g %d %u %u\n", (double)lp[0], (double)lp[1], tok, f32_bits(lg), f32_bits(x[tok]));
        }
        fclose(f);
        return 0;
    }
    if (!strcmp(argv[1], "map")) {
        const int nr = atoi(argv[2]), T = atoi(argv[3]);
        // row map: row i = (frame i % T of batch row i / T), as build_lists would produce for streams with all T frames left
        std::vector<unsigned> rowmap((size_t)nr);
        for (int i = 0; i < nr; i++) rowmap[(size_t)i] = ((unsigned)(i % T) << 16) | (unsigned)(i / T);
        const int B = (nr + T - 1) / T;
        int bad = 0;
        for (int kernel = 0; kernel < 2; kernel++) {
            const int np = kernel == 0 ? TILE_PARTS : WG_PARTS;
            std::vector<int> seen((size_t)B * T * np, 0);       // ASan guards the bounds of every index the maps produce
            if (kernel == 0) {
                for (int nt = 0; nt < TILE_PARTS; nt++)
                    for (int i0 = 0; i0 < nr; i0 += 64) {
                        const int mt = joint_pass_tiles(nr - i0);
                        for (int th = 0; th < 256; th++) {
                            const int row = joint_store_row(i0, mt, th >> 6, th & 63, nr);
                            if (row >= 0) seen[scratch_index(key_index(rowmap[(size_t)row], T), nt, np)]++;
                        }
                    }
            } else {
                for (int bx = 0; bx < WG_PARTS; bx++)
                    for (int by = 0; by < (B * T + 63) / 64; by++)
                        for (int th = 0; th < 256; th++) {
                            const int row = tiled_store_row(by, th, nr);
                            if (row >= 0) seen[scratch_index(key_index(rowmap[(size_t)row], T), bx, np)]++;
                        }
            }
            for (int i = 0; i < nr; i++)
                for (int p = 0; p < np; p++) {
                    const int c = seen[scratch_index(key_index(rowmap[(size_t)i], T), p, np)];
                    if (c != 1) bad++;
                    seen[scratch_index(key_index(rowmap[(size_t)i], T), p, np)] = 0;
                }
            for (int c : seen) if (c != 0) bad++;               // nothing outside the rows of the map
        }
        printf("{\"bad\": %d, \"n_parts_small\": %d, \"n_parts_large\": %d, \"scratch\": %zu}\n", bad, n_parts(64), n_parts(65), scratch_parts(nr));
        return 0;
    }
    return 1;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("lp")
    (d / "drv.cpp").write_text(DRIVER)
    out = d / "lp"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{CSRC}", str(d / "drv.cpp"), "-o", str(out)])
    return out, d


def run_lse(exe, rows):
    prog, d = exe
    rows = np.ascontiguousarray(rows, np.float32)
    assert rows.shape[1] == V
    path = d / "rows.f32"
    rows.tofile(path)
    r = subprocess.run([str(prog), "lse", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr
    out = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert len(out) == rows.shape[0]
    lp = np.array([[float(a), float(b)] for a, b, *_ in out])
    tok = np.array([int(o[2]) for o in out])
    bits = np.array([[int(o[3]), int(o[4])] for o in out], np.uint64)
    return lp, tok, bits


def reference_lp(rows):
    x = rows.astype(np.float64)
    return x.max(axis=1) - np.logaddexp.reduce(x, axis=1)


BOUND = 5e-6


@pytest.mark.parametrize("s", [0.1, 1.0, 4.0])
def test_parts_and_ordered_merge_match_float64(exe, s):
    rng = np.random.default_rng(int(s * 10))
    rows = (rng.standard_normal((200, V)) * s).astype(np.float32)
    for i in range(0, 200, 4):
        rows[i, rng.integers(0, V)] += np.float32(8 * s)
    lp, tok, _ = run_lse(exe, rows)
    assert (tok == rows.argmax(axis=1)).all()
    ref = reference_lp(rows)
    err = np.abs(lp - ref[:, None]).max(axis=0)
    print(f"s={s}: max |lp - ref| per part width (16, 64) = {err}")
    assert (err < BOUND).all(), err
    assert (lp <= 0).all() and (lp >= -np.log(V) - 1e-5).all()


def test_special_rows(exe):
    rows = np.zeros((6, V), np.float32)
    rows[0, :] = 3.25                                   # all equal: lse = 3.25 + log 1025, the first index wins
    rows[1, :] = -40.0; rows[1, 517] = 30.0             # one dominant logit: lp = 0
    rows[2, :] = -5.0; rows[2, 1024] = 2.0              # the 1025th entry, alone in its tile, wins
    rows[3, :] = 1.0; rows[3, 1024] = -60.0             # ... or is negligible
    rows[4, :] = -1e4; rows[4, 0] = -9990.0             # large negative logits: nothing underflows to log(0)
    rows[5, :] = 80.0; rows[5, 1000] = 88.0             # large positive ones: nothing overflows
    lp, tok, _ = run_lse(exe, rows)
    ref = reference_lp(rows)
    assert tok.tolist() == [0, 517, 1024, 0, 0, 1000]
    assert np.isfinite(lp).all()
    assert np.abs(lp[0] + np.log(1025.0)).max() < BOUND
    assert (lp[1] == 0.0).all()
    assert np.abs(lp - ref[:, None]).max() < BOUND
    assert (lp <= 0).all()


def test_key_gives_back_the_winning_logit_bit_for_bit(exe):
    rng = np.random.default_rng(7)
    rows = -np.abs(rng.standard_normal((8, V))).astype(np.float32) - 1.0      # all negative
    rows[1, 300] = -0.0                                                       # the winner is -0.0
    rows[2, 5] = 0.0
    rows[3, :] = -np.float32(1e-40)                                           # subnormals
    rows[4, 77] = np.float32(3.4e38)
    rows[5, :] = np.float32(-3.0e38); rows[5, 1024] = np.float32(-2.9e38)
    lp, tok, bits = run_lse(exe, rows)
    assert (bits[:, 0] == bits[:, 1]).all()
    want = rows[np.arange(8), rows.argmax(axis=1)].view(np.uint32)
    assert (bits[:, 0] == want).all()
    assert bits[1, 0] == 0x80000000 and tok[1] == 300
    assert tok[3] == 0                                                        # ties: the first index


@pytest.mark.parametrize("n_rows", [1, 16, 17, 64, 65, 896, 7168])
@pytest.mark.parametrize("T", [1, 14])
def test_every_row_part_slot_is_written_once(exe, n_rows, T):
    prog, _ = exe
    r = subprocess.run([str(prog), "map", str(n_rows), str(T)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr
    got = json.loads(r.stdout)
    assert got["bad"] == 0
    assert got["n_parts_small"] == 65 and got["n_parts_large"] == 17
    assert got["scratch"] >= max(64 * 65, n_rows * 17)
