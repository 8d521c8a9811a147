"""nasr_align.h (the recursions, the tie rule, the backtrace and the index maps of forced alignment) and host/align_words.h, compiled
with g++ under AddressSanitizer / UBSan -- no GPU.
(a) on random lb / ly lattices (T = 1, U = 0, U > T and exact ties built on purpose among them) loglik and best equal a numpy float64
    recursion with the same tie rule (tests/align_ref.py) to 1e-12 * (T + U); the frames are exact.
(b) for every cell of lattices around the tile edges and for align_cells in {64, 200, default}: each cell is owned by exactly one
    (launch, tile, thread) and no thread maps outside the lattice arrays.
(c) aligned tokens -> word rows."""
import json
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import align_ref as ar

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"
HOST = ROOT / "nemotron-asr.cpp_amd" / "host"

DRIVER = r"""
#include "nasr_align.h"
#include "align_words.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace nasr_align;
// lat <file> : records (int32 T, U; f32 lb[T][U+1]; f32 ly[T][U+1]) -> per record "loglik best f0 f1 .. | lp bits .."
// map <align_cells> T U [T U ..] : the launches of a sub-batch of these lattices -> JSON counts
// words <file> : lines "V piece" (vocabulary, in id order) and "T id frame lp" -> one row per word
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    if (!strcmp(argv[1], "lat")) {
        FILE *f = fopen(argv[2], "rb");
        if (!f) return 2;
        int32_t hd[2];
        while (fread(hd, 4, 2, f) == 2) {
            const int T = hd[0], U = hd[1];
            const size_t n = (size_t)n_cells(T, U);
            std::vector<float> lb(n), ly(n);
            if (fread(lb.data(), 4, n, f) != n || fread(ly.data(), 4, n, f) != n) return 3;
            std::vector<unsigned char> bp(n);
            std::vector<int32_t> frames((size_t)U);
            std::vector<float> lps((size_t)U);
            double loglik, best;
            run_lattice(lb.data(), ly.data(), T, U, &loglik, &best, bp.data(), frames.data(), lps.data());
            printf("%.17g %.17g", loglik, best);
            for (int i = 0; i < U; i++) printf(" %d", frames[(size_t)i]);
            printf(" |");
            for (int i = 0; i < U; i++) printf(" %u", nasr_lp::f32_bits(lps[(size_t)i]));
            printf("\n");
        }
        fclose(f);
        return 0;
    }
    if (!strcmp(argv[1], "map")) {
        const long long align_cells = atoll(argv[2]);
        std::vector<Utt> ud;
        long long cells = 0;
        int g = 0, tk = 0;
        for (int i = 3; i + 1 < argc; i += 2) {
            Utt u;
            u.enc_row = 0; u.g_row = g; u.T = atoi(argv[i]); u.U = atoi(argv[i + 1]); u.cell0 = cells; u.tok0 = tk; u.pad = 0;
            cells += n_cells(u.T, u.U); g += u.U + 1; tk += u.U;
            ud.push_back(u);
        }
        std::vector<Tile> tiles;
        std::vector<int> first;
        plan_launches(ud.data(), (int)ud.size(), align_cells, tiles, first);
        std::vector<int> seen((size_t)cells, 0);                  // ASan guards the bounds of every index the maps produce
        int bad = 0;
        long long max_launch = 0, multi_tile_over = 0;
        for (size_t l = 0; l + 1 < first.size(); l++) {
            long long in_launch = 0;
            if (first[l + 1] <= first[l]) bad++;
            for (int j = first[l]; j < first[l + 1]; j++) {
                const Tile td = tiles[(size_t)j];
                const Utt &u = ud[(size_t)td.utt];
                int n = 0;
                for (int th = 0; th < 256; th++) {
                    int t = -1, uu = -1;
                    const long long c = store_cell(u, td, th, &t, &uu);
                    if (c < 0) continue;
                    if (c != u.cell0 + cell_index(u.U, t, uu) || t < td.t0 || t >= td.t0 + TILE_T || uu < td.u0 || uu >= td.u0 + TILE_U) bad++;
                    seen[(size_t)c]++;
                    n++;
                }
                if (n != tile_cells(u.T, u.U, td.t0, td.u0) || n == 0) bad++;
                in_launch += n;
            }
            if (in_launch > max_launch) max_launch = in_launch;
            if (in_launch > align_cells && first[l + 1] - first[l] > 1) multi_tile_over++;
        }
        for (int c : seen) if (c != 1) bad++;
        printf("{\"bad\": %d, \"cells\": %lld, \"launches\": %zu, \"tiles\": %zu, \"max_launch\": %lld, \"multi_tile_over\": %lld}\n", bad, cells,
               first.size() - 1, tiles.size(), max_launch, multi_tile_over);
        return 0;
    }
    if (!strcmp(argv[1], "words")) {
        FILE *f = fopen(argv[2], "r");
        if (!f) return 2;
        std::vector<std::string> vocab;
        std::vector<int> tokens, frames;
        std::vector<float> lps;
        char kind, buf[256];
        while (fscanf(f, " %c", &kind) == 1) {
            if (kind == 'V') { if (fscanf(f, " %255s", buf) != 1) return 3; vocab.push_back(buf); }
            else { int id, fr; float lp; if (fscanf(f, " %d %d %f", &id, &fr, &lp) != 3) return 3; tokens.push_back(id); frames.push_back(fr); lps.push_back(lp); }
        }
        fclose(f);
        for (const align_words::Row &r : align_words::rows(tokens, frames, lps, vocab)) printf("%.4f %.4f %.6f %s\n", r.start_s, r.end_s, (double)r.confidence, r.word.c_str());
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
    d = tmp_path_factory.mktemp("align")
    (d / "drv.cpp").write_text(DRIVER)
    out = d / "align"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{CSRC}", f"-I{HOST}", str(d / "drv.cpp"), "-o", str(out)])
    return out, d


def make_lattices():
    rng = np.random.default_rng(2025)
    out = []
    for T, U in [(1, 0), (1, 1), (1, 7), (2, 0), (7, 0), (3, 9), (5, 5), (13, 16), (40, 7), (40, 33), (17, 8), (16, 7), (64, 60)]:
        out.append((-rng.random((T, U + 1)) * 8, -rng.random((T, U + 1)) * 8))
    # exact ties on purpose: every cell the same value (every path ties), and small integers (many equal path scores)
    out.append((np.full((6, 5), -1.0), np.full((6, 5), -1.0)))
    out.append((np.full((4, 9), -0.5), np.full((4, 9), -0.5)))
    for T, U in [(9, 6), (12, 12), (5, 11)]:
        out.append((-rng.integers(0, 3, (T, U + 1)).astype(np.float64), -rng.integers(0, 3, (T, U + 1)).astype(np.float64)))
    return [(lb.astype(np.float32), ly.astype(np.float32)) for lb, ly in out]


def test_recursions_equal_the_numpy_float64_recursion(exe):
    prog, d = exe
    lats = make_lattices()
    path = d / "lat.bin"
    with open(path, "wb") as f:
        for lb, ly in lats:
            f.write(struct.pack("<ii", lb.shape[0], lb.shape[1] - 1))
            f.write(lb.tobytes())
            f.write(ly.tobytes())
    r = subprocess.run([str(prog), "lat", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(lats)
    n_tie_cases = 0
    for (lb, ly), line in zip(lats, lines):
        T, U = lb.shape[0], lb.shape[1] - 1
        head, tail = line.split("|")
        vals = head.split()
        ref = ar.recursions(lb, ly)
        tol = 1e-12 * (T + U)
        assert abs(float(vals[0]) - ref["loglik"]) <= tol and abs(float(vals[1]) - ref["best"]) <= tol, (T, U)
        frames = [int(x) for x in vals[2:]]
        assert frames == ref["frames"], (T, U)
        assert float(vals[0]) >= float(vals[1])
        bits = [int(x) for x in tail.split()]
        assert bits == [int(ly[f, i].view(np.uint32)) for i, f in enumerate(frames)]
        assert abs(ar.path_score(lb.astype(np.float64), ly.astype(np.float64), frames) - ref["best"]) <= tol
        n_tie_cases += ref["margin"] == 0.0
    assert n_tie_cases >= 3                                            # the tie rule was exercised
    # all cells equal: a token move never beats the blank move into a cell, so the best path enters every cell from above and the
    # backtrace reaches frame 0 before it takes a token: all tokens are emitted there
    lb, ly = lats[13]
    assert [int(x) for x in lines[13].split("|")[0].split()[2:]] == [0] * (lb.shape[1] - 1)


EDGE = [(1, 0), (1, 7), (1, 8), (15, 6), (16, 7), (17, 8), (16, 15), (32, 16), (33, 17), (5, 1024), (40, 33)]


@pytest.mark.parametrize("cells", [64, 200, 1 << 20])
def test_every_cell_has_one_owner(exe, cells):
    prog, _ = exe
    batches = [[tu] for tu in EDGE] + [EDGE, [(1, 0)] * 70]
    for batch in batches:
        args = [str(x) for tu in batch for x in tu]
        r = subprocess.run([str(prog), "map", str(cells)] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, r.stderr
        got = json.loads(r.stdout)
        assert got["bad"] == 0, (batch, got)
        assert got["cells"] == sum(T * (U + 1) for T, U in batch)
        assert got["multi_tile_over"] == 0 and got["max_launch"] <= max(cells, 128)
        if cells == 1 << 20:
            assert got["launches"] == 1
        elif got["cells"] > 2 * max(cells, 128):
            assert got["launches"] >= got["cells"] // max(cells, 128)
    # 70 one-cell lattices: a launch of 64 cells holds 64 of them
    r = subprocess.run([str(prog), "map", "64"] + ["1", "0"] * 70, capture_output=True, text=True, timeout=120)
    assert json.loads(r.stdout)["launches"] == 2


def test_word_rows(exe):
    prog, d = exe
    vocab = ["▁he", "llo", "▁wor", "ld", "▁a", "x"]
    toks = [(5, 0, -0.1), (0, 2, -0.5), (1, 2, -0.25), (99, 3, -9.0), (2, 7, -1.0), (3, 9, -0.125), (4, 9, -2.0)]
    path = d / "words.txt"
    path.write_text("".join(f"V {p}\n" for p in vocab) + "".join(f"T {i} {f} {lp}\n" for i, f, lp in toks), encoding="utf-8")
    r = subprocess.run([str(prog), "words", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr
    rows = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert [row[3] for row in rows] == ["x", "hello", "world", "a"]
    want = [(0, 0, -0.1), (2, 2, -0.5), (7, 9, -1.0), (9, 9, -2.0)]        # first frame, last frame, min ln P (id 99 is outside the vocabulary)
    for row, (f0, f1, lp) in zip(rows, want):
        assert float(row[0]) == pytest.approx(f0 * 0.08, abs=1e-4) and float(row[1]) == pytest.approx((f1 + 1) * 0.08, abs=1e-4)
        assert float(row[2]) == pytest.approx(np.exp(lp), abs=1e-5)
    # tokens without a frame (an utterance with no encoder frame): no times, never negative ones
    path.write_text("".join(f"V {p}\n" for p in vocab) + "T 0 -1 -1.5\nT 1 -1 -0.5\n", encoding="utf-8")
    r = subprocess.run([str(prog), "words", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr
    row = r.stdout.split()
    assert float(row[0]) == float(row[1]) == -1.0 and row[3] == "hello"
