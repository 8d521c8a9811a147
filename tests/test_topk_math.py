"""nasr_topk.h (the selection arithmetic and the index maps of engine option "token_alternatives"), compiled with g++ under
AddressSanitizer / UBSan -- no GPU.
(a) the K largest packed keys of a row of 1025 logits, selected the way the kernels select them -- lane -> 16-entry tile -> row
    (k_dec_joint + k_dec_commit) and lane -> tile -> 64-entry workgroup -> row (k_dec_joint_tiled + k_dec_commit), only the first K
    keys of every slice reaching the row merge -- equal the K largest nasr_lp::pack_key values in descending order, computed in numpy
    from the key's definition, for K in {1, 4, 8}.
(b) ln P of every entry is within 5e-6 of float64 x[id] - logaddexp.reduce(x): the bound tests/test_logprob_math.py derives for the
    parts scheme (the entry's logit comes back from the key bit for bit, so only m + log s carries an error).
(c) every scratch slot (row, slice, k) of the rows in a row map is written exactly once by each kernel's grid."""
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
#include "nasr_topk.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace nasr_topk;
// topk <file> <K> : f32 rows of 1025 logits -> per row two lines (slices of 16, slices of 64): K x "key id lp"
// map <n_rows> <T> <K> : grids of both kernels over a row map of n_rows entries -> JSON counts
int main(int argc, char **argv) {
    if (!strcmp(argv[1], "topk")) {
        FILE *f = fopen(argv[2], "rb");
        const int K = atoi(argv[3]);
        if (!f || K < 1 || !valid_k(K)) return 2;
        std::vector<float> x(nasr_lp::LP_VOCAB);
        while (fread(x.data(), 4, nasr_lp::LP_VOCAB, f) == (size_t)nasr_lp::LP_VOCAB) {
            const int widths[2] = {nasr_lp::TILE_W, nasr_lp::WG_W};
            for (int w = 0; w < 2; w++) {
                const int np = nasr_lp::parts_of_width(widths[w]);
                std::vector<nasr_lp::Part> parts((size_t)np);
                nasr_lp::row_parts(x.data(), widths[w], parts.data());
                // the scratch of one row as the kernel leaves it: [slice][K], the first K keys of every slice's list
                std::vector<tkey> scratch(scratch_keys(1, K) , ~0ull);
                for (int s = 0; s < np; s++) {
                    tkey list[KMAX];
                    if (w == 0) tile_keys(x.data(), s, list); else wg_keys(x.data(), s, list);
                    for (int j = 0; j < K; j++) scratch[scratch_index(0, s, np, K) + (size_t)j] = list[j];
                }
                RowTop rt;
                row_begin(rt);
                row_merge(rt, K, scratch.data() + scratch_index(0, 0, np, K), np);
                float m, log_s;
                row_softmax(parts.data(), np, &m, &log_s);
                for (int j = 0; j < K; j++) printf("%llu %d %.9g ", rt.top[j], alt_id(rt.top[j]), (double)alt_lp(rt.top[j], m, log_s));
                // the token's own value is the same function of the same (m, log s) as nasr_lp::finish
                printf("%u %u\n", nasr_lp::f32_bits(lp_of(nasr_lp::key_logit(rt.top[0]), m, log_s)),
                       nasr_lp::f32_bits(nasr_lp::finish(nasr_lp::key_logit(rt.top[0]), parts.data(), np)));
            }
        }
        fclose(f);
        return 0;
    }
    if (!strcmp(argv[1], "map")) {
        const int nr = atoi(argv[2]), T = atoi(argv[3]), K = atoi(argv[4]);
        std::vector<unsigned> rowmap((size_t)nr);
        for (int i = 0; i < nr; i++) rowmap[(size_t)i] = ((unsigned)(i % T) << 16) | (unsigned)(i / T);
        const int B = (nr + T - 1) / T;
        int bad = 0;
        for (int kernel = 0; kernel < 2; kernel++) {
            const int np = kernel == 0 ? nasr_lp::TILE_PARTS : nasr_lp::WG_PARTS;
            std::vector<int> seen((size_t)B * T * np * K, 0);       // ASan guards the bounds of every index the maps produce
            auto store = [&](int row, int slice) {                  // what a writer thread does with its list
                const size_t at = scratch_index(nasr_lp::key_index(rowmap[(size_t)row], T), slice, np, K);
                for (int j = 0; j < KMAX; j++) if (j < K) seen[at + (size_t)j]++;
            };
            if (kernel == 0) {
                for (int nt = 0; nt < nasr_lp::TILE_PARTS; nt++)
                    for (int i0 = 0; i0 < nr; i0 += 64) {
                        const int mt = nasr_lp::joint_pass_tiles(nr - i0);
                        for (int th = 0; th < 256; th++) {
                            const int row = nasr_lp::joint_store_row(i0, mt, th >> 6, th & 63, nr);
                            if (row >= 0) store(row, nt);
                        }
                    }
            } else {
                for (int bx = 0; bx < nasr_lp::WG_PARTS; bx++)
                    for (int by = 0; by < (B * T + 63) / 64; by++)
                        for (int th = 0; th < 256; th++) {
                            const int row = nasr_lp::tiled_store_row(by, th, nr);
                            if (row >= 0) store(row, bx);
                        }
            }
            for (int i = 0; i < nr; i++)
                for (int p = 0; p < np; p++)
                    for (int j = 0; j < K; j++) {
                        int &c = seen[scratch_index(nasr_lp::key_index(rowmap[(size_t)i], T), p, np, K) + (size_t)j];
                        if (c != 1) bad++;
                        c = 0;
                    }
            for (int c : seen) if (c != 0) bad++;               // nothing outside the rows of the map
        }
        printf("{\"bad\": %d, \"scratch\": %zu, \"ring_last\": %zu}\n", bad, scratch_keys(nr, K), ring_index(2, 4096 + 5, 4096, K));
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
    d = tmp_path_factory.mktemp("topk")
    (d / "drv.cpp").write_text(DRIVER)
    out = d / "topk"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{CSRC}", str(d / "drv.cpp"), "-o", str(out)])
    return out, d


def pack_keys(rows):
    """nasr_lp::pack_key of every entry: (order-preserving image of the f32 bits) << 32 | (0xffffffff - id)"""
    bits = np.ascontiguousarray(rows, np.float32).view(np.uint32)
    u = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint64)
    ids = np.arange(rows.shape[1], dtype=np.uint64)
    return (u << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - ids)[None, :]


def make_rows():
    rng = np.random.default_rng(1025)
    rows = [(rng.standard_normal((24, V)) * s).astype(np.float32) for s in (0.1, 1.0, 4.0)]
    rows = np.concatenate(rows)
    special = np.zeros((10, V), np.float32)
    special[0] = 3.25                                                  # all equal: ids 0 .. K - 1
    special[1] = np.round(rng.standard_normal(V) * 1.5)                # many exactly equal values (about ten distinct levels)
    special[2] = np.round(rng.standard_normal(V))                      # ... fewer levels still: the top level holds far more than 8
    special[3] = rng.standard_normal(V); special[3, 1024] = 9.0        # the maximum at id 1024, alone in its slice
    special[4] = rng.standard_normal(V) - 5.0
    special[4, 592:608] = np.linspace(4.0, 7.0, 16)                    # every top entry in ONE 16-entry tile (tile 37)
    special[5] = rng.standard_normal(V) - 5.0
    special[5, 592:608] = 6.0                                          # ... and all equal there
    special[6] = -np.abs(rng.standard_normal(V)) - 1.0                 # all negative, -0.0 and +0.0 among them
    special[6, 300] = -0.0; special[6, 7] = 0.0
    special[7] = -1e4; special[7, [0, 1023, 1024]] = [-9990.0, -9990.0, -9990.0]      # ties across the first and the last slices
    special[8] = rng.standard_normal(V); special[8, 1020:1025] = [5, 5, 5, 5, 5]      # a tie that straddles the last full tile and entry 1024
    special[9] = np.float32(1e-40)                                     # subnormals
    special[9, 64] = np.float32(2e-40)
    return np.concatenate([rows, special])


def run_topk(exe, rows, K):
    prog, d = exe
    path = d / "rows.f32"
    np.ascontiguousarray(rows, np.float32).tofile(path)
    r = subprocess.run([str(prog), "topk", str(path), str(K)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert len(lines) == 2 * rows.shape[0]
    keys = np.array([[int(t) for t in ln[0:3 * K:3]] for ln in lines], np.uint64).reshape(rows.shape[0], 2, K)
    ids = np.array([[int(t) for t in ln[1:3 * K:3]] for ln in lines], np.int64).reshape(rows.shape[0], 2, K)
    lps = np.array([[float(t) for t in ln[2:3 * K:3]] for ln in lines], np.float64).reshape(rows.shape[0], 2, K)
    tail = np.array([[int(ln[3 * K]), int(ln[3 * K + 1])] for ln in lines], np.uint64).reshape(rows.shape[0], 2, 2)
    return keys, ids, lps, tail


BOUND = 5e-6


@pytest.mark.parametrize("K", [1, 4, 8])
def test_selection_through_both_merge_paths_equals_the_sorted_keys(exe, K):
    rows = make_rows()
    keys, ids, lps, tail = run_topk(exe, rows, K)
    want = np.sort(pack_keys(rows), axis=1)[:, ::-1][:, :K]
    assert (keys[:, 0, :] == want).all(), "lane -> tile -> row"
    assert (keys[:, 1, :] == want).all(), "lane -> tile -> workgroup -> row"
    want_ids = (np.uint64(0xFFFFFFFF) - (want & np.uint64(0xFFFFFFFF))).astype(np.int64)
    assert (ids[:, 0, :] == want_ids).all() and (ids[:, 1, :] == want_ids).all()
    # descending logit, the lower id first among equal logit bits; entry 0 is numpy's arg-max (its first maximum)
    assert (want_ids[:, 0] == rows.argmax(axis=1)).all()
    lg = np.take_along_axis(rows, want_ids, axis=1)
    assert (np.diff(lg, axis=1) <= 0).all()
    eq = np.diff(lg.view(np.uint32).astype(np.int64), axis=1) == 0
    assert (np.diff(want_ids, axis=1)[eq] > 0).all()
    n = rows.shape[0] - 10
    assert want_ids[n + 0].tolist() == list(range(K))
    assert want_ids[n + 3, 0] == 1024
    assert set(want_ids[n + 4].tolist()) <= set(range(592, 608)) and want_ids[n + 5].tolist() == list(range(592, 592 + K))
    assert want_ids[n + 7].tolist() == [0, 1023, 1024, 1, 2, 3, 4, 5][:K]
    assert want_ids[n + 8].tolist() == [1020, 1021, 1022, 1023, 1024][:K] + want_ids[n + 8].tolist()[5:]
    # (b) the values
    x = rows.astype(np.float64)
    ref = np.take_along_axis(x, want_ids, axis=1) - np.logaddexp.reduce(x, axis=1)[:, None]
    err = np.abs(lps - ref[:, None, :]).max(axis=(0, 2))
    print(f"K={K}: max |ln P - float64| per slice width (16, 64) = {err}")
    assert (err < BOUND).all(), err
    assert np.isfinite(lps).all() and (lps <= 0).all()
    assert (np.diff(lps, axis=2) <= 0).all()                          # same (m, log s) for the whole row: the order of the logits
    assert (np.exp(lps).sum(axis=2) <= 1 + 1e-5).all()
    assert (tail[:, :, 0] == tail[:, :, 1]).all(), "lp_of(m, log s) and nasr_lp::finish give the same bits"


def test_k4_is_a_prefix_of_k8(exe):
    rows = make_rows()
    k4 = run_topk(exe, rows, 4)
    k8 = run_topk(exe, rows, 8)
    assert (k4[0] == k8[0][:, :, :4]).all() and (k4[2] == k8[2][:, :, :4]).all()


@pytest.mark.parametrize("n_rows", [1, 14, 64, 65, 896])
@pytest.mark.parametrize("K", [1, 4, 8])
def test_every_scratch_slot_is_written_once(exe, n_rows, K):
    prog, _ = exe
    for T in (1, 14):
        r = subprocess.run([str(prog), "map", str(n_rows), str(T), str(K)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, r.stderr
        got = json.loads(r.stdout)
        assert got["bad"] == 0
        assert got["scratch"] >= max(64 * 65, n_rows * 17) * K
        assert got["ring_last"] == (2 * 4096 + 5) * K
