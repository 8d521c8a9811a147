"""nasr_beam.h (ordering and ties, insertion into C with merge and keep-W, selection of A from D, the prune, the trie, the backtrace and the
node bound of the beam search), compiled with g++ under AddressSanitizer / UBSan into a stand-alone driver -- no GPU.  The driver and
tests/beam_ref.py run the same synthetic table models: logits[t][state(y)][1025] with state(y) a fold of the sequence into NS classes.  The
driver is handed, per (t, state), what the joint kernels leave per row -- ln P(blank), the 8 largest packed keys (nasr_lp::pack_key) and the
softmax (m, log s) -- and turns them into expansion lists with nasr_beam::expand; the reference gets the same f32 values ((logit - m) - log s
in float32), so scores agree to 1e-12 * (T + U); tokens and frames are exact, results with the prune on and off are
identical, the trie never outgrows T * S * W nodes, and after every round the host search checks that each child's decoder slot lies in
0 .. 3 W - 1 and is held by no entry of C, no parent and no other child."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import beam_ref as br

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"
BLANK, V = 1024, 1025

DRIVER = r"""
#include "nasr_beam.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace nasr_beam;
// <file> <prune>: int32 T, W, N, S, NS; then per (t, state): f32 lb, u64 key[8], f32 m, f32 log_s -> "nodes bound", then one line per hypothesis
// expand <W> key .. : the expansion list of one row with m = log_s = 0 -> "id:lpbits .."
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    if (!strcmp(argv[1], "expand")) {
        nasr_topk::tkey top[KTOP] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 3; i < argc && i - 3 < KTOP; i++) top[i - 3] = strtoull(argv[i], nullptr, 10);
        int32_t tok[KTOP];
        float lp[KTOP];
        const int n = expand(top, atoi(argv[2]), 0.0f, 0.0f, tok, lp);
        for (int i = 0; i < n; i++) printf("%d:%u ", tok[i], nasr_lp::f32_bits(lp[i]));
        printf("\n");
        return 0;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[5];
    if (fread(hd, 4, 5, f) != 5) return 3;
    const int T = hd[0], W = hd[1], N = hd[2], S = hd[3], NS = hd[4];
    if (!valid_params(W, N, S)) return 4;
    struct Row { float lb; nasr_topk::tkey key[KTOP]; float m, log_s; };
    std::vector<Row> rows((size_t)T * NS);
    for (Row &r : rows)
        if (fread(&r.lb, 4, 1, f) != 1 || fread(r.key, 8, KTOP, f) != (size_t)KTOP || fread(&r.m, 4, 1, f) != 1 || fread(&r.log_s, 4, 1, f) != 1) return 3;
    fclose(f);
    std::vector<Result> out;
    const long long nodes = search(T, W, N, S, atoi(argv[2]) != 0, [&](int t, const int32_t *seq, int len, float *lb, nasr_topk::tkey *top, float *m, float *log_s) {
        long long s = 0;
        for (int i = 0; i < len; i++) s = (s * 31 + seq[i] + 1) % NS;
        const Row &r = rows[(size_t)t * NS + (size_t)s];
        *lb = r.lb; *m = r.m; *log_s = r.log_s;
        memcpy(top, r.key, sizeof(r.key));
    }, out);
    printf("%lld %lld\n", nodes, node_bound(T, W, S));
    for (const Result &r : out) {
        printf("%.17g", r.score);
        for (int32_t t : r.tokens) printf(" %d", t);
        printf(" |");
        for (int32_t t : r.frames) printf(" %d", t);
        printf(" |");
        for (float x : r.lps) printf(" %u", nasr_lp::f32_bits(x));
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("beam_math")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", "-o", str(exe), str(src)])
    return exe


def state_of(y, NS):
    s = 0
    for k in y:
        s = (s * 31 + int(k) + 1) % NS
    return s


def pack_key(v, idx):
    """nasr_lp::pack_key: (order-preserving image of the f32 bits) << 32 | (0xffffffff - index)"""
    u = struct.unpack("<I", struct.pack("<f", float(v)))[0]
    u = (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)
    return (u << 32) | (0xffffffff - int(idx))


class Table:
    """logits[t][state][1025]; per row m = the largest logit and log s = ln sum exp(logit - m) rounded to f32, ln P = (logit - m) - log s in
    float32 as nasr_topk::lp_of takes it.  `direct`: the entries are hand-made ln P values (m = log s = 0), dyadic so that double sums are exact
    and scores can tie"""

    def __init__(self, logits, direct=False):
        self.x = np.asarray(logits, np.float32)
        self.T, self.NS = self.x.shape[:2]
        self.direct = direct

    def softmax(self, row):
        if self.direct:
            return np.float32(0.0), np.float32(0.0)
        m = np.float32(row.max())
        return m, np.float32(np.log(np.exp(row.astype(np.float64) - np.float64(m)).sum()))

    def lp(self, row):
        row = np.asarray(row, np.float32)
        m, log_s = self.softmax(row)
        return ((row - m) - log_s).astype(np.float64)              # two float32 subtractions

    def joint(self, t, y):
        return self.x[t, state_of(y, self.NS)]

    def write(self, path, W, N, S):
        with open(path, "wb") as f:
            f.write(struct.pack("<5i", self.T, W, N, S, self.NS))
            for t in range(self.T):
                for s in range(self.NS):
                    row = self.x[t, s]
                    m, log_s = self.softmax(row)
                    top = br.top_order(row)[:8]
                    f.write(struct.pack("<f", self.lp(row)[BLANK]))
                    f.write(struct.pack("<8Q", *[pack_key(row[k], k) for k in top]))
                    f.write(struct.pack("<2f", m, log_s))


def run_driver(driver, tab, W, N, S, prune, tmp_path):
    path = tmp_path / "model.bin"
    tab.write(path, W, N, S)
    r = subprocess.run([str(driver), str(path), "1" if prune else "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    nodes, bound = (int(v) for v in lines[0].split())
    hyps = []
    for ln in lines[1:]:
        a, b, c = ln.split("|")
        a = a.split()
        hyps.append(dict(score=float(a[0]), tokens=[int(v) for v in a[1:]], frames=[int(v) for v in b.split()], lp_bits=[int(v) for v in c.split()]))
    return hyps, nodes, bound


def check(driver, tab, W, N, S, tmp_path):
    """driver (prune off and on) against the reference (prune off and on); returns (hyps, stats)"""
    ref, stats = br.search(tab.joint, tab.T, W, N, S, prune=False, logsoftmax=tab.lp)
    ref_p, _ = br.search(tab.joint, tab.T, W, N, S, prune=True, logsoftmax=tab.lp)
    assert ref == ref_p
    got, nodes, bound = run_driver(driver, tab, W, N, S, False, tmp_path)
    got_p, nodes_p, _ = run_driver(driver, tab, W, N, S, True, tmp_path)
    assert got == got_p
    assert 0 <= nodes_p <= nodes <= bound == tab.T * S * W
    assert len(got) == len(ref) and 1 <= len(got) <= N
    for g, r in zip(got, ref):
        assert g["tokens"] == r["tokens"] and g["frames"] == r["frames"]
        assert abs(g["score"] - r["score"]) <= 1e-12 * max(tab.T + len(r["tokens"]), 1)
        assert g["lp_bits"] == [struct.unpack("<I", struct.pack("<f", x))[0] for x in r["lps"]]
    assert len({tuple(g["tokens"]) for g in got}) == len(got)
    assert all(a["score"] >= b["score"] for a, b in zip(got, got[1:]))
    return got, stats


def peaky(rng, T, NS, scale, blank_bias):
    x = rng.standard_normal((T, NS, V)).astype(np.float32) * np.float32(scale)
    x[:, :, BLANK] += np.float32(blank_bias)
    return x


@pytest.mark.parametrize("T,W,N,S,NS,scale,bias", [(6, 1, 1, 10, 5, 4.0, 6.0), (6, 2, 2, 3, 5, 4.0, 8.0), (9, 4, 3, 3, 7, 3.0, 7.0), (7, 8, 8, 2, 4, 3.0, 7.0),
                                                    (13, 4, 4, 4, 1, 3.0, 9.0), (5, 3, 1, 1, 3, 5.0, 5.0), (4, 7, 7, 4, 6, 2.0, 2.0)])
def test_random_lattices(driver, tmp_path, T, W, N, S, NS, scale, bias):
    rng = np.random.default_rng(1000 * T + 10 * W + S)
    got, stats = check(driver, Table(peaky(rng, T, NS, scale, bias)), W, N, S, tmp_path)
    assert stats["evals"] > T


def test_ties_and_equal_logit_bits(driver, tmp_path):
    """hand-made dyadic ln P values: whole groups of outputs share their bits (the lower id goes first), the same row at every frame and
    state, so a sequence's score does not depend on where its tokens fall -- every merge meets an exact tie and the earlier arrival stays"""
    row = np.full(V, -64.0, np.float32)
    row[[7, 3, 900]] = -1.5                                            # equal bits: order 3, 7, 900
    row[[12, 11]] = -2.25
    row[BLANK] = -0.75
    row[[500, 20, 21, 22]] = -3.0
    for T, W, N, S in ((4, 4, 4, 3), (3, 8, 8, 2), (5, 2, 2, 4), (1, 3, 3, 3)):
        tab = Table(np.broadcast_to(row, (T, 1, V)).copy(), direct=True)
        got, stats = check(driver, tab, W, N, S, tmp_path)
        if T > 1:
            assert stats["merges"] > 0 and stats["merge_margin"] == 0.0
        assert got[0]["tokens"] == [] and got[0]["score"] == -0.75 * T
        if W >= 4 and T > 1:
            assert [g["tokens"] for g in got[1:4]] == [[3], [7], [900]]       # equal scores: the expansion order decides
            assert all(g["frames"] == [0] for g in got[1:4])                  # ... and the earliest path keeps its frames


def test_two_paths_in_one_frame(driver, tmp_path):
    """(a) sits in Beam_t and () makes the child (a) at frame t: both reach C in the same frame; the better path's frames stay"""
    rng = np.random.default_rng(5)
    base = peaky(rng, 1, 1, 2.5, 6.5)                                      # nearly the same row at every frame: the same tokens lead everywhere
    x = base + rng.standard_normal((8, 1, V)).astype(np.float32) * np.float32(0.3)
    got, stats = check(driver, Table(x), 4, 4, 3, tmp_path)
    assert stats["merges"] > 0 and 0 < stats["merge_margin"] < np.inf


def test_no_frame_one_frame_and_more_tokens_than_frames(driver, tmp_path):
    rng = np.random.default_rng(6)
    got, _ = check(driver, Table(np.zeros((0, 2, V), np.float32)), 4, 4, 3, tmp_path)
    assert got == [dict(score=0.0, tokens=[], frames=[], lp_bits=[])]
    for W, S in ((1, 10), (4, 3), (8, 2)):                                 # blank is unlikely until S tokens are out: S symbols on the one frame
        got, _ = check(driver, chain_table(1, S), W, W, S, tmp_path)
        assert len(got[0]["tokens"]) == S and got[0]["frames"] == [0] * S
    got, _ = check(driver, chain_table(3, 7), 4, 4, 4, tmp_path)           # U > T
    assert len(got[0]["tokens"]) == 7
    frames = got[0]["frames"]
    assert all(a <= b for a, b in zip(frames, frames[1:])) and max(np.bincount(frames)) <= 4 and max(frames) < 3


def chain_table(T, U, NS=997):
    """hand-made ln P: along the chain 100, 101, .. the next token is likely and blank is not, until U tokens are out"""
    x = np.full((T, NS, V), -64.0, np.float32)
    x[:, :, BLANK] = -0.125
    x[:, :, 1:9] = -8.0
    y, seen = (), set()
    for i in range(U):
        s = state_of(y, NS)
        assert s not in seen
        seen.add(s)
        x[:, s, BLANK], x[:, s, 100 + i] = -2.0, -0.125
        y += (100 + i,)
    assert state_of(y, NS) not in seen
    return Table(x, direct=True)


def test_beam_8_with_blank_inside_and_outside_the_top_8(driver, tmp_path):
    rng = np.random.default_rng(8)
    x = peaky(rng, 4, 6, 3.0, 0.0)
    x[0::2, :, BLANK] = x[0::2].max(axis=2) + 1.0                          # blank first: 7 tokens expand
    x[1::2, :, BLANK] = np.sort(x[1::2], axis=2)[:, :, -12]                # blank outside the top 8: 8 tokens expand
    tab = Table(x)
    assert BLANK in br.top_order(x[0, 0])[:8] and BLANK not in br.top_order(x[1, 0])[:8]
    check(driver, tab, 8, 8, 2, tmp_path)
    check(driver, tab, 8, 5, 3, tmp_path)


def test_beam_1_is_not_greedy(driver, tmp_path):
    """the search may drop a token whose continuation scores below the blank: the header's beam 1 against the greedy decode of the same table"""
    rows = np.full((2, V), -30.0, np.float32)
    rows[0, 5], rows[0, BLANK] = 1.0, 0.9                                  # state 0: token 5 just ahead of blank ...
    rows[1, BLANK], rows[1, 9] = 0.0, 0.5                                  # ... but after it nothing is likely: blank 0.38, token 0.62, then the same again
    tab = Table(np.stack([rows, rows]))
    g, _ = br.greedy(tab.joint, 2)
    got, _ = check(driver, tab, 1, 1, 3, tmp_path)
    assert g[:1] == [5] and got[0]["tokens"] != g and got[0]["tokens"] == []


def test_expand_skips_blank_and_empty_keys(driver):
    """nasr_beam::expand on packed keys: blank is dropped wherever it stands, a list with fewer than 8 keys (0 = none) ends early, the
    first W of the rest are kept and ln P is the key's own logit"""
    def run(W, keys):
        r = subprocess.run([str(driver), "expand", str(W)] + [str(k) for k in keys], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return [tuple(int(v) for v in item.split(":")) for item in r.stdout.split()]

    bits = lambda v: struct.unpack("<I", struct.pack("<f", v))[0]
    vals = [(-0.5, 7), (-0.75, BLANK), (-1.0, 3), (-1.0, 900), (-2.5, 0), (-3.0, 11), (-3.5, 12), (-4.0, 13)]
    keys = [pack_key(v, k) for v, k in vals]
    assert keys == sorted(keys, reverse=True)
    toks = [(k, bits(v)) for v, k in vals if k != BLANK]
    for W in range(1, 9):
        assert run(W, keys) == toks[:W]
    assert run(8, keys[:3] + [0] * 5) == [toks[0], toks[1]]
    assert run(4, [keys[1]] + [0] * 7) == [] and run(4, [0] * 8) == []
