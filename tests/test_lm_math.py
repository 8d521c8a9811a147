"""nasr_lm.h (the builder, the compiled tables and the lookup of the back-off n-gram model) and the fused rules of nasr_beam.h, compiled with
g++ under AddressSanitizer / UBSan into a stand-alone driver -- no GPU.  Random models of order 1 .. 5 over 6 to 40 distinct tokens, with BOS
and EOS n-grams present and absent and positive back-offs present and absent: every (state, token) lookup and every next state against
tests/lm_ref.py, exactly (both are double sums of the same float32 values in the same order); a table at its smallest capacity, where probes
wrap around the end; max_probe is the real maximum; each validity error.  The fused host search equals tests/beam_lm_ref.py on the random
lattices of tests/test_beam_math.py at W in {1, 2, 4, 8}; pruned equals unpruned where the prune condition holds and the search runs
unpruned where it does not; weight 0 / bonus 0 equals the LM-free search in every field."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import beam_lm_ref as blr
from tests import lm_ref
from tests.test_beam_math import Table, peaky

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"
BOS, EOS = lm_ref.BOS, lm_ref.EOS

DRIVER = r"""
#include "nasr_beam.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace nasr_beam;
// model file: i32 order, i32 n, f32 unk, i32 tight; per n-gram: i32 len, i32 tok[len], f32 lp, f32 bo
static int read_lm(const char *path, nasr_lm::Model &m, std::string &err, std::vector<int32_t> &len, std::vector<int32_t> &tok) {
    FILE *f = fopen(path, "rb");
    if (!f) { err = "cannot open"; return -2; }
    int32_t order, n, tight; float unk;
    if (fread(&order, 4, 1, f) != 1 || fread(&n, 4, 1, f) != 1 || fread(&unk, 4, 1, f) != 1 || fread(&tight, 4, 1, f) != 1) return -2;
    std::vector<float> lp, bo;
    for (int i = 0; i < n; i++) {
        int32_t l;
        if (fread(&l, 4, 1, f) != 1) return -2;
        len.push_back(l);
        for (int j = 0; j < (l > 0 ? l : 0); j++) { int32_t t; if (fread(&t, 4, 1, f) != 1) return -2; tok.push_back(t); }
        float a, b;
        if (fread(&a, 4, 1, f) != 1 || fread(&b, 4, 1, f) != 1) return -2;
        lp.push_back(a); bo.push_back(b);
    }
    fclose(f);
    return nasr_lm::build(order, n, len.data(), tok.data(), lp.data(), bo.data(), unk, m, err, tight != 0);
}
struct Row { float lb; nasr_topk::tkey key[KTOP]; float m, log_s; };
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    nasr_lm::Model m;
    std::string err;
    std::vector<int32_t> len, tok;
    const bool have_lm = strcmp(argv[2], "-") != 0;
    if (have_lm && read_lm(argv[2], m, err, len, tok)) { printf("error: %s\n", err.c_str()); return 0; }
    const nasr_lm::View v = m.view();
    if (!strcmp(argv[1], "lm")) {
        // lm <model> probe tokens ..: the header, then per n-gram shorter than the order "index state" and per probe token "value next"
        int real_probe = 0, wrapped = 0;
        long long arcs = 0;
        const size_t cap = m.arcs.size();
        for (size_t at = 0; at < cap; at++) {
            if (m.arcs[at].key == nasr_lm::EMPTY) continue;
            arcs++;
            const size_t home = (size_t)(nasr_lm::mix(m.arcs[at].key) & (cap - 1));
            const int probes = (int)((at + cap - home) & (cap - 1)) + 1;
            if (probes > real_probe) real_probe = probes;
            if (at < home) wrapped++;
        }
        printf("%d %d %zu %lld %zu %d %d %d %d\n", m.max_probe, real_probe, cap, arcs, m.states.size(), m.start, (int)m.has_eos, (int)m.all_nonpositive, wrapped);
        size_t at = 0;
        for (size_t i = 0; i < len.size(); at += (size_t)len[i], i++) {
            if (len[i] >= m.order) continue;
            int32_t st = 0;
            for (int j = 0; j < len[i]; j++) nasr_lm::lookup(v, st, tok[at + (size_t)j], &st);
            printf("%zu %d", i, st);
            for (int a = 3; a < argc; a++) {
                int32_t next = -1;
                const double x = nasr_lm::lookup(v, st, atoi(argv[a]), &next);
                printf(" %.17g %d", x, next);
            }
            printf("\n");
        }
        printf("-1 0");
        for (int a = 3; a < argc; a++) {
            int32_t next = -1;
            const double x = nasr_lm::lookup(v, 0, atoi(argv[a]), &next);
            printf(" %.17g %d", x, next);
        }
        printf("\n");
        return 0;
    }
    // <lattice> <model or -> <prune> <weight> <bonus>: the lattice file of tests/test_beam_math.py
    if (argc < 6) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[5];
    if (fread(hd, 4, 5, f) != 5) return 3;
    const int T = hd[0], W = hd[1], N = hd[2], S = hd[3], NS = hd[4];
    if (!valid_params(W, N, S)) return 4;
    std::vector<Row> rows((size_t)T * NS);
    for (Row &r : rows)
        if (fread(&r.lb, 4, 1, f) != 1 || fread(r.key, 8, KTOP, f) != (size_t)KTOP || fread(&r.m, 4, 1, f) != 1 || fread(&r.log_s, 4, 1, f) != 1) return 3;
    fclose(f);
    auto eval = [&](int t, const int32_t *seq, int n, float *lb, nasr_topk::tkey *top, float *mm, float *log_s) {
        long long s = 0;
        for (int i = 0; i < n; i++) s = (s * 31 + seq[i] + 1) % NS;
        const Row &r = rows[(size_t)t * NS + (size_t)s];
        *lb = r.lb; *mm = r.m; *log_s = r.log_s;
        memcpy(top, r.key, sizeof(r.key));
    };
    std::vector<Result> out;
    bool pruned = atoi(argv[3]) != 0;
    const float weight = strtof(argv[4], nullptr), bonus = strtof(argv[5], nullptr);
    if (have_lm && !valid_weights(weight, bonus)) { printf("error: weights\n"); return 0; }
    const long long nodes = have_lm ? search(T, W, N, S, pruned, eval, out, v, weight, bonus, &pruned) : search(T, W, N, S, pruned, eval, out);
    printf("%lld %d\n", nodes, (int)pruned);
    for (const Result &r : out) {
        printf("%.17g %.17g %.17g %.17g", r.score, r.lm, r.lm_final, r.total);
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
    d = tmp_path_factory.mktemp("lm_math")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", "-o", str(exe), str(src)])
    return exe


def write_lm(path, ngrams, order, unk, tight=False):
    """ngrams: {tuple: (lp, bo)} or a list of (tuple, lp, bo) -- the list form may hold what a dictionary cannot (duplicates)"""
    items = [(k, v[0], v[1]) for k, v in ngrams.items()] if isinstance(ngrams, dict) else list(ngrams)
    with open(path, "wb") as f:
        f.write(struct.pack("<iifi", order, len(items), unk, 1 if tight else 0))
        for k, lp, bo in items:
            f.write(struct.pack(f"<i{len(k)}iff", len(k), *k, lp, bo))
    return items


def run(driver, *args):
    r = subprocess.run([str(driver)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r.stdout.strip().splitlines()


def check_lm(driver, tmp_path, ngrams, order, unk, tight=False):
    """every (state, token) lookup and next state against the reference; -> the header figures"""
    path = tmp_path / "lm.bin"
    items = write_lm(path, ngrams, order, unk, tight)
    ref = lm_ref.RefLM(ngrams, order, unk)
    toks = sorted({t for k in ngrams for t in k if t < 1024})
    probe = toks + [EOS] + [t for t in (0, 511, 1023) if t not in toks][:2]
    lines = run(driver, "lm", path, *probe)
    assert not lines[0].startswith("error"), lines[0]
    max_probe, real_probe, cap, arcs, n_states, start, has_eos, nonpos, wrapped = (int(x) for x in lines[0].split())
    n_arcs = sum(1 for k in ngrams if len(k) > 1)
    contexts = [k for k, _, _ in items if len(k) < order]
    assert arcs == n_arcs and n_states == len(contexts) + 1
    assert cap & (cap - 1) == 0 and (cap >= n_arcs + 1 if tight else cap >= max(2 * n_arcs, 1)) and (not tight or cap < 2 * (n_arcs + 1))
    assert max_probe == real_probe and (n_arcs == 0 or max_probe >= 1)
    assert bool(has_eos) == ref.has_eos and bool(nonpos) == ref.all_nonpositive
    state_of = {(): 0}
    rows = {}
    for ln in lines[1:]:
        a = ln.split()
        i, st = int(a[0]), int(a[1])
        ctx = () if i < 0 else items[i][0]
        state_of[ctx] = st
        rows[ctx] = [(float(a[2 + 2 * j]), int(a[3 + 2 * j])) for j in range(len(probe))]
    assert len(set(state_of.values())) == len(state_of) == n_states and sorted(state_of.values()) == list(range(n_states))
    assert start == (state_of[(BOS,)] if (BOS,) in state_of else 0)
    n = 0
    for ctx, row in rows.items():
        for w, (val, nxt) in zip(probe, row):
            assert val == ref.term(ctx, w), (ctx, w, val, ref.term(ctx, w))
            assert nxt == state_of[ref.context_after(ctx, w)], (ctx, w, nxt, ref.context_after(ctx, w))
            n += 1
    return dict(max_probe=max_probe, cap=cap, arcs=n_arcs, wrapped=wrapped, lookups=n, ref=ref)


CASES = [(order, n_tok, bos, eos, pos) for order, n_tok in ((1, 6), (2, 9), (3, 17), (4, 40), (5, 12), (3, 6), (5, 40))
         for bos, eos, pos in ((True, True, False), (False, False, True), (True, False, True), (False, True, False))]


@pytest.mark.parametrize("order,n_tok,bos,eos,pos", CASES)
def test_every_lookup_and_next_state_against_the_reference(driver, tmp_path, order, n_tok, bos, eos, pos):
    rng = np.random.default_rng(100 * order + n_tok + 7 * bos + 3 * eos + pos)
    g = lm_ref.random_lm(rng, order, n_tok, bos=bos, eos=eos, positive_backoff=pos)
    info = check_lm(driver, tmp_path, g, order, -7.5)
    ref = info["ref"]
    assert ref.has_eos == eos and (order == 1 or ref.all_nonpositive == (not pos))
    assert info["lookups"] > n_tok and (order == 1 or info["arcs"] > 0)


def test_smallest_capacity_probes_wrap_around_the_end(driver, tmp_path):
    """capacity = the smallest power of two above the arc count: long probe sequences, some of which pass the table's last slot"""
    wrapped = 0
    for seed in range(4):
        rng = np.random.default_rng(900 + seed)
        g = lm_ref.random_lm(rng, 3, 24, positive_backoff=bool(seed & 1), max_per_level=250 + seed)
        info = check_lm(driver, tmp_path, g, 3, -9.0, tight=True)
        loose = check_lm(driver, tmp_path, g, 3, -9.0)
        assert info["cap"] <= loose["cap"] and info["max_probe"] >= loose["max_probe"] and info["max_probe"] >= 3
        wrapped += info["wrapped"]
    assert wrapped > 0


def test_each_validity_error_names_the_ngram(driver, tmp_path):
    ok = [((5,), -1.0, -0.5), ((6,), -1.5, 0.0), ((5, 6), -0.5, 0.0), ((BOS,), -3.0, -0.25), ((BOS, 5), -0.75, 0.0), ((5, EOS), -1.0, 0.0)]

    def err(items, order=2, unk=-5.0):
        path = tmp_path / "bad.bin"
        write_lm(path, items, order, unk)
        out = run(driver, "lm", path, 5)
        assert out[0].startswith("error: "), out[0]
        return out[0]

    path = tmp_path / "ok.bin"
    write_lm(path, ok, 2, -5.0)
    assert not run(driver, "lm", path, 5)[0].startswith("error")
    assert "duplicate" in err(ok + [((5, 6), -0.25, 0.0)]) and "(5 6)" in err(ok + [((5, 6), -0.25, 0.0)])
    assert "length" in err(ok + [((5, 6, 5), -0.25, 0.0)]) and "length" in err(ok + [((), -0.25, 0.0)])
    for bad in ((1024,), (5, BOS), (EOS, 5), (1027,), (-1,), (5, 1024)):
        msg = err(ok + [(bad, -0.25, 0.0)])
        assert "out of place" in msg and "(" + " ".join(str(t) for t in bad) + ")" in msg
    for lp, bo in ((float("nan"), 0.0), (float("-inf"), 0.0), (0.5, 0.0), (-1.0, float("inf")), (-1.0, float("nan"))):
        assert "(7)" in err(ok + [((7,), lp, bo)])
    msg = err(ok + [((9, 6), -0.25, 0.0)])
    assert "context" in msg and "(9 6)" in msg
    assert "order" in err(ok, order=0) and "order" in err(ok, order=6)
    assert "unk" in err(ok, unk=0.5) and "unk" in err(ok, unk=float("nan"))


def test_too_many_ngrams_is_refused_before_anything_is_read(driver, tmp_path):
    """more than 2^24 n-grams: the count alone fails the build (the arrays are not touched), so the file holds none"""
    path = tmp_path / "many.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<iifi", 2, 0, -5.0, 0))
    src = tmp_path / "many.cpp"
    src.write_text('#include "nasr_lm.h"\n#include <cstdio>\nint main() { nasr_lm::Model m; std::string e; int32_t one = 1, t = 5; float lp = -1.0f;\n'
                   'int rc = nasr_lm::build(2, nasr_lm::MAX_NGRAMS + 1, &one, &t, &lp, nullptr, -5.0f, m, e); printf("%d %s\\n", rc, e.c_str()); return 0; }\n')
    exe = tmp_path / "many"
    subprocess.check_call([shutil.which("g++") or "c++", "-std=c++17", "-O1", "-fsanitize=address,undefined", f"-I{CSRC}", "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("-1 ") and "more than" in out.stdout, (out.stdout, out.stderr[-2000:])


# ---- the fused search ---------------------------------------------------------------------------------------------------------------
def run_search(driver, tab, W, N, S, prune, tmp_path, lm_path="-", weight=0.0, bonus=0.0):
    path = tmp_path / "model.bin"
    tab.write(path, W, N, S)
    lines = run(driver, path, lm_path, 1 if prune else 0, repr(float(weight)), repr(float(bonus)))
    nodes, pruned = (int(v) for v in lines[0].split())
    hyps = []
    for ln in lines[1:]:
        a, b, c = ln.split("|")
        a = a.split()
        hyps.append(dict(score=float(a[0]), lm=float(a[1]), lm_final=float(a[2]), total=float(a[3]), tokens=[int(v) for v in a[4:]],
                         frames=[int(v) for v in b.split()], lp_bits=[int(v) for v in c.split()]))
    return hyps, nodes, bool(pruned)


def lattice_tokens(tab, W):
    """tokens the lattice's rows rank high: an LM over them bites"""
    ids = set()
    for t in range(tab.T):
        for s in range(tab.NS):
            ids.update(int(k) for k in np.argsort(-tab.x[t, s])[:W + 2] if k != 1024)
    return sorted(ids)


LATTICES = [(6, 1, 1, 10, 5, 4.0, 6.0), (6, 2, 2, 3, 5, 4.0, 8.0), (9, 4, 3, 3, 7, 3.0, 7.0), (7, 8, 8, 2, 4, 3.0, 7.0), (4, 7, 7, 4, 6, 2.0, 2.0)]


@pytest.mark.parametrize("T,W,N,S,NS,scale,bias", LATTICES)
@pytest.mark.parametrize("pos,weight,bonus", [(False, 0.6, 0.0), (True, 0.8, 0.5), (False, 0.4, 0.75)], ids=["prunable", "positive-backoff+bonus", "bonus"])
def test_fused_search_equals_the_reference(driver, tmp_path, T, W, N, S, NS, scale, bias, pos, weight, bonus):
    rng = np.random.default_rng(1000 * T + 10 * W + S)                     # the lattices of tests/test_beam_math.py
    tab = Table(peaky(rng, T, NS, scale, bias))
    ids = lattice_tokens(tab, W)
    lrng = np.random.default_rng(77 + W)
    g = lm_ref.random_lm(lrng, 3, len(ids), tokens=ids[:40], bos=True, eos=True, positive_backoff=pos, density=0.2)
    ref_lm = lm_ref.RefLM(g, 3, -6.0)
    lm_path = tmp_path / "lm.bin"
    write_lm(lm_path, g, 3, -6.0)
    ref, stats = blr.search(tab.joint, tab.T, W, N, S, prune=False, logsoftmax=tab.lp, lm=ref_lm, weight=weight, bonus=bonus)
    ref_p, stats_p = blr.search(tab.joint, tab.T, W, N, S, prune=True, logsoftmax=tab.lp, lm=ref_lm, weight=weight, bonus=bonus)
    allowed = bonus == 0.0 and not pos
    assert ref == ref_p and stats_p["pruned"] == allowed
    got, nodes, pruned = run_search(driver, tab, W, N, S, False, tmp_path, lm_path, weight, bonus)
    got_p, nodes_p, pruned_p = run_search(driver, tab, W, N, S, True, tmp_path, lm_path, weight, bonus)
    assert not pruned and pruned_p == allowed                              # unpruned whenever the condition does not hold ...
    assert got == got_p                                                    # ... and the same result where it does
    assert nodes_p <= nodes <= T * S * W and (allowed or nodes_p == nodes)
    assert len(got) == len(ref) >= 1
    bound = 1e-12 * max(tab.T + max(len(r["tokens"]) for r in ref), 1)
    for h, r in zip(got, ref):
        assert h["tokens"] == r["tokens"] and h["frames"] == r["frames"]
        assert abs(h["score"] - r["score"]) <= bound
        assert h["lm"] == r["lm"] == ref_lm.score(r["tokens"], eos=False)[0] and h["lm_final"] == r["lm_final"] == ref_lm.score(r["tokens"])[0]
        assert h["total"] == blr.total_of(h["score"], h["lm_final"], len(h["tokens"]), weight, bonus)
        assert abs(h["total"] - r["total"]) <= bound
    assert all(a["total"] >= b["total"] for a, b in zip(got, got[1:])) and len({tuple(h["tokens"]) for h in got}) == len(got)
    free, _, _ = run_search(driver, tab, W, N, S, True, tmp_path)
    assert any(h["lm"] != 0.0 for h in got) or all(not h["tokens"] for h in free)


@pytest.mark.parametrize("T,W,N,S,NS,scale,bias", LATTICES)
def test_weight_zero_equals_the_lm_free_search_in_every_field(driver, tmp_path, T, W, N, S, NS, scale, bias):
    rng = np.random.default_rng(1000 * T + 10 * W + S)
    tab = Table(peaky(rng, T, NS, scale, bias))
    g = lm_ref.random_lm(np.random.default_rng(5), 3, 0, tokens=lattice_tokens(tab, W)[:40], density=0.2)          # no EOS term would move the final order at weight 0 anyway
    lm_path = tmp_path / "lm.bin"
    write_lm(lm_path, g, 3, -6.0)
    for prune in (False, True):
        free, nodes, _ = run_search(driver, tab, W, N, S, prune, tmp_path)
        got, nodes_lm, _ = run_search(driver, tab, W, N, S, prune, tmp_path, lm_path, 0.0, 0.0)
        assert nodes == nodes_lm and len(got) == len(free)
        for h, f in zip(got, free):
            assert (h["score"], h["tokens"], h["frames"], h["lp_bits"]) == (f["score"], f["tokens"], f["frames"], f["lp_bits"])
            assert h["total"] == h["score"]


def test_no_frame_gives_the_empty_hypothesis_with_its_eos_term(driver, tmp_path):
    g = {(5,): (-1.0, 0.0), (BOS,): (-9.0, -0.5), (BOS, EOS): (-0.25, 0.0), (EOS,): (-3.0, 0.0)}
    lm_path = tmp_path / "lm.bin"
    write_lm(lm_path, g, 2, -6.0)
    got, nodes, _ = run_search(driver, Table(np.zeros((0, 2, 1025), np.float32)), 4, 4, 3, True, tmp_path, lm_path, 2.0, 0.5)
    assert nodes == 0 and got == [dict(score=0.0, lm=0.0, lm_final=-0.25, total=-0.5, tokens=[], frames=[], lp_bits=[])]
