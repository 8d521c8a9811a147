"""The BOOST rules of nasr_beam.h (phrase boosting inside the beam search: the boosted expansion list, the key with boost added last, the
automaton state and the bonus sum per hypothesis, prune_allowed with a set, the boosted final order), compiled with g++ under
AddressSanitizer / UBSan into a stand-alone driver -- no GPU.  The driver runs nasr_beam::search_boost over the synthetic table models of
tests/test_beam_math.py, handed the rows' RAW logits, with the tables nasr_boost::build makes of a seeded phrase set; the reference is
tests/beam_boost_ref.py, whose bonus is brute force over the phrases (the definition, not the automaton).  Tokens and frames are exact, ln P
equal in their bits, boost and the per-token bonuses exact (dyadic bonuses), scores within 1e-12 * (T + U); the host search's slot-binding
checks return clean on every run (a negative node count is a failure)."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import beam_boost_ref as bbr
from tests import beam_lm_ref as blr
from tests import beam_ref as br
from tests import lm_ref
from tests.test_beam_math import Table, peaky
from tests.test_lm_math import lattice_tokens, write_lm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"
BLANK, V = 1024, 1025
BONUSES = (0.5, 1.0, 2.0, 4.0)

DRIVER = r"""
#include "nasr_beam.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
using namespace nasr_beam;
static int read_lm(const char *path, nasr_lm::Model &m, std::string &err) {      // the model file of tests/test_lm_math.py
    FILE *f = fopen(path, "rb");
    if (!f) { err = "cannot open"; return -2; }
    int32_t order, n, tight; float unk;
    if (fread(&order, 4, 1, f) != 1 || fread(&n, 4, 1, f) != 1 || fread(&unk, 4, 1, f) != 1 || fread(&tight, 4, 1, f) != 1) return -2;
    std::vector<int32_t> len, tok;
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
struct Row { float lb, m, log_s; float raw[1025]; };
// prune: the table of prune_allowed
// <lattice> <phrases> <model or -> <prune> <weight> <bonus> <boost | plain>
//   lattice: i32 T, W, N, S, NS; per (t, state): f32 lb, m, log_s, raw[1025].  phrases: i32 n; per phrase i32 len, i32 tok[len], f32 bonus
int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "prune")) {
        for (int tb = 0; tb < 2; tb++) for (int nonpos = 0; nonpos < 2; nonpos++) for (int st = 2; st < 5; st++)
            printf("%d %d %d %d\n", tb, nonpos, st, (int)prune_allowed(tb ? 0.5f : 0.0f, nonpos != 0, st));
        return 0;
    }
    if (argc < 8) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[5];
    if (fread(hd, 4, 5, f) != 5) return 3;
    const int T = hd[0], W = hd[1], N = hd[2], S = hd[3], NS = hd[4];
    if (!valid_params(W, N, S)) return 4;
    std::vector<Row> rows((size_t)T * NS);
    for (Row &r : rows)
        if (fread(&r.lb, 4, 1, f) != 1 || fread(&r.m, 4, 1, f) != 1 || fread(&r.log_s, 4, 1, f) != 1 || fread(r.raw, 4, 1025, f) != 1025) return 3;
    fclose(f);
    f = fopen(argv[2], "rb");
    if (!f) return 2;
    int32_t np = 0;
    if (fread(&np, 4, 1, f) != 1) return 3;
    std::vector<std::vector<int32_t>> ptok((size_t)np);
    std::vector<const int32_t *> pp;
    std::vector<int32_t> plen;
    std::vector<float> pbon((size_t)np);
    for (int i = 0; i < np; i++) {
        int32_t l;
        if (fread(&l, 4, 1, f) != 1) return 3;
        ptok[(size_t)i].resize((size_t)l);
        if (fread(ptok[(size_t)i].data(), 4, (size_t)l, f) != (size_t)l || fread(&pbon[(size_t)i], 4, 1, f) != 1) return 3;
        plen.push_back(l);
    }
    fclose(f);
    for (auto &p : ptok) pp.push_back(p.data());
    nasr_boost::Automaton au;
    if (nasr_boost::build(np, pp.data(), plen.data(), pbon.data(), nasr_boost::MAX_STATES, au)) return 5;
    const BoostTables bt = {au.bonus.data(), au.next.data(), au.n_states};
    nasr_lm::Model m;
    std::string err;
    const bool have_lm = strcmp(argv[3], "-") != 0;
    if (have_lm && read_lm(argv[3], m, err)) { printf("error: %s\n", err.c_str()); return 0; }
    const nasr_lm::View v = m.view();
    auto row_of = [&](int t, const int32_t *seq, int n) -> const Row & {
        long long s = 0;
        for (int i = 0; i < n; i++) s = (s * 31 + seq[i] + 1) % NS;
        return rows[(size_t)t * NS + (size_t)s];
    };
    auto eval_raw = [&](int t, const int32_t *seq, int n, float *lb, const float **raw, float *mm, float *log_s) {
        const Row &r = row_of(t, seq, n);
        *lb = r.lb; *mm = r.m; *log_s = r.log_s; *raw = r.raw;
    };
    auto eval_keys = [&](int t, const int32_t *seq, int n, float *lb, nasr_topk::tkey *top, float *mm, float *log_s) {      // what the unboosted joint leaves
        const Row &r = row_of(t, seq, n);
        *lb = r.lb; *mm = r.m; *log_s = r.log_s;
        boosted_top(r.raw, au.bonus.data(), top);                                  // the disabled state's row: all 0
    };
    std::vector<Result> out;
    bool pruned = atoi(argv[4]) != 0;
    const float weight = strtof(argv[5], nullptr), bonus = strtof(argv[6], nullptr);
    long long nodes;
    if (!strcmp(argv[7], "boost")) nodes = have_lm ? search_boost(T, W, N, S, pruned, eval_raw, out, bt, v, weight, bonus, &pruned) : search_boost(T, W, N, S, pruned, eval_raw, out, bt, &pruned);
    else nodes = have_lm ? search(T, W, N, S, pruned, eval_keys, out, v, weight, bonus, &pruned) : search(T, W, N, S, pruned, eval_keys, out);
    printf("%lld %d %d\n", nodes, (int)pruned, au.n_states);
    for (const Result &r : out) {
        printf("%.17g %.17g %.17g %.17g %.17g %d", r.score, r.lm, r.lm_final, r.total, r.boost, r.boost_state > 0 ? au.depth[(size_t)r.boost_state] : -1);
        for (int32_t t : r.tokens) printf(" %d", t);
        printf(" |");
        for (int32_t t : r.frames) printf(" %d", t);
        printf(" |");
        for (float x : r.lps) printf(" %u", nasr_lp::f32_bits(x));
        printf(" |");
        for (float x : r.bonuses) printf(" %.9g", x);
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
    d = tmp_path_factory.mktemp("beam_boost_math")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", "-o", str(exe), str(src)])
    return exe


def write_lattice(path, tab, W, N, S):
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", tab.T, W, N, S, tab.NS))
        for t in range(tab.T):
            for s in range(tab.NS):
                row = tab.x[t, s]
                m, log_s = tab.softmax(row)
                f.write(struct.pack("<3f", tab.lp(row)[BLANK], m, log_s))
                f.write(np.asarray(row, "<f4").tobytes())


def write_phrases(path, phrases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(phrases)))
        for p, w in phrases:
            f.write(struct.pack(f"<i{len(p)}if", len(p), *p, w))


def run_search(driver, tab, W, N, S, prune, tmp_path, phrases, lm_path="-", weight=0.0, bonus=0.0, mode="boost"):
    lat, ph = tmp_path / "lattice.bin", tmp_path / "phrases.bin"
    write_lattice(lat, tab, W, N, S)
    write_phrases(ph, phrases)
    r = subprocess.run([str(driver), str(lat), str(ph), str(lm_path), "1" if prune else "0", repr(float(weight)), repr(float(bonus)), mode],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    nodes, pruned, states = (int(v) for v in lines[0].split())
    assert nodes >= 0, "the trie or the slots ran out (-1) or a slot was bound twice (-2)"
    hyps = []
    for ln in lines[1:]:
        a, b, c, d = ln.split("|")
        a = a.split()
        hyps.append(dict(score=float(a[0]), lm=float(a[1]), lm_final=float(a[2]), total=float(a[3]), boost=float(a[4]), depth=int(a[5]),
                         tokens=[int(v) for v in a[6:]], frames=[int(v) for v in b.split()], lp_bits=[int(v) for v in c.split()],
                         bonuses=[float(v) for v in d.split()]))
    return hyps, nodes, bool(pruned), states


def random_phrases(rng, tab, W, n, outside):
    """n phrases of 1 .. 3 tokens with dyadic bonuses: from tokens the rows rank high (they occur in hypotheses: matches complete, fail midway
    and overlap -- some phrases share a prefix, some start with another's last token) and `outside` one-token phrases over ids no row ranks
    among its 8 largest"""
    ids = lattice_tokens(tab, W)
    out = []
    for i in range(n):
        ln = int(rng.integers(1, 4))
        if out and i % 3 == 1:                                             # share a prefix with / continue the previous phrase
            prev = out[-1][0]
            toks = (prev[:1] if i % 2 else prev[-1:]) + tuple(int(t) for t in rng.choice(ids, ln))
            toks = toks[:3]
        else:
            toks = tuple(int(t) for t in rng.choice(ids, ln))
        out.append((toks, float(rng.choice(BONUSES))))
    top8 = set()
    for t in range(tab.T):
        for s in range(tab.NS):
            top8.update(int(k) for k in br.top_order(tab.x[t, s])[:8])
    rest = [v for v in range(BLANK) if v not in top8]
    for v in rng.choice(rest, outside, replace=False):
        out.append(((int(v),), 4.0))
    return out


def longest_prefix_suffix(phrases, tokens):
    """the depth of the automaton state after `tokens`: the longest suffix of the history that is a prefix of some phrase"""
    best = 0
    for p, _ in phrases:
        for k in range(1, len(p) + 1):
            if k <= len(tokens) and tuple(tokens[len(tokens) - k:]) == tuple(p[:k]):
                best = max(best, k)
    return best


def compare(got, ref, phrases, T, weight, bonus, with_lm):
    assert len(got) == len(ref) >= 1
    bound = 1e-12 * max(T + max(len(r["tokens"]) for r in ref), 1)
    ph = bbr.Phrases(phrases)
    for h, r in zip(got, ref):
        assert h["tokens"] == r["tokens"] and h["frames"] == r["frames"]
        assert h["lp_bits"] == [struct.unpack("<I", struct.pack("<f", x))[0] for x in r["lps"]]
        assert abs(h["score"] - r["score"]) <= bound
        assert h["bonuses"] == ph.bonuses(tuple(h["tokens"])) == r["bonuses"]                     # brute force, exactly
        assert h["boost"] == sum(h["bonuses"]) == r["boost"]                                      # dyadic: the sums are exact
        assert h["depth"] == longest_prefix_suffix(phrases, h["tokens"])                          # the child state the search carried
        assert h["total"] == bbr.key_of(h["score"], h["lm_final"], len(h["tokens"]), weight, bonus, h["boost"], with_lm)
        assert abs(h["total"] - r["total"]) <= bound
        if with_lm:
            assert h["lm"] == r["lm"] and h["lm_final"] == r["lm_final"]
    assert all(a["total"] >= b["total"] for a, b in zip(got, got[1:])) and len({tuple(h["tokens"]) for h in got}) == len(got)


LATTICES = [(6, 1, 1, 10, 5, 4.0, 6.0), (6, 2, 2, 3, 5, 4.0, 8.0), (9, 4, 3, 3, 7, 3.0, 7.0), (7, 8, 8, 2, 4, 3.0, 7.0), (4, 7, 7, 4, 6, 2.0, 2.0)]


@pytest.mark.parametrize("T,W,N,S,NS,scale,bias", LATTICES)
def test_boosted_search_equals_the_reference(driver, tmp_path, T, W, N, S, NS, scale, bias):
    rng = np.random.default_rng(1000 * T + 10 * W + S)                     # the lattices of tests/test_beam_math.py
    tab = Table(peaky(rng, T, NS, scale, bias))
    phrases = random_phrases(np.random.default_rng(31 + W), tab, W, 12, 3)
    ref, stats = bbr.search(tab.joint, tab.T, W, N, S, prune=True, logsoftmax=tab.lp, phrases=bbr.Phrases(phrases))
    assert stats["pruned"] is False
    got, nodes, pruned, states = run_search(driver, tab, W, N, S, True, tmp_path, phrases)
    got_u, nodes_u, _, _ = run_search(driver, tab, W, N, S, False, tmp_path, phrases)
    assert not pruned and states > 2 and got == got_u and nodes == nodes_u <= T * S * W      # a non-empty set: unpruned whatever the caller wishes
    compare(got, ref, phrases, T, 0.0, 0.0, False)
    free, _ = br.search(tab.joint, tab.T, W, N, S, logsoftmax=tab.lp)
    print(f"boost W{W}-S{S}-T{T}: proposed_by_boost {stats['proposed_by_boost']}, boosts {[h['boost'] for h in got]}, "
          f"N-best moved {[h['tokens'] for h in got] != [h['tokens'] for h in free]}")
    assert any(h["boost"] > 0 for h in got)


@pytest.mark.parametrize("T,W,N,S,NS,scale,bias", LATTICES)
@pytest.mark.parametrize("pos,weight,bonus", [(False, 0.6, 0.0), (True, 0.8, 0.5)], ids=["prunable", "positive-backoff+bonus"])
def test_boost_and_lm_together(driver, tmp_path, T, W, N, S, NS, scale, bias, pos, weight, bonus):
    rng = np.random.default_rng(1000 * T + 10 * W + S)
    tab = Table(peaky(rng, T, NS, scale, bias))
    ids = lattice_tokens(tab, W)
    g = lm_ref.random_lm(np.random.default_rng(77 + W), 3, len(ids), tokens=ids[:40], bos=True, eos=True, positive_backoff=pos, density=0.2)
    ref_lm = lm_ref.RefLM(g, 3, -6.0)
    lm_path = tmp_path / "lm.bin"
    write_lm(lm_path, g, 3, -6.0)
    phrases = random_phrases(np.random.default_rng(31 + W), tab, W, 12, 3)
    ref, stats = bbr.search(tab.joint, tab.T, W, N, S, prune=True, logsoftmax=tab.lp, phrases=bbr.Phrases(phrases), lm=ref_lm, weight=weight, bonus=bonus)
    got, nodes, pruned, _ = run_search(driver, tab, W, N, S, True, tmp_path, phrases, lm_path, weight, bonus)
    assert not pruned and not stats["pruned"]
    compare(got, ref, phrases, T, weight, bonus, True)
    for h in got:
        assert h["lm_final"] == ref_lm.score(h["tokens"])[0]


@pytest.mark.parametrize("T,W,N,S,NS,scale,bias", LATTICES)
def test_the_empty_set_equals_the_unboosted_search_bit_for_bit(driver, tmp_path, T, W, N, S, NS, scale, bias):
    rng = np.random.default_rng(1000 * T + 10 * W + S)
    tab = Table(peaky(rng, T, NS, scale, bias))
    g = lm_ref.random_lm(np.random.default_rng(5), 3, 30, tokens=lattice_tokens(tab, W)[:40], bos=True, eos=True, density=0.2)
    lm_path = tmp_path / "lm.bin"
    write_lm(lm_path, g, 3, -6.0)
    for lm, weight in (("-", 0.0), (lm_path, 0.7)):
        for prune in (False, True):
            plain, nodes_p, pruned_p, _ = run_search(driver, tab, W, N, S, prune, tmp_path, [], lm, weight, 0.0, mode="plain")
            got, nodes, pruned, states = run_search(driver, tab, W, N, S, prune, tmp_path, [], lm, weight, 0.0)
            assert states == 2 and pruned == pruned_p == prune and nodes == nodes_p and len(got) == len(plain)       # the empty set keeps the prune
            for h, f in zip(got, plain):
                assert (h["score"], h["tokens"], h["frames"], h["lp_bits"], h["lm"], h["lm_final"]) == (f["score"], f["tokens"], f["frames"], f["lp_bits"], f["lm"], f["lm_final"])
                assert h["boost"] == 0.0 and h["total"] == (f["total"] if lm != "-" else h["score"])


def test_prune_allowed(driver):
    r = subprocess.run([str(driver), "prune"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    for ln in r.stdout.strip().splitlines():
        tb, nonpos, states, allowed = (int(v) for v in ln.split())
        assert bool(allowed) == (tb == 0 and nonpos == 1 and states <= 2), ln


def test_a_phrase_completes_fails_midway_and_overlaps(driver, tmp_path):
    """hand-made dyadic ln P: the chain 100, 101, 102, 103 is likely.  (100, 101) completes; (101, 7) is paid for 101 and then fails -- the
    bonus stays; (101, 102, 103) overlaps the first phrase's end; after 100 101 the state is the longest match, and the bonus of 102 is the
    max over the failure chain.  A one-token phrase with a large bonus over an id outside every row's 8 largest is proposed and wins"""
    from tests.test_beam_math import chain_table
    tab = chain_table(2, 4)
    phrases = [((100, 101), 2.0), ((101, 7), 4.0), ((101, 102, 103), 1.0), ((102,), 0.5)]
    ref, stats = bbr.search(tab.joint, tab.T, 4, 4, 4, logsoftmax=tab.lp, phrases=bbr.Phrases(phrases))
    got, _, pruned, _ = run_search(driver, tab, 4, 4, 4, True, tmp_path, phrases)
    assert not pruned
    compare(got, ref, phrases, tab.T, 0.0, 0.0, False)
    top = got[0]
    assert top["tokens"] == [100, 101, 102, 103]
    assert top["bonuses"] == [2.0, 4.0, 1.0, 1.0]         # 100 starts (100, 101): 2; 101: max(2 completing, 4 starting (101, 7)); 102 and 103 continue the overlap; 7 never came: 4 is kept
    assert top["boost"] == 8.0 and top["depth"] == 3
    far = [((600,), 64.0)]
    assert all(600 not in br.top_order(tab.x[t, s])[:8] for t in range(tab.T) for s in range(tab.NS))
    ref, stats = bbr.search(tab.joint, tab.T, 4, 4, 4, logsoftmax=tab.lp, phrases=bbr.Phrases(far))
    got, _, _, _ = run_search(driver, tab, 4, 4, 4, True, tmp_path, far)
    compare(got, ref, far, tab.T, 0.0, 0.0, False)
    assert stats["proposed_by_boost"] >= 1 and 600 in got[0]["tokens"] and got[0]["boost"] == 64.0 * got[0]["tokens"].count(600)
