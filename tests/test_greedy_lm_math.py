"""The bias arithmetic of the greedy decode's LM fusion (nasr_lm.h: Greedy, greedy_start, lmbias; engine option "lm_fusion"), compiled with g++
under AddressSanitizer / UBSan into a stand-alone driver -- no GPU.  The refresh kernel, the host and the GPU tests share this one statement.

For random models -- order 1 and order 5, with and without BOS n-grams, a table at its smallest capacity, one positive back-off -- the driver
writes lmbias(state, v) and the next state for EVERY state of the compiled model and every column v in 0 .. 1039; each is compared bit for
bit with the numpy restatement lmbias_ref below over tests/lm_ref.py (the recursive ARPA definition): the f32 weight times the double lookup,
rounded, plus the f32 bonus, rounded, then rounded to f32 -- Python floats are IEEE doubles and never fuse the two.  Weight 0 / bonus 0 gives
+0.0 everywhere (bits 0, not -0.0); the disabled state and a detached model give zeros and leave the state alone."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import lm_ref
from tests.test_lm_math import write_lm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"
BOS, EOS = lm_ref.BOS, lm_ref.EOS
COLS, N_TOKENS, DISABLED = 1040, 1024, -1

DRIVER = r"""
#include "nasr_lm.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
// model file: that of tests/test_lm_math.py.  Output: i32 start, i32 start_disabled, then records {i32 n-gram index (-1: the empty context, -2: the
// disabled state), i32 state, u32 bias bits[1040], i32 next[1040]} for every n-gram shorter than the order, the empty context and the disabled state
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
        for (int j = 0; j < l; j++) { int32_t t; if (fread(&t, 4, 1, f) != 1) return -2; tok.push_back(t); }
        float a, b;
        if (fread(&a, 4, 1, f) != 1 || fread(&b, 4, 1, f) != 1) return -2;
        lp.push_back(a); bo.push_back(b);
    }
    fclose(f);
    return nasr_lm::build(order, n, len.data(), tok.data(), lp.data(), bo.data(), unk, m, err, tight != 0);
}
static void record(FILE *out, const nasr_lm::Greedy &g, int32_t index, int32_t state) {
    std::vector<uint32_t> bits(nasr_lm::ROW_COLS);
    std::vector<int32_t> next(nasr_lm::ROW_COLS);
    for (int v = 0; v < nasr_lm::ROW_COLS; v++) {
        const float b = nasr_lm::lmbias(g, state, v, &next[v]);
        memcpy(&bits[v], &b, 4);
    }
    fwrite(&index, 4, 1, out); fwrite(&state, 4, 1, out);
    fwrite(bits.data(), 4, bits.size(), out); fwrite(next.data(), 4, next.size(), out);
}
int main(int argc, char **argv) {
    if (argc < 5) return 1;
    nasr_lm::Model m;
    std::string err;
    std::vector<int32_t> len, tok;
    const bool have_lm = strcmp(argv[1], "-") != 0;
    if (have_lm && read_lm(argv[1], m, err, len, tok)) { fprintf(stderr, "error: %s\n", err.c_str()); return 3; }
    nasr_lm::Greedy g = {};
    if (have_lm) { g.lm = m.view(); g.attached = 1; }
    g.weight = strtof(argv[2], nullptr); g.token_bonus = strtof(argv[3], nullptr);
    FILE *out = fopen(argv[4], "wb");
    if (!out) return 2;
    const int32_t s_on = nasr_lm::greedy_start(g, true), s_off = nasr_lm::greedy_start(g, false);
    fwrite(&s_on, 4, 1, out); fwrite(&s_off, 4, 1, out);
    size_t at = 0;
    for (size_t i = 0; have_lm && i < len.size(); at += (size_t)len[i], i++) {
        if (len[i] >= m.order) continue;
        int32_t st = 0;
        for (int j = 0; j < len[i]; j++) nasr_lm::lookup(g.lm, st, tok[at + (size_t)j], &st);
        record(out, g, (int32_t)i, st);
    }
    record(out, g, -1, 0);
    record(out, g, -2, nasr_lm::STATE_DISABLED);
    fclose(out);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("greedy_lm_math")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", "-o", str(exe), str(src)])
    return exe


def lmbias_ref(ref, history, v, weight, bonus):
    """the definition: (float)((double)weight * lookup + (double)token_bonus), product and sum rounded on their own; 0 for blank and the padding"""
    if v >= N_TOKENS:
        return np.float32(0.0)
    a = float(np.float32(weight)) * ref.term(history, v)
    return np.float32(a + float(np.float32(bonus)))


def run_driver(driver, tmp_path, model, weight, bonus):
    out = tmp_path / "rows.bin"
    r = subprocess.run([str(driver), str(model), repr(float(weight)), repr(float(bonus)), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.fromfile(out, np.int32)
    start, start_off = int(raw[0]), int(raw[1])
    rec = raw[2:].reshape(-1, 2 + 2 * COLS)
    return start, start_off, [(int(x[0]), int(x[1]), x[2:2 + COLS].view(np.uint32), x[2 + COLS:]) for x in rec]


def check_model(driver, tmp_path, ngrams, order, unk, weight, bonus, tight=False):
    """every (state, column) of the compiled model against the restatement; -> (states checked, values checked)"""
    path = tmp_path / "lm.bin"
    items = write_lm(path, ngrams, order, unk, tight)
    ref = lm_ref.RefLM(ngrams, order, unk)
    start, start_off, recs = run_driver(driver, tmp_path, path, weight, bonus)
    ctx_of = {-1: ()}
    for i, (k, _, _) in enumerate(items):
        ctx_of[i] = k
    state_of = {ctx_of[i]: st for i, st, _, _ in recs if i >= -1}
    assert len(set(state_of.values())) == len(state_of)
    assert start == state_of.get((BOS,), 0) and start_off == DISABLED
    n = 0
    for i, st, bits, nxt in recs:
        if i == -2:
            assert st == DISABLED and not bits.any() and (nxt == DISABLED).all()
            continue
        ctx = ctx_of[i]
        want = np.asarray([lmbias_ref(ref, ctx, v, weight, bonus) for v in range(COLS)], np.float32).view(np.uint32)
        bad = np.nonzero(want != bits)[0]
        assert bad.size == 0, (ctx, int(bad[0]), bits[bad[0]], want[bad[0]])
        assert [int(x) for x in nxt[:N_TOKENS]] == [state_of[ref.context_after(ctx, v)] for v in range(N_TOKENS)], ctx
        assert (nxt[N_TOKENS:] == st).all()                    # blank and the padding: never emitted, the state stays
        n += COLS
    return len(recs) - 1, n


CASES = [(1, 12, False, False), (1, 12, True, False), (5, 10, True, False), (5, 10, False, True), (3, 17, True, True), (2, 9, False, False)]


@pytest.mark.parametrize("order,n_tok,bos,pos", CASES)
def test_every_state_and_column_against_the_restatement(driver, tmp_path, order, n_tok, bos, pos):
    rng = np.random.default_rng(4000 + 100 * order + n_tok + 7 * bos + pos)
    g = lm_ref.random_lm(rng, order, n_tok, bos=bos, eos=bool(order & 1), positive_backoff=pos, max_per_level=30)
    assert any(k[0] == BOS for k in g) == bos
    if pos and order > 1:
        assert sum(1 for _, bo in g.values() if bo > 0) >= 1
    states, n = check_model(driver, tmp_path, g, order, -7.5, 0.7, 1.25)
    assert states >= (2 if order > 1 else 1) and n == states * COLS      # at order 1 the empty context is the only state
    check_model(driver, tmp_path, g, order, -7.5, 100.0, 0.0)   # the largest weight, no bonus


def test_exactly_one_positive_backoff(driver, tmp_path):
    g = lm_ref.random_lm(np.random.default_rng(77), 3, 8, bos=True, eos=False, positive_backoff=False, max_per_level=30)
    k = next(k for k in g if len(k) == 2)
    g[k] = (g[k][0], lm_ref.f32(0.375))
    assert sum(1 for _, bo in g.values() if bo > 0) == 1
    check_model(driver, tmp_path, g, 3, -6.0, 0.5, 0.25)


def test_smallest_arc_capacity(driver, tmp_path):
    """capacity = the smallest power of two above the arc count: long probe sequences, some wrapping around the table's end"""
    g = lm_ref.random_lm(np.random.default_rng(901), 3, 24, positive_backoff=True, max_per_level=60)
    states, _ = check_model(driver, tmp_path, g, 3, -9.0, 0.3, 2.0, tight=True)
    assert states > 20


def test_weight_zero_and_bonus_zero_give_plus_zero_everywhere(driver, tmp_path):
    g = lm_ref.random_lm(np.random.default_rng(5), 4, 12, positive_backoff=True, max_per_level=30)
    path = tmp_path / "lm.bin"
    write_lm(path, g, 4, -6.0)
    _, _, recs = run_driver(driver, tmp_path, path, 0.0, 0.0)
    assert len(recs) > 10
    for _, _, bits, _ in recs:
        assert not bits.any()                                  # 0x00000000: + 0.0, never - 0.0 (0 * a negative lookup is - 0.0; + 0.0 makes it + 0.0)
    check_model(driver, tmp_path, g, 4, -6.0, 0.0, 0.0)         # ... and the next states are the model's all the same


def test_detached_model_and_disabled_state_give_zeros(driver, tmp_path):
    start, start_off, recs = run_driver(driver, tmp_path, "-", 3.0, 2.0)
    assert start == 0 and start_off == DISABLED and [r[0] for r in recs] == [-1, -2]
    for _, st, bits, nxt in recs:
        assert not bits.any() and (nxt == st).all()            # no bias, and the state never moves
