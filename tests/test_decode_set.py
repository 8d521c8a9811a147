"""The greedy decode's working set (nemotron-asr.cpp_amd/csrc/nasr_decode_set.h: DecFeatures, DecodeSet, dec_set_ensure, dec_set_bind).
No GPU: the header is compiled with the host compiler under AddressSanitizer and UBSan into a stand-alone program whose allocator is
malloc and records (buffer name, bytes), like tests/test_small_step_plan.py.

Expected sizes are the formulas of the two sites the header replaced, restated here and not read from it:
  * the live engine (engine_create + the option branches of nasr_engine_set_option), S = max_streams slots, M = w_rows =
    max(max_streams x 14, 256) rows:  ctrl S x 48 bytes, h and c S x 4 x 640 f32, predg S x 640 f32, key M x 8, n_active 16 bytes,
    dlist S x 4, rowmap M x 4, tok_ring and tok_frame S x 4096 x 4;  with any of "token_logprobs" / "token_alternatives" /
    "frame_blank_logprobs": lp_part P x 8 with P = max(64 x 65, M x 17) and tok_logprob S x 4096 x 4;  "token_alternatives" = K: alt_key
    P x K x 8, alt_id and alt_lp S x 4096 x K x 4;  "frame_blank_logprobs": fb_row M x 4, frame_blank S x 4096 x 4;  "phrase_boost":
    boost_state S x 4 and boost_raw P x 4;  "lm_fusion": lm_state S x 4, lm_row and lm_next S x 1040 x 4, and boost_raw
  * the offline path (ensure_rows): the same formulas at S = 256 utterances and M = 256 x 256 window rows
"""
import itertools
import shutil
import subprocess
from pathlib import Path

import pytest

from tests.test_gemm_plan import HIP_STUB

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"

DRIVER = r"""
#include "nasr_internal.h"
#include "nasr_decode_set.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>
using namespace nasr;
// one case per line of stdin (a feature set = token_logprobs alt_k frame_blank phrase_boost lm_fusion), one answer per line of stdout:
//   E slots rows n <n feature sets>     dec_set_ensure once per feature set on one DecodeSet ->
//       "<rc of every call> | <1 if a buffer that existed moved> | <name:bytes of every allocation, in order> | <non-null buffers> | <set.alt_k> | <last message>"
//   B slots rows <ensured set> <bound set>   dec_set_ensure, then dec_set_bind -> "<non-null DecParams fields> | alt_k lm_fold lm_relook | <ok or what is wrong>"
static std::vector<std::pair<std::string, size_t>> g_recs;
static std::vector<void *> g_ptrs;
static int rec_alloc(const char *name, void **p, size_t bytes) {
    *p = malloc(bytes ? bytes : 1);
    if (!*p) return -1;
    g_ptrs.push_back(*p);
    g_recs.push_back({name, bytes});
    return 0;
}
static char g_err[160];
static int refuse(const char *fmt, int v) { snprintf(g_err, sizeof(g_err), fmt, v); return -1; }
static bool read_features(DecFeatures &f) {
    int lp, k, fb, pb, lm;
    if (scanf("%d %d %d %d %d", &lp, &k, &fb, &pb, &lm) != 5) return false;
    f.token_logprobs = lp; f.alt_k = k; f.frame_blank = fb; f.phrase_boost = pb; f.lm_fusion = lm;
    return true;
}
static std::map<std::string, const void *> pointers(DecodeSet &d) {
    std::map<std::string, const void *> m;
    dec_set_layout(d, DecFeatures(), 1, 1, [&](const char *name, auto *&p, bool, size_t) { m[name] = p; });
    return m;
}
int main() {
    char op;
    while (scanf(" %c", &op) == 1) {
        int slots, rows;
        if (scanf("%d %d", &slots, &rows) != 2) return 2;
        DecodeSet d;
        g_err[0] = 0;
        g_recs.clear();
        if (op == 'E') {
            int n, moved = 0;
            if (scanf("%d", &n) != 1) return 2;
            for (int i = 0; i < n; i++) {
                DecFeatures f;
                if (!read_features(f)) return 2;
                const auto before = pointers(d);
                printf("%d ", dec_set_ensure(d, f, slots, rows, rec_alloc, refuse));
                const auto after = pointers(d);
                for (auto &kv : before) if (kv.second && after.at(kv.first) != kv.second) moved = 1;
            }
            printf("| %d |", moved);
            for (auto &r : g_recs) printf(" %s:%zu", r.first.c_str(), r.second);
            printf(" |");
            for (auto &kv : pointers(d)) if (kv.second) printf(" %s", kv.first.c_str());
            printf(" | %d | %s\n", d.alt_k, g_err);
        } else if (op == 'B') {
            DecFeatures fe, fb;
            if (!read_features(fe) || !read_features(fb)) return 2;
            fb.lm_fold = 1; fb.lm_relook = 1;
            if (dec_set_ensure(d, fe, slots, rows, rec_alloc, refuse)) return 3;
            static const float bonus = 0; static const int32_t next = 0; static const nasr_lm::Greedy blk = {};
            DecParams dp;
            dec_set_bind(d, fb, DecTables{&bonus, &next, &blk}, dp);
            std::string bad;
            const struct { const char *name; const void *got, *want; } fields[] = {
                {"ctrl", dp.ctrl, d.ctrl}, {"h", dp.h, d.h}, {"c", dp.c, d.c}, {"predg", dp.predg, d.predg}, {"key", dp.key, d.key}, {"n_active", dp.n_active, d.n_active},
                {"n_dirty", dp.n_dirty, d.n_active + 1}, {"n_rows", dp.n_rows, d.n_active + 2}, {"dlist", dp.dlist, d.dlist}, {"rowmap", dp.rowmap, d.rowmap},
                {"tok_ring", dp.tok_ring, d.tok_ring}, {"tok_frame", dp.tok_frame, d.tok_frame}, {"lp_part", dp.lp_part, d.lp_part}, {"tok_logprob", dp.tok_logprob, d.tok_logprob},
                {"boost_bonus", dp.boost_bonus, &bonus}, {"boost_next", dp.boost_next, &next}, {"boost_state", dp.boost_state, d.boost_state}, {"boost_raw", dp.boost_raw, d.boost_raw},
                {"alt_key", dp.alt_key, d.alt_key}, {"alt_id", dp.alt_id, d.alt_id}, {"alt_lp", dp.alt_lp, d.alt_lp}, {"fb_row", dp.fb_row, d.fb_row},
                {"frame_blank", dp.frame_blank, d.frame_blank}, {"lm_blk", dp.lm_blk, &blk}, {"lm_state", dp.lm_state, d.lm_state}, {"lm_row", dp.lm_row, d.lm_row},
                {"lm_next", dp.lm_next, d.lm_next}};
            for (auto &f : fields) {
                if (!f.got) continue;
                printf("%s ", f.name);
                if (f.got != f.want) bad += std::string(" ") + f.name + " points elsewhere";
            }
            if (dp.rows || dp.B || dp.T || dp.encproj || dp.embed || dp.w_ih[0] || dp.out_b || dp.raw_logits) bad += " a field of the caller's is set";
            printf("| %d %d %d | %s\n", dp.alt_k, dp.lm_fold, dp.lm_relook, bad.empty() ? "ok" : bad.c_str());
        } else return 2;
        for (void *p : g_ptrs) free(p);
        g_ptrs.clear();
    }
    return 0;
}
"""

BASE = ["ctrl", "h", "c", "predg", "key", "n_active", "dlist", "rowmap", "tok_ring", "tok_frame"]
TOK_CAP = FRAME_CAP = 4096


def engine_sizing(max_streams):
    return max_streams, max(max_streams * 14, 256)


SIZINGS = {"engine, 1 stream": engine_sizing(1), "engine, 64 streams (R = 13: 896 rows a step)": engine_sizing(64), "offline": (256, 256 * 256)}
COMBOS = list(itertools.product((0, 1), (0, 1, 8), (0, 1), (0, 1), (0, 1)))          # token_logprobs, alt_k, frame_blank, phrase_boost, lm_fusion
NONE, ALL = (0, 0, 0, 0, 0), (1, 8, 1, 1, 1)


def parent_buffers(S, M, lp, k, fb, pb, lm):
    """name -> bytes: the docstring's formulas"""
    P = max(64 * 65, M * 17)
    b = dict(ctrl=S * 48, h=S * 4 * 640 * 4, c=S * 4 * 640 * 4, predg=S * 640 * 4, key=M * 8, n_active=16, dlist=S * 4, rowmap=M * 4,
             tok_ring=S * TOK_CAP * 4, tok_frame=S * TOK_CAP * 4)
    if lp or k or fb:
        b.update(lp_part=P * 8, tok_logprob=S * TOK_CAP * 4)
    if k:
        b.update(alt_key=P * k * 8, alt_id=S * TOK_CAP * k * 4, alt_lp=S * TOK_CAP * k * 4)
    if fb:
        b.update(fb_row=M * 4, frame_blank=S * FRAME_CAP * 4)
    if pb:
        b.update(boost_state=S * 4, boost_raw=P * 4)
    if lm:
        b.update(lm_state=S * 4, lm_row=S * 1040 * 4, lm_next=S * 1040 * 4, boost_raw=P * 4)
    return b


@pytest.fixture(scope="module")
def decode_set(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("decode_set")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(HIP_STUB)
    (d / "drv.cpp").write_text(DRIVER)
    exe = d / "decode_set"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{d}", f"-I{CSRC}", f"-I{ROOT / 'include'}", str(d / "drv.cpp"), "-o", str(exe)])

    def run(cases):
        text = "".join(" ".join(str(v) for v in c) + "\n" for c in cases)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
        out = [[part.split() for part in ln.split("|")] for ln in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return run


def ensure_case(S, M, steps):
    return ("E", S, M, len(steps)) + tuple(v for f in steps for v in f)


def parse_ensure(ans):
    rcs, moved, allocs, nonnull, alt_k = ans[:5]
    allocs = [(a.split(":")[0], int(a.split(":")[1])) for a in allocs]
    assert len({n for n, _ in allocs}) == len(allocs)              # no buffer allocated twice
    return [int(r) for r in rcs], int(moved[0]), dict(allocs), sorted(nonnull), int(alt_k[0]), " ".join(ans[5])


def test_one_call_allocates_what_the_parent_allocated(decode_set):
    cases = [(name, f) for name in SIZINGS for f in COMBOS]
    assert len(COMBOS) == 48
    got = decode_set([ensure_case(*SIZINGS[name], [f]) for name, f in cases])
    for (name, f), ans in zip(cases, got):
        rcs, moved, allocs, nonnull, alt_k, _ = parse_ensure(ans)
        want = parent_buffers(*SIZINGS[name], *f)
        assert rcs == [0] and not moved and alt_k == f[1], (name, f)
        assert allocs == want, (name, f)
        assert nonnull == sorted(want), (name, f)


def test_the_order_of_the_options_does_not_matter(decode_set):
    """dec_set_ensure after every option, in every order of the five (as nasr_engine_set_option calls it, the set starting from the base part
    engine_create allocated): the same buffers and sizes as one call with all of them, nothing allocated twice, nothing moved"""
    orders = list(itertools.permutations(range(5)))
    assert len(orders) == 120
    cases = []
    for name in SIZINGS:
        for order in orders:
            steps, f = [NONE], list(NONE)
            for i in order:
                f[i] = ALL[i]
                steps.append(tuple(f))
            cases.append((name, order, steps))
    got = decode_set([ensure_case(*SIZINGS[name], steps) for name, _, steps in cases])
    for (name, order, steps), ans in zip(cases, got):
        rcs, moved, allocs, nonnull, alt_k, _ = parse_ensure(ans)
        want = parent_buffers(*SIZINGS[name], *ALL)
        assert rcs == [0] * 6 and not moved and alt_k == 8, (name, order)
        assert allocs == want and nonnull == sorted(want), (name, order)
        assert list(allocs)[:len(BASE)] == BASE                    # the first call allocated the base part and nothing else


def bound_fields(lp, k, fb, pb, lm):
    names = BASE + ["n_dirty", "n_rows"]
    if lp or k or fb:
        names += ["lp_part", "tok_logprob"]
    if k:
        names += ["alt_key", "alt_id", "alt_lp"]
    if fb:
        names += ["fb_row", "frame_blank"]
    if pb:
        names += ["boost_bonus", "boost_next", "boost_state"]
    if lm:
        names += ["lm_blk", "lm_state", "lm_row", "lm_next"]
    if pb or lm:
        names += ["boost_raw"]
    return sorted(names)


def test_bind_follows_the_features_not_the_buffers(decode_set):
    """every buffer exists (all five options were set once); what a DecParams gets is decided by the features it is bound for -- as when
    "phrase_boost" is set and cleared again before the first step"""
    S, M = SIZINGS["engine, 1 stream"]
    got = decode_set([("B", S, M) + ALL + f for f in COMBOS if f[1] in (0, 8)] + [("B", S, M) + (1, 1, 1, 1, 1) + f for f in COMBOS if f[1] == 1])
    order = [f for f in COMBOS if f[1] in (0, 8)] + [f for f in COMBOS if f[1] == 1]
    by = {}
    for f, (fields, ints, verdict) in zip(order, got):
        assert verdict == ["ok"], (f, verdict)
        assert sorted(fields) == bound_fields(*f), f
        assert [int(v) for v in ints] == [f[1], 1 if f[4] else 0, 1 if f[4] else 0], f          # alt_k; lm_fold and lm_relook ride with "lm_fusion"
        by[f] = set(fields)
    assert "boost_raw" in by[(0, 0, 0, 0, 1)] and not by[(0, 0, 0, 0, 1)] & {"boost_state", "boost_bonus", "boost_next"}          # "lm_fusion" alone
    for alone in ((0, 1, 0, 0, 0), (0, 8, 0, 0, 0), (0, 0, 1, 0, 0)):                                                                # alt_k or frame_blank alone
        assert {"lp_part", "tok_logprob"} <= by[alone]
    assert by[NONE] == set(BASE + ["n_dirty", "n_rows"])
    # ... and a set that only has the base part binds exactly that for all-off features (the align path)
    (fields, ints, verdict), = decode_set([("B", S, M) + NONE + NONE])
    assert verdict == ["ok"] and sorted(fields) == bound_fields(*NONE) and [int(v) for v in ints] == [0, 0, 0]


def test_a_second_alt_k_is_refused(decode_set):
    S, M = SIZINGS["engine, 64 streams (R = 13: 896 rows a step)"]
    (a, b, c) = decode_set([ensure_case(S, M, [NONE, (0, 4, 0, 0, 0), (0, 8, 0, 0, 0)]), ensure_case(S, M, [(1, 4, 0, 0, 0), (1, 0, 0, 0, 0), (1, 4, 1, 0, 0)]),
                            ensure_case(S, M, [(0, 8, 0, 0, 0), (0, 1, 0, 1, 1)])])
    rcs, moved, allocs, nonnull, alt_k, err = parse_ensure(a)
    assert rcs == [0, 0, -1] and not moved and alt_k == 4
    assert err == "token_alternatives: the rings already hold 4 entries per token"
    assert allocs == parent_buffers(S, M, 0, 4, 0, 0, 0)           # the refused call allocated nothing
    rcs, moved, allocs, nonnull, alt_k, err = parse_ensure(b)      # off and on again at the same K is no change
    assert rcs == [0, 0, 0] and not moved and alt_k == 4 and err == "" and allocs == parent_buffers(S, M, 1, 4, 1, 0, 0)
    rcs, moved, allocs, nonnull, alt_k, err = parse_ensure(c)      # a refusal comes before any allocation of the same call
    assert rcs == [0, -1] and alt_k == 8 and allocs == parent_buffers(S, M, 0, 8, 0, 0, 0) and "already hold 8" in err
