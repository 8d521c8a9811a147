"""Engine option "token_entropy" in the greedy decode's working set (csrc/nasr_decode_set.h).  No GPU: the header is compiled with the host
compiler under AddressSanitizer and UBSan, as tests/test_decode_set.py does, whose expected sizes of the other buffers are reused.

With DecFeatures::entropy_milli != 0: the LP kernels' buffers (lp_part, tok_logprob) and two more -- ent_part, P x 4 bytes beside lp_part
(P = max(64 x 65, rows x 17) parts), and tok_entropy, S x 4096 x 4 bytes; dec_set_bind sets both and ent_alpha = milli / 1000.  With 0:
the allocations, the slot layout and the bound DecParams are what they were before the option existed."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.test_decode_set import ALL, COMBOS, NONE, SIZINGS, TOK_CAP, bound_fields, parent_buffers
from tests.test_gemm_plan import HIP_STUB

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"

DRIVER = r"""
#include "nasr_internal.h"
#include "nasr_decode_set.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
using namespace nasr;
// one case per line of stdin: slots rows  <5 features> milli ->
//   "<name:bytes of every allocation> | <name:bytes per slot of dec_set_slot_layout> | <non-null DecParams pointer fields> | <ent_alpha %.9g> <lp_kernels> | ok or what is wrong"
static std::vector<void *> g_ptrs;
static std::string g_allocs;
static int rec_alloc(const char *name, void **p, size_t bytes) {
    *p = malloc(bytes ? bytes : 1);
    if (!*p) return -1;
    g_ptrs.push_back(*p);
    g_allocs += std::string(" ") + name + ":" + std::to_string(bytes);
    return 0;
}
static int refuse(const char *, int) { return -1; }
int main() {
    int slots, rows, lp, k, fb, pb, lm, milli;
    while (scanf("%d %d %d %d %d %d %d %d", &slots, &rows, &lp, &k, &fb, &pb, &lm, &milli) == 8) {
        DecFeatures f;
        f.token_logprobs = lp; f.alt_k = k; f.frame_blank = fb; f.phrase_boost = pb; f.lm_fusion = lm; f.entropy_milli = milli;
        DecodeSet d;
        g_allocs.clear();
        if (dec_set_ensure(d, f, slots, rows, rec_alloc, refuse)) return 3;
        printf("%s |", g_allocs.c_str());
        dec_set_slot_layout(d, f, [&](const char *name, auto *&p, bool, size_t per_slot) { printf(" %s:%zu", name, per_slot * sizeof(*p)); });
        static const float bonus = 0; static const int32_t next = 0; static const nasr_lm::Greedy blk = {};
        DecParams dp;
        dec_set_bind(d, f, DecTables{&bonus, &next, &blk}, dp);
        std::string bad;
        const struct { const char *name; const void *got, *want; } fields[] = {
            {"ctrl", dp.ctrl, d.ctrl}, {"h", dp.h, d.h}, {"c", dp.c, d.c}, {"predg", dp.predg, d.predg}, {"key", dp.key, d.key}, {"n_active", dp.n_active, d.n_active},
            {"n_dirty", dp.n_dirty, d.n_active + 1}, {"n_rows", dp.n_rows, d.n_active + 2}, {"dlist", dp.dlist, d.dlist}, {"rowmap", dp.rowmap, d.rowmap},
            {"tok_ring", dp.tok_ring, d.tok_ring}, {"tok_frame", dp.tok_frame, d.tok_frame}, {"lp_part", dp.lp_part, d.lp_part}, {"tok_logprob", dp.tok_logprob, d.tok_logprob},
            {"boost_bonus", dp.boost_bonus, &bonus}, {"boost_next", dp.boost_next, &next}, {"boost_state", dp.boost_state, d.boost_state}, {"boost_raw", dp.boost_raw, d.boost_raw},
            {"alt_key", dp.alt_key, d.alt_key}, {"alt_id", dp.alt_id, d.alt_id}, {"alt_lp", dp.alt_lp, d.alt_lp}, {"fb_row", dp.fb_row, d.fb_row},
            {"frame_blank", dp.frame_blank, d.frame_blank}, {"lm_blk", dp.lm_blk, &blk}, {"lm_state", dp.lm_state, d.lm_state}, {"lm_row", dp.lm_row, d.lm_row},
            {"lm_next", dp.lm_next, d.lm_next}, {"ent_part", dp.ent_part, d.ent_part}, {"tok_entropy", dp.tok_entropy, d.tok_entropy}};
        printf(" |");
        for (auto &fl : fields) {
            if (!fl.got) continue;
            printf(" %s", fl.name);
            if (fl.got != fl.want) bad += std::string(" ") + fl.name + " points elsewhere";
        }
        // the fields of the caller's stay zero, and the struct holds nothing this list does not name
        if (dp.rows || dp.B || dp.T || dp.encproj || dp.embed || dp.w_ih[0] || dp.out_b || dp.raw_logits) bad += " a field of the caller's is set";
        printf(" | %.9g %d | %s\n", (double)dp.ent_alpha, (int)f.lp_kernels(), bad.empty() ? "ok" : bad.c_str());
        for (void *p : g_ptrs) free(p);
        g_ptrs.clear();
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("ent_decode_set")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(HIP_STUB)
    (d / "drv.cpp").write_text(DRIVER)
    exe = d / "ent_decode_set"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{d}", f"-I{CSRC}", f"-I{ROOT / 'include'}", str(d / "drv.cpp"), "-o", str(exe)])

    def go(cases):
        text = "".join(" ".join(str(v) for v in c) + "\n" for c in cases)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
        out = []
        for ln in r.stdout.splitlines():
            allocs, slot, fields, tail, verdict = [p.split() for p in ln.split("|")]
            pairs = lambda xs: {x.split(":")[0]: int(x.split(":")[1]) for x in xs}
            out.append(dict(allocs=pairs(allocs), order=[x.split(":")[0] for x in allocs], slot=pairs(slot), fields=sorted(fields), alpha=float(tail[0]),
                            lp_kernels=int(tail[1]), verdict=" ".join(verdict)))
        assert len(out) == len(cases)
        return out
    return go


# what one slot owns of every per-slot buffer, in bytes (tests/test_fork_plan.py restates the same for the fork)
SLOT_BYTES = dict(ctrl=48, h=4 * 640 * 4, c=4 * 640 * 4, predg=640 * 4, dlist=4, tok_ring=TOK_CAP * 4, tok_frame=TOK_CAP * 4, tok_logprob=TOK_CAP * 4,
                  boost_state=4, frame_blank=4096 * 4, lm_state=4, lm_row=1040 * 4, lm_next=1040 * 4, tok_entropy=TOK_CAP * 4)


def slot_part(buffers, k):
    out = {n: SLOT_BYTES[n] for n in buffers if n in SLOT_BYTES}
    if k:
        out.update(alt_id=TOK_CAP * k * 4, alt_lp=TOK_CAP * k * 4)
    return out


def test_buffers_appear_exactly_with_the_option(run):
    cases = [(name, f, milli) for name in SIZINGS for f in COMBOS for milli in (0, 333, 1000)]
    got = run([SIZINGS[name] + f + (milli,) for name, f, milli in cases])
    for (name, f, milli), g in zip(cases, got):
        S, M = SIZINGS[name]
        P = max(64 * 65, M * 17)
        want = parent_buffers(S, M, *f)                                # what the parent commit allocates under the five older options
        if milli:
            want = parent_buffers(S, M, 1, *f[1:])                     # the LP kernels' buffers come with it
            want.update(ent_part=P * 4, tok_entropy=S * TOK_CAP * 4)
        assert g["verdict"] == "ok", (name, f, milli, g["verdict"])
        assert g["allocs"] == want, (name, f, milli)
        assert g["lp_kernels"] == (1 if milli or f[0] or f[1] or f[2] else 0)
        # one slot's part: tok_entropy is in it, the scratch ent_part is not
        assert g["slot"] == slot_part(want, f[1]), (name, f, milli)
        assert ("tok_entropy" in g["slot"]) == bool(milli) and "ent_part" not in g["slot"] and "lp_part" not in g["slot"]
        # bind
        fields = bound_fields(*f)
        if milli:
            fields = sorted(set(fields) | {"lp_part", "tok_logprob", "ent_part", "tok_entropy"})
        assert g["fields"] == fields, (name, f, milli)
        assert np.float32(g["alpha"]) == np.float32(milli) / np.float32(1000.0)          # printed with 9 digits: an f32, exactly


def test_option_off_is_the_layout_of_today(run):
    """the allocation order of the older buffers does not move, and the two new ones come last"""
    S, M = SIZINGS["engine, 64 streams (R = 13: 896 rows a step)"]
    off, on = run([(S, M) + ALL + (0,), (S, M) + ALL + (333,)])
    assert on["order"][:len(off["order"])] == off["order"] and on["order"][len(off["order"]):] == ["ent_part", "tok_entropy"]
    assert off["order"] == ["ctrl", "h", "c", "predg", "key", "n_active", "dlist", "rowmap", "tok_ring", "tok_frame", "lp_part", "tok_logprob", "boost_state", "boost_raw",
                            "alt_key", "alt_id", "alt_lp", "fb_row", "frame_blank", "lm_state", "lm_row", "lm_next"]
    none, = run([(S, M) + NONE + (0,)])
    assert none["fields"] == bound_fields(*NONE) and none["alpha"] == 0.0 and none["lp_kernels"] == 0
