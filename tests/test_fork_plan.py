"""The copy plan of a stream fork (nemotron-asr.cpp_amd/csrc/nasr_fork_plan.h) and the per-slot part of the decode set's layout
(dec_set_slot_layout, nasr_decode_set.h).  No GPU: the headers are compiled with the host compiler under AddressSanitizer and UBSan
into a stand-alone program, like tests/test_decode_set.py.

What a fork must copy is restated here and not read from the header: per layer and plane the 70 K/V window rows (kv_head + j) % 326 at
the same ring indices, both parities of the conv cache (2 x (ks - 1) x 1024 floats), mel frames mel_start .. mel_start + mel_count - 1
mod 4096, abuf_cnt samples of parity abuf_par rounded up to 16 bytes, last_sample, both parities of the converter's history (2 x 193
floats), and of the decoder every per-slot buffer the features need: ctrl 48 bytes, h and c 4 x 640 f32, predg 640 f32, tok_ring and
tok_frame 4096 x 4; with any LP option tok_logprob 4096 x 4; "token_alternatives" = K: alt_id and alt_lp 4096 x K x 4;
"frame_blank_logprobs": frame_blank 4096 x 4; "phrase_boost": boost_state 4; "lm_fusion": lm_state 4, lm_row and lm_next 1040 x 4.
Scratch (key, rowmap, dlist, n_active, lp_part, boost_raw, alt_key, fb_row) is not copied."""
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
#include "nasr_fork_plan.h"
#include <cstdio>
#include <map>
#include <string>
#include <vector>
using namespace nasr;
// one case per line of stdin (a feature set = token_logprobs alt_k frame_blank phrase_boost lm_fusion), one answer per line of stdout:
//   L <features>     "<name:elements at 1 slot:elements at 2 slots:needed of dec_set_layout> | <name:elements per slot:element bytes of dec_set_slot_layout>"
//   P kv_head mel_start mel_count abuf_cnt abuf_par esz n_layers ks src_slot dst_slot <features>
//                    "<buf:layer:name:src:dst:bytes:slot_bytes of every segment> | <plan_fault or ok> | <pieces> <largest> <bytes in pieces> <pieces that leave their segment>"
static bool read_features(DecFeatures &f) {
    int lp, k, fb, pb, lm;
    if (scanf("%d %d %d %d %d", &lp, &k, &fb, &pb, &lm) != 5) return false;
    f.token_logprobs = lp; f.alt_k = k; f.frame_blank = fb; f.phrase_boost = pb; f.lm_fusion = lm;
    return true;
}
int main() {
    char op;
    while (scanf(" %c", &op) == 1) {
        DecodeSet d;
        DecFeatures f;
        if (op == 'L') {
            if (!read_features(f)) return 2;
            std::vector<std::string> names;
            std::vector<size_t> one, two;
            std::vector<int> need;
            dec_set_layout(d, f, 1, 5, [&](const char *name, auto *&, bool needed, size_t n) { names.push_back(name); one.push_back(n); need.push_back(needed); });
            dec_set_layout(d, f, 2, 5, [&](const char *, auto *&, bool, size_t n) { two.push_back(n); });
            for (size_t i = 0; i < names.size(); i++) printf("%s:%zu:%zu:%d ", names[i].c_str(), one[i], two[i], need[i]);
            printf("|");
            dec_set_slot_layout(d, f, [&](const char *name, auto *&p, bool needed, size_t n) { printf(" %s:%zu:%zu:%d", name, n, sizeof(*p), (int)needed); });
            printf("\n");
        } else if (op == 'P') {
            nasr_fork::Source m;
            int esz, n_layers, ks, src_slot, dst_slot;
            if (scanf("%d %d %d %d %d %d %d %d %d %d", &m.kv_head, &m.mel_start, &m.mel_count, &m.abuf_cnt, &m.abuf_par, &esz, &n_layers, &ks, &src_slot, &dst_slot) != 10) return 2;
            if (!read_features(f)) return 2;
            const std::vector<nasr_fork::Seg> segs = nasr_fork::fork_plan(m, src_slot, dst_slot, esz, n_layers, ks, d, f);
            for (const auto &s : segs) printf("%d:%d:%s:%lld:%lld:%lld:%lld ", s.buf, s.layer, s.name, (long long)s.src, (long long)s.dst, (long long)s.bytes, (long long)s.slot_bytes);
            const char *fault = nasr_fork::plan_fault(segs, src_slot, dst_slot);
            long long n_pieces = 0, largest = 0, total = 0, outside = 0;
            for (const auto &s : segs) {
                std::vector<nasr_fork::Piece> pieces;
                nasr_fork::cut_pieces(pieces, s, nullptr, nasr_fork::PIECE_BYTES);
                for (const auto &p : pieces) {
                    const long long ps = (long long)(intptr_t)p.src, pd = (long long)(intptr_t)p.dst;
                    n_pieces++; total += p.bytes;
                    if (p.bytes > largest) largest = p.bytes;
                    if (ps < s.src || ps + p.bytes > s.src + s.bytes || pd - ps != s.dst - s.src) outside++;
                }
            }
            printf("| %s | %lld %lld %lld %lld\n", fault ? fault : "ok", n_pieces, largest, total, outside);
        } else return 2;
    }
    return 0;
}
"""

COMBOS = list(itertools.product((0, 1), (0, 1, 8), (0, 1), (0, 1), (0, 1)))          # tests/test_decode_set.py's grid
ALL = (1, 8, 1, 1, 1)
KVC, LCTX, D, MEL_RING, NMEL, ABUF_CAP, HIST_MAX, TOK_CAP = 326, 70, 1024, 4096, 128, 1280 * 256 + 512 + 64, 193, 4096
BUF_KV, BUF_CC, BUF_MEL, BUF_ABUF, BUF_LAST, BUF_HIST, BUF_DEC = range(7)
WORD_ITEMS = {"last_sample", "aud_hist", "boost_state", "lm_state"}
SCRATCH = {"key", "rowmap", "dlist", "n_active", "lp_part", "boost_raw", "alt_key", "fb_row"}


def slot_bytes_of_the_decoder(lp, k, fb, pb, lm):
    """name -> bytes one slot owns: the docstring's list"""
    b = dict(ctrl=48, h=4 * 640 * 4, c=4 * 640 * 4, predg=640 * 4, tok_ring=TOK_CAP * 4, tok_frame=TOK_CAP * 4)
    if lp or k or fb:
        b.update(tok_logprob=TOK_CAP * 4)
    if k:
        b.update(alt_id=TOK_CAP * k * 4, alt_lp=TOK_CAP * k * 4)
    if fb:
        b.update(frame_blank=4096 * 4)
    if pb:
        b.update(boost_state=4)
    if lm:
        b.update(lm_state=4, lm_row=1040 * 4, lm_next=1040 * 4)
    return b


@pytest.fixture(scope="module")
def fork_plan(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("fork_plan")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(HIP_STUB)
    (d / "drv.cpp").write_text(DRIVER)
    exe = d / "fork_plan"
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


def test_slot_layout_is_the_per_slot_part_of_the_full_layout(fork_plan):
    """dec_set_slot_layout lists a buffer with n elements per slot exactly when dec_set_layout's element count for it at 2 slots minus that at
    1 slot is n > 0 and its option is needed -- and nothing else.  The byte sizes are the docstring's; the only buffer sized by the slots that
    is no state is dlist (a list by position), which the plan leaves out by name"""
    assert len(COMBOS) == 48
    for f, (full, slot) in zip(COMBOS, fork_plan([("L",) + f for f in COMBOS])):
        want = {}
        for rec in full:
            name, one, two, needed = rec.split(":")
            if int(two) - int(one) > 0 and int(needed):
                want[name] = int(two) - int(one)
        got = {}
        for rec in slot:
            name, n, esz, needed = rec.split(":")
            assert name not in got and int(needed) == 1, (f, name)
            got[name] = (int(n), int(esz))
        assert {k: v[0] for k, v in got.items()} == want, f
        by_bytes = {k: n * esz for k, (n, esz) in got.items() if k != "dlist"}
        assert by_bytes == slot_bytes_of_the_decoder(*f), f
        assert got["dlist"] == (1, 4) and not set(got) & (SCRATCH - {"dlist"})


def plan_case(kv_head, mel, abuf_cnt, abuf_par, esz, f, n_layers=3, ks=9, src_slot=1, dst_slot=4):
    return ("P", kv_head, mel[0], mel[1], abuf_cnt, abuf_par, esz, n_layers, ks, src_slot, dst_slot) + tuple(f)


def parse_plan(ans):
    segs = []
    for rec in ans[0]:
        buf, layer, name, src, dst, nbytes, slot_bytes = rec.split(":")
        segs.append(dict(buf=int(buf), layer=int(layer), name=name, src=int(src), dst=int(dst), bytes=int(nbytes), slot_bytes=int(slot_bytes)))
    return segs, " ".join(ans[1]), [int(v) for v in ans[2]]


def ring_rows_covered(segs, slot, slot_bytes, at, row_bytes, ring):
    """ring rows the segments of one ring cover, from their source offsets; the destination is the same place of the other slot"""
    rows = []
    for s in segs:
        rel = s["src"] - slot * slot_bytes - at
        assert rel >= 0 and rel % row_bytes == 0 and s["bytes"] % row_bytes == 0 and s["bytes"] > 0
        first, n = rel // row_bytes, s["bytes"] // row_bytes
        assert first + n <= ring, "a segment runs past the end of the ring"
        rows += list(range(first, first + n))
    return rows


def check_plan(case, ans):
    _, kv_head, mel_start, mel_count, abuf_cnt, abuf_par, esz, n_layers, ks, src_slot, dst_slot = case[:11]
    f = case[11:]
    segs, fault, (n_pieces, largest, piece_total, outside) = parse_plan(ans)
    assert fault == "ok", (case, fault)
    for s in segs:                                                     # every segment stays in its own slot's part, the same place on both sides
        assert s["src"] - src_slot * s["slot_bytes"] == s["dst"] - dst_slot * s["slot_bytes"], (case, s)
        assert 0 <= s["src"] - src_slot * s["slot_bytes"] and s["src"] + s["bytes"] <= (src_slot + 1) * s["slot_bytes"], (case, s)
        gran = 4 if s["name"] in WORD_ITEMS else 16
        assert s["src"] % gran == 0 and s["dst"] % gran == 0 and s["bytes"] % gran == 0, (case, s)
        if s["name"] in WORD_ITEMS - {"aud_hist"}:
            assert s["bytes"] == 4
    # K/V: per layer and plane exactly the 70 window rows, no row twice, at most two segments
    row, plane = D * esz, KVC * D * esz
    kv = [s for s in segs if s["buf"] == BUF_KV]
    assert sum(s["bytes"] for s in kv) == n_layers * 2 * LCTX * D * esz, case
    want_rows = sorted((kv_head + j) % KVC for j in range(LCTX))
    for layer in range(n_layers):
        for p in range(2):
            mine = [s for s in kv if s["layer"] == layer and p * plane <= s["src"] - src_slot * 2 * plane < (p + 1) * plane]
            assert 1 <= len(mine) <= 2 and all(s["slot_bytes"] == 2 * plane for s in mine), case
            assert sorted(ring_rows_covered(mine, src_slot, 2 * plane, p * plane, row, KVC)) == want_rows, (case, layer, p)
    cc = [s for s in segs if s["buf"] == BUF_CC]
    assert sorted(s["layer"] for s in cc) == list(range(n_layers)) and all(s["bytes"] == s["slot_bytes"] == 2 * (ks - 1) * D * 4 for s in cc), case
    mel = [s for s in segs if s["buf"] == BUF_MEL]
    assert len(mel) <= 2 and sorted(ring_rows_covered(mel, src_slot, MEL_RING * NMEL * 4, 0, NMEL * 4, MEL_RING)) == sorted((mel_start + i) % MEL_RING for i in range(mel_count)), case
    ab = [s for s in segs if s["buf"] == BUF_ABUF]
    if abuf_cnt == 0:
        assert not ab
    else:
        (a,) = ab
        assert a["src"] == (src_slot * 2 + abuf_par) * ABUF_CAP * 4 and a["bytes"] == (abuf_cnt * 4 + 15) // 16 * 16 and a["slot_bytes"] == 2 * ABUF_CAP * 4, case
    (ls,) = [s for s in segs if s["buf"] == BUF_LAST]
    (ah,) = [s for s in segs if s["buf"] == BUF_HIST]
    assert (ls["name"], ls["bytes"], ls["src"]) == ("last_sample", 4, 4 * src_slot) and (ah["name"], ah["bytes"], ah["src"]) == ("aud_hist", 2 * HIST_MAX * 4, src_slot * 2 * HIST_MAX * 4)
    dec = {s["name"]: s for s in segs if s["buf"] == BUF_DEC}
    assert len(dec) == sum(s["buf"] == BUF_DEC for s in segs)
    assert {k: s["bytes"] for k, s in dec.items()} == slot_bytes_of_the_decoder(*f), case
    assert all(s["bytes"] == s["slot_bytes"] for s in dec.values()) and not set(dec) & SCRATCH
    # source and destination ranges of one plan are pairwise disjoint: per buffer, every range of either side against every other
    groups = {}
    for s in segs:
        g = groups.setdefault((s["buf"], s["layer"], s["name"]), [])
        g += [(s["src"], s["src"] + s["bytes"]), (s["dst"], s["dst"] + s["bytes"])]
    for g in groups.values():
        g.sort()
        assert all(a[1] <= b[0] for a, b in zip(g, g[1:])), case
    # the pieces: all the bytes, none larger than 256 KiB, each inside its segment
    total = sum(s["bytes"] for s in segs)
    assert piece_total == total and largest <= 256 * 1024 and outside == 0 and n_pieces >= len(segs), case
    return total


KV_HEADS = (0, 255, 256, 257, 300, 325)
MELS = ((0, 9), (4000, 121), (4090, 9), (4095, 1))
ABUFS = (0, 256, 257, 7777)


def test_segments_cover_exactly_the_live_part(fork_plan):
    grid = list(itertools.product(KV_HEADS, MELS, ABUFS, (0, 1), (2, 4)))
    cases = [plan_case(kv, mel, cnt, par, esz, COMBOS[i % len(COMBOS)] if i % 5 else ALL) for i, (kv, mel, cnt, par, esz) in enumerate(grid)]
    assert len(cases) == 384
    for case, ans in zip(cases, fork_plan(cases)):
        check_plan(case, ans)
    # the wraps were met: a head at 257 and beyond splits the window, a mel window that crosses frame 4095 splits too
    segs, _, _ = parse_plan(fork_plan([plan_case(300, (4090, 9), 256, 1, 2, ALL)])[0])
    assert sum(s["buf"] == BUF_KV for s in segs) == 3 * 2 * 2 and sum(s["buf"] == BUF_MEL for s in segs) == 2
    segs, _, _ = parse_plan(fork_plan([plan_case(256, (4000, 96), 256, 1, 2, ALL)])[0])
    assert sum(s["buf"] == BUF_KV for s in segs) == 3 * 2 and sum(s["buf"] == BUF_MEL for s in segs) == 1


def test_a_whole_slot_copy_would_not_pass(fork_plan):
    """24 layers at bf16, every option on, a chunk's worth buffered: the plan moves 8.9 MB (8.6 MB with no option on) of the 38 MB a slot owns, 6.9 MB of it K/V rows: under a quarter"""
    case = plan_case(123, (2000, 121), 2000, 0, 2, ALL, n_layers=24, ks=9, src_slot=0, dst_slot=1)
    (ans,) = fork_plan([case])
    total = check_plan(case, ans)
    kv = 24 * 2 * 70 * 1024 * 2
    assert kv == 6881280 and kv < total < kv + 2 * 1024 * 1024
    assert total < (24 * (2 * KVC * D * 2 + 2 * 8 * D * 4) + MEL_RING * NMEL * 4 + 2 * ABUF_CAP * 4) // 4
    # neighbouring slots in either order, and slot 0
    for src, dst in ((0, 1), (1, 0), (7, 0), (0, 4095)):
        case = plan_case(325, (4095, 1), 7777, 1, 4, ALL, src_slot=src, dst_slot=dst)
        check_plan(case, fork_plan([case])[0])


def test_headers_are_pure_host_code():
    src = (CSRC / "nasr_fork_plan.h").read_text()
    assert "#include <hip" not in src and "__global__" not in src and "hipLaunch" not in src
    for name in ("struct Source", "struct Seg", "inline std::vector<Seg> fork_plan", "inline const char *plan_fault", "inline void cut_pieces"):
        assert name in src
    assert "inline void dec_set_slot_layout" in (CSRC / "nasr_decode_set.h").read_text()
