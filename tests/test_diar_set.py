"""The working set of a TitaNet-L embedding call (nemotron-asr.cpp_amd/csrc/nasr_diar_set.h: SpkSet, spk_set_layout, spk_set_ensure).
No GPU: the header is compiled with the host compiler under AddressSanitizer and UBSan into a stand-alone program whose allocator is
malloc, has the engine's 16-byte minimum (dalloc in nasr_diar.hip) and records (buffer name, bytes), like tests/test_decode_set.py.

Expected sizes, restated here and not read from the header, with S = max_segments and M = 160 S rows:
  * both engines:      s_mel M x 96 f32, Y M x 3072 f32, se_z 2S x 3072 f32, se_h S x 384 f32, att_c S x 128 f32, att_g M x 128 f32,
                       pool S x 6144 f32, emb S x 192 f32, s_lens S i32, s_off S i64
  * f32 engine only:   X0, X1 M x 3072 f32, R M x 1024 f32, st_mean, st_std S x 3072 f32, A M x 3072 f32
  * bf16 engine only:  sA0, sA1, sX0, sX1 M x 1024 bf16, sX4 M x 3072 bf16, st_ms S x 6144 f32, fc_part 16 x S x 512 f32, A M x 128 bf16
Before the set existed the engine allocated the union of the three lists whatever its dtype, with A at M x 3072 elements of the GEMM
operand type (parent_bf16_total).
"""
import shutil
import subprocess
from pathlib import Path

import pytest

from tests.test_gemm_plan import HIP_STUB

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"

DRIVER = r"""
#include "nasr_internal.h"
#include "nasr_diar_set.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
using namespace nasr;
// one case "<max_segments> <bf16>" per line of stdin: spk_set_ensure twice on one SpkSet -> one line of stdout
//   "<rc of both calls> | <1 if the second call moved a buffer> | <name:bytes of the first call's allocations> | <allocations of the second call> | <non-null buffers>"
static std::vector<std::pair<std::string, size_t>> g_recs;
static std::vector<void *> g_ptrs;
static int rec_alloc(const char *name, void **p, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    *p = malloc(bytes);
    if (!*p) return -1;
    g_ptrs.push_back(*p);
    g_recs.push_back({name, bytes});
    return 0;
}
static std::vector<std::pair<std::string, const void *>> pointers(SpkSet &d) {
    std::vector<std::pair<std::string, const void *>> v;
    spk_set_layout(d, false, 1, [&](const char *name, auto *&p, bool, size_t) { v.push_back({name, p}); });
    return v;
}
int main() {
    int S, bf16;
    while (scanf("%d %d", &S, &bf16) == 2) {
        SpkSet d;
        g_recs.clear();
        const int rc1 = spk_set_ensure(d, bf16 != 0, S, rec_alloc);
        const auto before = pointers(d);
        const size_t n1 = g_recs.size();
        const int rc2 = spk_set_ensure(d, bf16 != 0, S, rec_alloc);
        const auto after = pointers(d);
        int moved = before.size() != after.size();
        for (size_t i = 0; i < before.size() && !moved; i++) moved = before[i].second != after[i].second;
        printf("%d %d | %d |", rc1, rc2, moved);
        for (size_t i = 0; i < n1; i++) printf(" %s:%zu", g_recs[i].first.c_str(), g_recs[i].second);
        printf(" | %zu |", g_recs.size() - n1);
        for (auto &kv : after) if (kv.second) printf(" %s", kv.first.c_str());
        printf("\n");
        for (void *p : g_ptrs) free(p);
        g_ptrs.clear();
    }
    return 0;
}
"""

SEGMENTS = (1, 2, 96, 128)
F32_ONLY = ("X0", "X1", "R", "st_mean", "st_std")
BF16_ONLY = ("sA0", "sA1", "sX0", "sX1", "sX4", "st_ms", "fc_part")


def shared_buffers(S):
    M = 160 * S
    return dict(s_mel=M * 96 * 4, Y=M * 3072 * 4, se_z=2 * S * 3072 * 4, se_h=S * 384 * 4, att_c=S * 128 * 4, att_g=M * 128 * 4,
                pool=S * 6144 * 4, emb=S * 192 * 4, s_lens=S * 4, s_off=S * 8)


def f32_only_buffers(S):
    M = 160 * S
    return dict(X0=M * 3072 * 4, X1=M * 3072 * 4, R=M * 1024 * 4, st_mean=S * 3072 * 4, st_std=S * 3072 * 4)


def bf16_only_buffers(S):
    M = 160 * S
    return dict(sA0=M * 1024 * 2, sA1=M * 1024 * 2, sX0=M * 1024 * 2, sX1=M * 1024 * 2, sX4=M * 3072 * 2, st_ms=S * 6144 * 4, fc_part=16 * S * 512 * 4)


def table(S, bf16):
    """name -> bytes: the docstring's table, every allocation at least 16 bytes"""
    M = 160 * S
    b = shared_buffers(S)
    b.update(bf16_only_buffers(S) if bf16 else f32_only_buffers(S))
    b["A"] = M * 128 * 2 if bf16 else M * 3072 * 4
    return {k: max(v, 16) for k, v in b.items()}


def parent_bf16_total(S):
    """what a bf16 engine allocated before: the union of the three lists, A at M x 3072 bf16"""
    b = shared_buffers(S)
    b.update(f32_only_buffers(S))
    b.update(bf16_only_buffers(S))
    b["A"] = 160 * S * 3072 * 2
    return sum(max(v, 16) for v in b.values())


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("diar_set")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(HIP_STUB)
    (d / "drv.cpp").write_text(DRIVER)
    exe = d / "diar_set"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{d}", f"-I{CSRC}", f"-I{ROOT / 'include'}", str(d / "drv.cpp"), "-o", str(exe)])
    cases = [(S, bf16) for S in SEGMENTS for bf16 in (0, 1)]
    r = subprocess.run([str(exe)], input="".join(f"{S} {bf16}\n" for S, bf16 in cases), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    out = {}
    for case, ln in zip(cases, lines):
        rcs, moved, allocs, again, nonnull = [part.split() for part in ln.split("|")]
        allocs = [(a.split(":")[0], int(a.split(":")[1])) for a in allocs]
        assert len({n for n, _ in allocs}) == len(allocs), case          # no buffer allocated twice
        out[case] = dict(rcs=[int(v) for v in rcs], moved=int(moved[0]), allocs=dict(allocs), again=int(again[0]), nonnull=sorted(nonnull))
    return out


@pytest.mark.parametrize("bf16", (0, 1), ids=("f32", "bf16"))
@pytest.mark.parametrize("S", SEGMENTS)
def test_each_engine_allocates_its_own_table(answers, S, bf16):
    a = answers[(S, bf16)]
    assert a["rcs"] == [0, 0]
    assert a["allocs"] == table(S, bf16)
    assert a["nonnull"] == sorted(table(S, bf16))
    other = F32_ONLY if bf16 else BF16_ONLY
    assert not set(other) & set(a["allocs"]) and not set(other) & set(a["nonnull"])
    if S == 1:
        assert a["allocs"]["s_lens"] == 16 and a["allocs"]["s_off"] == 16          # 4 and 8 bytes asked: the allocator's minimum


@pytest.mark.parametrize("bf16", (0, 1), ids=("f32", "bf16"))
@pytest.mark.parametrize("S", SEGMENTS)
def test_a_second_ensure_allocates_nothing_and_moves_nothing(answers, S, bf16):
    a = answers[(S, bf16)]
    assert a["again"] == 0 and a["moved"] == 0


def test_bf16_engine_at_128_segments_saves_what_it_never_touched(answers):
    S, M = 128, 160 * 128
    saved = 2 * M * 3072 * 4 + M * 1024 * 4 + 2 * S * 3072 * 4 + (M * 3072 * 2 - M * 128 * 2)
    assert sum(answers[(S, 1)]["allocs"].values()) == parent_bf16_total(S) - saved
    assert saved > 700e6          # 0.71 GB per engine
