"""gemm_plan_bf16 (nemotron-asr.cpp_amd/csrc/nasr_gemm_plan.h) chooses what the launcher ladder it replaced chose: kernel instance, grid, block,
dynamic LDS bytes, n_groups, m_chunks and the `splits` the kernel sees, on every row of a sweep whose expected values were recorded from that
ladder (tests/golden/gemm_plan_v1.json), never from the plan function.  No GPU: the header is plain C++ and is compiled with g++ under
AddressSanitizer and UBSan, like tests/test_offline_abi.py.

The sweep (SWEEP below, the one text both sides run): for every option tuple x num_cus in (256, 64) x (N, K, epilogue) group --
M = 1 .. 1 024, every multiple of 7 and of 16 up to 16 384, 769, 1 343, 1 344, 1 791, 1 792, ascending; per M the K slices 1, 2, 4, 8 and pick_splits'
value, in that order; per slice count GemmParams::coresident 0 .. 3; per coresident chain.head_wgs 0 and, where gemm_chain_ok(), the value enqueue_layers
computes.  EPI_RESID_F32 rows exist only where gemm_resid_foldable().  One row per launch, as text:
    "M splits coresident head_wgs kernel gx gy gz block lds n_groups m_chunks kernel_splits\n"
(kernel = the instance as written in the source without blanks and parentheses, k_gemm_persist<EPI> with the epilogue's number) and one 64-bit FNV-1a digest
(offset 14695981039346656037, prime 1099511628211, byte by byte) per group over its rows in that order: "plan".  "pred" is the digest of one line per M,
"M pick_splits gemm_tile_n" followed by " <gemm_chain_ok><gemm_resid_foldable>" (0 / 1) for each of the five slice counts.  The engine's own shapes at
the default options (B in 1 .. 512 streams x T in 1, 2, 7, 14 rows, synchronous and pipelined) are kept as rows, so a change there names its kernel.
When a digest differs the test names the group; re-run the recorder on that group to find the row.

How the golden file was recorded (the recorder is not kept in the tree): at the commit before this header existed, a host program
    #include <hip/hip_runtime.h>
    #include "nasr_internal.h"
    struct Row ...; static Row g_row;          // as in BACKEND below
    template <typename... A> static void rec_(const char *, dim3, dim3, size_t, const A &...) {}
    static void rec_(const char *k, dim3 g, dim3 b, size_t lds, const nasr::GemmParams &p)                  { g_row = {canon(k), g.x, g.y, g.z, b.x, (long)lds, 0, 0, p.splits}; }
    static void rec_(const char *k, dim3 g, dim3 b, size_t lds, const nasr::GemmParams &p, int ng, int mc)  { g_row = {canon(k), g.x, g.y, g.z, b.x, (long)lds, ng, mc, p.splits}; }
    #undef hipLaunchKernelGGL
    #define hipLaunchKernelGGL(k, g, b, lds, st, ...) rec_(#k, g, b, lds, __VA_ARGS__)
    #include "kernels_gemm.hip"
    backend_plan(p, cus, r):  nasr::g_num_cus = cus; nasr::launch_gemm_bf16(p, nullptr); r = g_row;
    backend_pick_splits(...): the body of nasr_eng::pick_splits of that commit with e->opt_t64_tiles + 1 and e->opt_split_tasks as parameters
    + SWEEP
built with `hipcc --offload-arch=gfx950 -O2 -std=c++17 -Iinclude -Inemotron-asr.cpp_amd/csrc` (the launcher made no other HIP call: it runs without a GPU);
its output lines, "G ..." and "R ...", are the golden file's "groups" and "engine_shapes"."""
import json
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"
GOLDEN = json.loads((ROOT / "tests" / "golden" / "gemm_plan_v1.json").read_text())

# what nasr_internal.h needs of <hip/hip_runtime.h> to be read by a host compiler
HIP_STUB = r"""#pragma once
#include <cstring>
typedef struct ihipStream_t *hipStream_t;
#define __device__
#define __forceinline__ inline
static inline float __uint_as_float(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
static inline unsigned __float_as_uint(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
"""

BACKEND = r"""
#include "nasr_internal.h"
#include "nasr_gemm_plan.h"
#include <cstdio>
#include <cstdlib>
#include <string>
struct Row { const char *name; unsigned gx, gy, gz, block; long lds; int ng, mc, splits; };
static std::string g_names[nasr::GI_COUNT];
static void init_names() {          // "(k_gemm_persist<EPI_QKV>)" -> "k_gemm_persist<2>"
    if (nasr::gemm_pick_splits(false, 896, 1024, 4096, 65, 0) != 1) { printf("BAD: the f32 engine never splits K\n"); exit(1); }
    static const char *epis[][2] = {{"EPI_PART_F32", "0"}, {"EPI_SILU_ACT", "1"}, {"EPI_QKV", "2"}, {"EPI_GLU", "3"}, {"EPI_BIAS_F32", "4"}, {"EPI_BIAS_RELU_F32", "6"}};
    for (int i = 0; i < nasr::GI_COUNT; i++) {
        std::string s;
        for (const char *c = nasr::GEMM_INST_NAME[i]; *c; c++) if (*c != ' ' && *c != '(' && *c != ')') s += *c;
        for (auto &e : epis) { size_t at = s.find(e[0]); if (at != std::string::npos) s.replace(at, std::string(e[0]).size(), e[1]); }
        g_names[i] = s;
    }
}
static void backend_plan(const nasr::GemmParams &p, int num_cus, Row &r) {
    if (g_names[0].empty()) init_names();
    const nasr::GemmPlan pl = nasr::gemm_plan_bf16(p, num_cus);
    // every plan's LDS size is the one registered for its instance (init_gemm_kernel_attributes walks the same table) and fits a CU
    if (pl.inst < 0 || pl.inst >= nasr::GI_COUNT || pl.lds != nasr::GEMM_INST_LDS[pl.inst] || pl.lds > 160 * 1024) {
        printf("BAD plan: instance %d LDS %d (M %d N %d K %d)\n", (int)pl.inst, pl.lds, p.M, p.N, p.K);
        exit(1);
    }
    r = Row{g_names[pl.inst].c_str(), pl.grid[0], pl.grid[1], pl.grid[2], (unsigned)pl.block, (long)pl.lds, pl.n_groups, pl.m_chunks, pl.splits};
}
static int backend_pick_splits(int M, int N, int K, int t64_p1, int split_tasks) { return nasr::gemm_pick_splits(true, M, N, K, t64_p1, split_tasks); }
"""

SWEEP = r"""// ---- the sweep (one text for the recorder of the golden file and for the test) ----------------------------------------------
// The including file provides, before this text: nasr::GemmParams, the Epi values, nasr::gemm_tile_n / gemm_chain_ok /
// gemm_resid_foldable, and
//   struct Row { const char *name; unsigned gx, gy, gz, block; long lds; int ng, mc, splits; };
//   static void backend_plan(const nasr::GemmParams &p, int num_cus, Row &r);
//   static int backend_pick_splits(int M, int N, int K, int t64_p1, int split_tasks);
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct Opt { const char *name; int prio, no_persist, no_wide, wide_rows, tile_bands, t64_p1, narrow, wide_min_tiles, wide_min_rows, split_tasks; };
struct Shape { int N, K, epi; };

// engine options as run_gemm translates them (defaults: persistent_gemm 0, wide_tiles 1, tile_bands -1, t64_tiles 64, epilogue16 1)
static const Opt OPTS[] = {
    {"default", 0, 1, 0, 0, 0, 65, 0, 0, 0, 0},
    {"persistent_gemm=1", 0, 0, 0, 0, 0, 65, 0, 0, 0, 0},
    {"wide_tiles=0,tile_bands=0,t64_tiles=127", 0, 1, 1, 0, 2, 128, 0, 0, 0, 0},
    {"wide_tiles=256,tile_bands=1", 0, 1, 0, 256, 1, 65, 0, 0, 0, 0},
    {"gemm_prio=20", 20, 1, 0, 0, 0, 65, 0, 0, 0, 0},
    {"gemm_prio=16,epilogue16=0", 16, 1, 0, 0, 0, 65, 1, 0, 0, 0},
    {"wide_tiles=0", 0, 1, 1, 0, 0, 65, 0, 0, 0, 0},
    {"wide_tiles=3", 0, 1, 0, 2, 0, 65, 0, 0, 0, 0},
    {"wide_min_tiles=16", 0, 1, 0, 0, 0, 65, 0, 16, 0, 0},
    {"wide_min_rows=1000", 0, 1, 0, 0, 0, 65, 0, 0, 1000, 0},
    {"split_tasks=100", 0, 1, 0, 0, 0, 65, 0, 0, 0, 100},
    {"spk_gemm", 0, 1, 0, 0, 0, 0, 0, 0, 0, 0},          // nasr_diar.hip: memset 0, no_persist = 1 (coresident = 1 is part of the sweep)
};
// run_gemm call sites of nasr_encoder.hip / nasr_offline.hip for the 24-layer model: W1, W2 (+ folded), QKV (streaming, offline), Wo = pw2 (+ folded), pw1,
// subsampling pw3 / pw6 / output projection
static const Shape ENC_SHAPES[] = {
    {4096, 1024, nasr::EPI_SILU_ACT}, {1024, 4096, nasr::EPI_PART_F32}, {1024, 4096, nasr::EPI_RESID_F32}, {3072, 1024, nasr::EPI_QKV},
    {3072, 1024, nasr::EPI_BIAS_ACT}, {1024, 1024, nasr::EPI_PART_F32}, {1024, 1024, nasr::EPI_RESID_F32}, {2048, 1024, nasr::EPI_GLU},
    {256, 256, nasr::EPI_BIAS_RELU_F32}, {256, 256, nasr::EPI_BIAS_RELU_ACT}, {1024, 4352, nasr::EPI_BIAS_F32},
};
// spk_gemm call sites for TitaNet-L: block 0 (80 -> 128 padded), blocks 1-3 sub-convs (ReLU between) and residual convs, block 4, the two attention convs
static const Shape SPK_SHAPES[] = {
    {1024, 128, nasr::EPI_BIAS_F32}, {1024, 1024, nasr::EPI_BIAS_RELU_F32}, {1024, 1024, nasr::EPI_BIAS_F32}, {3072, 1024, nasr::EPI_BIAS_F32},
    {128, 3072, nasr::EPI_BIAS_F32}, {3072, 128, nasr::EPI_BIAS_F32},
};
static const int NUM_CUS[] = {256, 64};

struct Fnv {
    uint64_t h = 14695981039346656037ull;
    void add(const char *s, size_t n) { for (size_t i = 0; i < n; i++) { h ^= (unsigned char)s[i]; h *= 1099511628211ull; } }
};
static char *put_int(char *o, long v) {
    if (v < 0) { *o++ = '-'; v = -v; }
    char t[24]; int n = 0;
    do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) *o++ = t[--n];
    return o;
}
static char *put_str(char *o, const char *s) { while (*s) *o++ = *s++; return o; }
// "M splits coresident head_wgs name gx gy gz block lds n_groups m_chunks kernel_splits\n"
static size_t fmt_row(char *buf, int M, int splits, int cores, int head, const Row &r) {
    char *o = buf;
    o = put_int(o, M); *o++ = ' '; o = put_int(o, splits); *o++ = ' '; o = put_int(o, cores); *o++ = ' '; o = put_int(o, head); *o++ = ' ';
    o = put_str(o, r.name); *o++ = ' ';
    o = put_int(o, r.gx); *o++ = ' '; o = put_int(o, r.gy); *o++ = ' '; o = put_int(o, r.gz); *o++ = ' '; o = put_int(o, r.block); *o++ = ' ';
    o = put_int(o, r.lds); *o++ = ' '; o = put_int(o, r.ng); *o++ = ' '; o = put_int(o, r.mc); *o++ = ' '; o = put_int(o, r.splits); *o++ = '\n';
    return (size_t)(o - buf);
}
static void fill(nasr::GemmParams &g, const Opt &o, int M, int N, int K, int epi, int splits, int cores, int head) {
    memset(&g, 0, sizeof(g));
    g.M = M; g.N = N; g.K = K; g.lda = K; g.splits = splits; g.epi = epi; g.ldo = N; g.ldo_act = N; g.T = 1;
    g.coresident = cores; g.prio = o.prio; g.no_persist = o.no_persist; g.no_wide = o.no_wide; g.wide_rows = o.wide_rows; g.tile_bands = o.tile_bands;
    g.t64_tiles_p1 = o.t64_p1; g.narrow_stores = o.narrow; g.wide_min_tiles = o.wide_min_tiles; g.wide_min_rows = o.wide_min_rows;
    g.chain.head_wgs = head; g.chain.head_rows = head ? 4 : 0;
}
static int chain_head_wgs(int M) { return (((M + 3) / 4) + 7) & ~7; }          // enqueue_layers

int main() {
    std::vector<int> Ms;
    for (int m = 1; m <= 1024; m++) Ms.push_back(m);
    for (int m = 7; m <= 16384; m += 7) Ms.push_back(m);
    for (int m = 16; m <= 16384; m += 16) Ms.push_back(m);
    for (int m : {769, 1343, 1344, 1791, 1792}) Ms.push_back(m);
    std::sort(Ms.begin(), Ms.end());
    Ms.erase(std::unique(Ms.begin(), Ms.end()), Ms.end());
    char buf[512];
    nasr::GemmParams g;
    Row r;
    const int n_opts = (int)(sizeof(OPTS) / sizeof(OPTS[0]));
    for (int oi = 0; oi < n_opts; oi++) {
        const Opt &o = OPTS[oi];
        const bool spk = oi == n_opts - 1;
        const Shape *shapes = spk ? SPK_SHAPES : ENC_SHAPES;
        const int n_shapes = spk ? (int)(sizeof(SPK_SHAPES) / sizeof(Shape)) : (int)(sizeof(ENC_SHAPES) / sizeof(Shape));
        for (int cus : NUM_CUS)
            for (int si = 0; si < n_shapes; si++) {
                const Shape &s = shapes[si];
                Fnv plan, pred;
                long rows = 0;
                for (int M : Ms) {
                    const int pick = backend_pick_splits(M, s.N, s.K, o.t64_p1, o.split_tasks);
                    const int sp[5] = {1, 2, 4, 8, pick};
                    char *q = buf;
                    q = put_int(q, M); *q++ = ' '; q = put_int(q, pick); *q++ = ' '; q = put_int(q, nasr::gemm_tile_n(M, s.N, s.epi, o.t64_p1));
                    for (int splits : sp) {
                        const bool chain = nasr::gemm_chain_ok(M, s.N, s.K, splits), fold = nasr::gemm_resid_foldable(M, s.N, s.K, splits, o.t64_p1);
                        *q++ = ' '; *q++ = chain ? '1' : '0'; *q++ = fold ? '1' : '0';
                        if (s.epi == nasr::EPI_RESID_F32 && !fold) continue;          // the engine asks gemm_resid_foldable() first
                        for (int cores = 0; cores < 4; cores++)
                            for (int hv = 0; hv < (chain ? 2 : 1); hv++) {
                                const int head = hv ? chain_head_wgs(M) : 0;
                                fill(g, o, M, s.N, s.K, s.epi, splits, cores, head);
                                backend_plan(g, cus, r);
                                plan.add(buf + 256, fmt_row(buf + 256, M, splits, cores, head, r));
                                rows++;
                            }
                    }
                    *q++ = '\n';
                    pred.add(buf, (size_t)(q - buf));
                }
                printf("G %s %d %d %d %d %ld %016llx %016llx\n", o.name, cus, s.N, s.K, s.epi, rows, (unsigned long long)plan.h, (unsigned long long)pred.h);
            }
    }
    // the engine's own shapes at the default options, in full: B streams x T rows, synchronous (coresident 0) and pipelined (1) steps, 256 CUs; the residual
    // GEMMs with pick_splits' slices and folded where enqueue_layers folds them
    const Opt &o = OPTS[0];
    for (int B : {1, 8, 16, 32, 64, 128, 256, 512})
        for (int T : {1, 2, 7, 14})
            for (int cores = 0; cores < 2; cores++)
                for (const Shape &s : ENC_SHAPES) {
                    if (s.epi == nasr::EPI_RESID_F32) continue;
                    const int M = B * T;
                    int splits = 1, epi = s.epi;
                    if (s.N == 1024 && s.epi == nasr::EPI_PART_F32) {
                        splits = backend_pick_splits(M, s.N, s.K, o.t64_p1, o.split_tasks);
                        if ((splits == 1 || cores == 1) && nasr::gemm_resid_foldable(M, s.N, s.K, splits, o.t64_p1)) epi = nasr::EPI_RESID_F32;
                    }
                    fill(g, o, M, s.N, s.K, epi, splits, cores, 0);
                    backend_plan(g, 256, r);
                    const size_t n = fmt_row(buf, M, splits, cores, 0, r);
                    buf[n - 1] = 0;
                    printf("R %d %d %d %s\n", s.N, s.K, epi, buf);
                }
    return 0;
}
"""


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("gemm_plan")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(HIP_STUB)
    (d / "sweep.cpp").write_text(BACKEND + SWEEP + "\nstatic_assert(nasr::GEMM_INST_LDS[nasr::GI_WIDE2_256_7] == 153600 && nasr::GEMM_INST_LDS[nasr::GI_WIDE2_192_7] == 139264, \"wide2_lds\");\n")
    exe = d / "sweep"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{d}", f"-I{CSRC}", f"-I{ROOT / 'include'}", str(d / "sweep.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    groups, rows = [], []
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "G":
            groups.append(dict(opt=t[1], num_cus=int(t[2]), N=int(t[3]), K=int(t[4]), epi=int(t[5]), rows=int(t[6]), plan=t[7], pred=t[8]))
        else:
            assert t[0] == "R", line
            rows.append(line[2:])
    return groups, rows


def test_every_group_of_the_sweep_has_the_recorded_digest(sweep):
    groups, _ = sweep
    key = lambda g: (g["opt"], g["num_cus"], g["N"], g["K"], g["epi"])
    assert [key(g) for g in groups] == [key(g) for g in GOLDEN["groups"]]          # no group skipped, none added
    assert len(groups) == 254 and sum(g["rows"] for g in groups) == 21938952
    bad = [(key(g), [f for f in ("rows", "plan", "pred") if g[f] != w[f]]) for g, w in zip(groups, GOLDEN["groups"]) if g != w]
    assert not bad, "groups (option tuple, num_cus, N, K, epi) whose launches or predicates differ from the recorded ladder: %r" % bad


def test_engine_shapes_take_the_recorded_kernels(sweep):
    _, rows = sweep
    want = GOLDEN["engine_shapes"]
    assert len(rows) == len(want) == 576
    diff = ["%s  (recorded: %s)" % (a, b) for a, b in zip(rows, want) if a != b]
    assert not diff, "\n".join(diff[:40])
    # the issue's own spot checks of the recorded table: N = 4096, K = 1024, SiLU
    assert "4096 1024 1 896 1 0 0 k_gemm_roles<4> 224 1 1 1024 131072 32 7 1" in want
    assert "4096 1024 1 896 1 1 0 k_gemm_tiled3 224 1 1 512 81920 32 7 1" in want
    assert "4096 1024 1 7168 1 0 0 k_gemm_wide2<256,7> 512 1 1 512 153600 16 32 1" in want
