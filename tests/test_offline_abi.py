"""Offline full-context transcription, host side (no GPU): the C ABI declares and exports the new entry points, and the plan
of a call (nasr_offline_plan.h: encoder frames, the 2048-frame limit, sub-batches under the row budget) -- compiled under
AddressSanitizer / UBSan -- agrees with the reference's own lengths."""
import json
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi
from oracle import binding as ob

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"

DRIVER = r"""
#include "nasr_offline_plan.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
// argv: budget max_utts n_mel...  ->  {"rc": r, "bad": b, "T": [...], "batches": [[first, count, rows], ...]}
int main(int argc, char **argv) {
    if (atoi(argv[1]) == 0) {                 // budget 0: the values are sample counts -> {"mel": [...], "max_samples": n}
        printf("{\"mel\": [");
        for (int i = 3; i < argc; i++) printf("%s%d", i > 3 ? ", " : "", nasr_plan::mel_frames(atoll(argv[i])));
        printf("], \"max_samples\": %lld}\n", (long long)nasr_plan::max_samples());
        return 0;
    }
    const int budget = atoi(argv[1]), max_utts = atoi(argv[2]), B = argc - 3;
    std::vector<int32_t> n(B > 0 ? B : 1);
    for (int b = 0; b < B; b++) n[b] = atoi(argv[3 + b]);
    std::vector<int> T;
    std::vector<nasr_plan::Batch> bt;
    int bad = -2;
    const int rc = nasr_plan::plan_offline(n.data(), B, budget, max_utts, T, bt, &bad);
    printf("{\"rc\": %d, \"bad\": %d, \"T\": [", rc, bad);
    for (size_t i = 0; i < T.size(); i++) printf("%s%d", i ? ", " : "", T[i]);
    printf("], \"batches\": [");
    for (size_t i = 0; i < bt.size(); i++) printf("%s[%d, %d, %d]", i ? ", " : "", bt[i].first, bt[i].count, bt[i].rows);
    printf("]}\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("plan")
    (d / "drv.cpp").write_text(DRIVER)
    exe = d / "plan"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{CSRC}", str(d / "drv.cpp"), "-o", str(exe)])

    def run(n_mel, budget=16384, max_utts=256):
        r = subprocess.run([str(exe), str(budget), str(max_utts), *[str(int(v)) for v in n_mel]], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return json.loads(r.stdout)
    return run


def test_header_declares_and_library_exports_offline_entry_points():
    assert re.search(r"#define NASR_OFFLINE_MAX_FRAMES 2048\b", HEADER)
    assert re.search(r"#define NASR_ABI_VERSION 1\b", HEADER)
    for name in ("nasr_engine_transcribe_mel", "nasr_engine_offline_tap"):
        assert re.search(rf"\b{name}\s*\(", HEADER), name
        assert name in capi.EXPORTS
    L = capi.lib()
    L.nasr_engine_transcribe_mel, L.nasr_engine_offline_tap    # noqa: B018  (raises if not exported)
    assert capi.check_exports()


def test_encoder_frames_follow_sub_out_len_three_times(planner):
    n_mel = [0, 1, 2, 7, 8, 9, 15, 16, 17, 121, 1000, 16376, 16377, 16378]
    got = planner(n_mel, budget=10 ** 9)
    s = lambda n: n // 2 + 1  # noqa: E731
    assert got["rc"] == -1 and got["bad"] == n_mel.index(16378)          # 16 378 mel frames -> 2049 > 2048
    ok = planner(n_mel[:-1], budget=10 ** 9)
    assert ok["rc"] == 0
    assert ok["T"] == [0 if n == 0 else s(s(s(n))) for n in n_mel[:-1]]
    assert ok["T"][n_mel.index(8)] == 2                                   # not ceil(8 / 8)
    assert ok["T"][n_mel.index(16377)] == 2048


def test_lengths_agree_with_the_reference(planner, weights1):
    rng = np.random.default_rng(1)
    n_mel = [1, 8, 9, 17, 40, 97]
    got = planner(n_mel)["T"]
    model = ob.OracleModel(weights1, 1)
    for n, T in zip(n_mel, got):
        mel = rng.standard_normal((n, 128)).astype(np.float32)
        assert model.subsampling(mel).shape[0] == T
        if ob.have_ref():
            assert ob.ref_subsampling(weights1, mel).shape[0] == T


def test_mel_frames_of_whole_utterances_agree_with_the_preprocessor(planner, weights1):
    ns = [0, 1, 100, 255, 256, 257, 415, 416, 417, 4000, 16000, 33333, 1280 * 256 + 7]
    got = planner(ns, budget=0)
    pp_args = (weights1["preprocessor.featurizer.fb"], weights1["preprocessor.featurizer.window"])
    rng = np.random.default_rng(4)
    for n, m in zip(ns, got["mel"]):
        pp = ob.OraclePreproc(*pp_args)
        assert pp.process((rng.standard_normal(n) * 500).astype(np.int16)).shape[0] == m, n
    mx = got["max_samples"]
    lim = planner([mx, mx + 1], budget=0)["mel"]
    s = lambda n: n // 2 + 1  # noqa: E731
    assert s(s(s(lim[0]))) == 2048 and s(s(s(lim[1]))) == 2049


def test_sub_batches_cover_in_order_within_budget(planner):
    rng = np.random.default_rng(2)
    for trial in range(30):
        B = int(rng.integers(1, 40))
        n_mel = [int(v) for v in rng.integers(0, 16384, B)]
        budget = int(rng.choice([1, 64, 700, 2048, 5000, 16384]))
        max_utts = int(rng.choice([1, 3, 256]))
        r = planner(n_mel, budget, max_utts)
        assert r["rc"] == 0
        nxt = 0
        for first, count, rows in r["batches"]:
            assert first == nxt and count >= 1 and count <= max_utts
            assert rows == sum(r["T"][first:first + count])
            assert rows <= budget or count == 1                       # only a lone utterance may exceed the budget
            nxt = first + count
        assert nxt == B


def test_limit_names_2048(planner):
    r = planner([16377, 16378, 5])
    assert r["rc"] == -1 and r["bad"] == 1
    assert planner([-1])["rc"] == -1
