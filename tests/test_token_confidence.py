"""host/token_confidence.h (entropy-based token and word confidence above the C ABI), compiled with the host compiler under
AddressSanitizer / UBSan -- no GPU.  The maps are restated here in float64 from their definitions (Laptev and Ginsburg's entropy-based
confidence): Renyi / Shannon lin 1 - H / ln V, exp (V e^-H - 1) / (V - 1); Tsallis T = (1 - e^((1 - a) H)) / (a - 1),
T_max = (1 - V^(1 - a)) / (a - 1), lin 1 - T / T_max, exp (e^-T - e^-T_max) / (1 - e^-T_max); V = 1025.  The header rounds to f32 once,
so it agrees with the restatement within 2^-23 (asserted: 2e-7)."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "nemotron-asr.cpp_amd" / "host"
V = 1025.0
LN_V = math.log(V)

DRIVER = r"""
#include "token_confidence.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace token_conf;
// map <method 0|1> <norm 0|1> <alpha> <H ...>       -> one confidence per H, %.9g ("nan" for NaN)
// agg <agg 0|1|2> <c ...>                           -> the aggregate
// words <agg> <n> <token conf>*n                    -> the words of the fixed vocabulary below: "text:first:n:conf" each
int main(int argc, char **argv) {
    if (!strcmp(argv[1], "map")) {
        for (int i = 5; i < argc; i++) printf("%.9g\n", (double)confidence(strtof(argv[i], nullptr), atof(argv[4]), (Method)atoi(argv[2]), (Norm)atoi(argv[3])));
        return 0;
    }
    if (!strcmp(argv[1], "agg")) {
        std::vector<float> c;
        for (int i = 3; i < argc; i++) c.push_back(strtof(argv[i], nullptr));
        printf("%.9g\n", (double)aggregate(c.data(), c.size(), (Agg)atoi(argv[2])));
        return 0;
    }
    if (!strcmp(argv[1], "words")) {
        const std::vector<std::string> vocab = {"\xe2\x96\x81he", "llo", "\xe2\x96\x81wor", "ld", "\xe2\x96\x81" "a", "x"};
        std::vector<int> toks;
        std::vector<float> conf;
        const int n = atoi(argv[3]);
        for (int i = 0; i < n; i++) { toks.push_back(atoi(argv[4 + 2 * i])); conf.push_back(strtof(argv[5 + 2 * i], nullptr)); }
        if (argc > 4 + 2 * n) conf.resize((size_t)atoi(argv[4 + 2 * n]));          // a shorter list of confidences
        for (const word_conf::Word &w : words(toks, conf, vocab, (Agg)atoi(argv[2]))) printf("%s:%d:%d:%.9g\n", w.text.c_str(), w.first_token, w.n_tokens, (double)w.confidence);
        bool mp; Method m; Norm nn; Agg a;
        printf("%d%d%d%d%d%d%d\n", parse_method("max_prob", &mp, &m) && mp, parse_method("entropy", &mp, &m) && !mp && m == METHOD_ENTROPY, parse_method("tsallis", &mp, &m) && m == METHOD_TSALLIS,
               !parse_method("renyi", &mp, &m), parse_norm("lin", &nn) && nn == NORM_LIN && parse_norm("exp", &nn) && nn == NORM_EXP && !parse_norm("", &nn),
               parse_agg("min", &a) && a == AGG_MIN && parse_agg("mean", &a) && a == AGG_MEAN && parse_agg("prod", &a) && a == AGG_PROD, !parse_agg("max", &a));
        return 0;
    }
    return 1;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("tconf")
    (d / "drv.cpp").write_text(DRIVER)
    out = d / "tconf"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{HOST}", str(d / "drv.cpp"), "-o", str(out)])

    def run(*args):
        r = subprocess.run([str(out), *[str(a) for a in args]], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return r.stdout.split()
    return run


def restated(H, alpha, method, norm):
    H = np.asarray(H, np.float64)
    if method == 0 or alpha == 1.0:
        return 1.0 - H / LN_V if norm == 0 else (V * np.exp(-H) - 1.0) / (V - 1.0)
    T = (1.0 - np.exp((1.0 - alpha) * H)) / (alpha - 1.0)
    Tmax = (1.0 - V ** (1.0 - alpha)) / (alpha - 1.0)
    return 1.0 - T / Tmax if norm == 0 else (np.exp(-T) - np.exp(-Tmax)) / (1.0 - np.exp(-Tmax))


CASES = [(m, n, a) for m in (0, 1) for n in (0, 1) for a in (0.05, 0.333, 0.9, 1.0, 1.1, 2.0, 4.0)]


@pytest.mark.parametrize("method,norm,alpha", CASES)
def test_maps_end_points_monotone_and_float64(exe, method, norm, alpha):
    H = np.linspace(0.0, LN_V, 41).astype(np.float32)
    H[-1] = np.float32(6.9324479)                                   # (float) ln 1025, the engine's largest value
    got = np.array([float(v) for v in exe("map", method, norm, alpha, *[repr(float(h)) for h in H])])
    assert got[0] == 1.0 and abs(got[-1]) < 2e-7                    # 1 at H = 0, 0 at H = ln V
    assert ((got >= 0.0) & (got <= 1.0)).all()
    ref = np.clip(restated(H.astype(np.float64), alpha, method, norm), 0.0, 1.0)
    assert (np.diff(got) <= 0).all()                                # falling in H, strictly while the value is an f32 normal number
    assert (np.diff(got)[ref[1:] > 1e-37] < 0).all()                # (Tsallis exp at alpha = 0.05: T_max = 760, e^-T leaves f32 half way)
    assert np.abs(got - ref).max() < 2e-7, np.abs(got - ref).max()


def test_tsallis_is_not_renyi_and_meets_shannon_at_one(exe):
    H = ["0.5", "2.0", "5.0"]
    ren = [float(v) for v in exe("map", 0, 1, 0.333, *H)]
    tsa = [float(v) for v in exe("map", 1, 1, 0.333, *H)]
    assert all(abs(a - b) > 1e-3 for a, b in zip(ren, tsa))
    assert exe("map", 1, 0, 1.0, *H) == exe("map", 0, 0, 1.0, *H)
    # close to 1 the Tsallis maps tend to Shannon's: nothing cancels (expm1)
    near = [float(v) for v in exe("map", 1, 0, 1.0000001, *H)]
    assert np.abs(np.array(near) - np.array([float(v) for v in exe("map", 0, 0, 1.0, *H)])).max() < 1e-5


def test_nan_and_out_of_range(exe):
    for m, n, a in CASES[::3]:
        assert exe("map", m, n, a, "nan") == ["nan"]
        lo, hi = exe("map", m, n, a, "-0.25", "9.0")                # outside [0, ln V]: clamped
        assert float(lo) == 1.0 and float(hi) == 0.0


def test_aggregations(exe):
    c = ["0.5", "0.25", "0.8"]
    assert float(exe("agg", 0, *c)[0]) == 0.25
    assert abs(float(exe("agg", 1, *c)[0]) - (0.5 + 0.25 + 0.8) / 3) < 1e-7
    assert abs(float(exe("agg", 2, *c)[0]) - 0.1) < 1e-7
    for agg in (0, 1, 2):
        assert exe("agg", agg, "0.5", "nan", "0.8") == ["nan"]
        assert exe("agg", agg) == ["nan"]
        assert float(exe("agg", agg, "0.625")[0]) == 0.625


def test_words_are_cut_as_word_confidence_cuts_them(exe):
    # he llo | wor ld | a ; id 9 is outside the vocabulary and is skipped; "x" in front of the first marker is a word of its own
    toks = [(5, 0.9), (0, 0.5), (1, 0.25), (9, 0.01), (2, 0.8), (3, 0.4), (4, 0.7)]
    flat = [v for t in toks for v in t]
    out = exe("words", 0, len(toks), *flat)
    assert out[-1] == "1111111"
    words = [w.split(":") for w in out[:-1]]
    assert [(w[0], int(w[1]), int(w[2])) for w in words] == [("x", 0, 1), ("hello", 1, 2), ("world", 4, 2), ("a", 6, 1)]
    assert [float(w[3]) for w in words] == pytest.approx([0.9, 0.25, 0.4, 0.7])
    mean = [float(w.split(":")[3]) for w in exe("words", 1, len(toks), *flat)[:-1]]
    assert mean == pytest.approx([0.9, 0.375, 0.6, 0.7])
    prod = [float(w.split(":")[3]) for w in exe("words", 2, len(toks), *flat)[:-1]]
    assert prod == pytest.approx([0.9, 0.125, 0.32, 0.7])
    # a shorter list leaves the tokens beyond it at NaN, and a NaN token makes its word NaN
    short = [w.split(":")[3] for w in exe("words", 0, len(toks), *flat, 5)[:-1]]
    assert short[:2] == ["0.899999976", "0.25"] and short[2:] == ["nan", "nan"]
