"""CPU-side checks of the language-model ABI (no compute call, no GPU): the three entry points are declared, exported and bound;
nasr_lm_desc has the layout the header states, as a C compiler sees it and as capi declares it; the ARPA reader (host/lm_arpa.h) on the
hand-written tests/golden/lm_tiny.arpa (three orders, <s>, </s>, <unk>, an `ids:` word) and on malformed files, in a stand-alone driver
compiled with g++ under AddressSanitizer / UBSan; what it reads goes through nasr_lm::build and scores a sequence as tests/lm_ref.py does."""
import ctypes as C
import inspect
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi, gguf_io
from tests import lm_ref

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "nemotron-asr.cpp_amd"
NAMES = ("nasr_engine_set_lm", "nasr_engine_set_lm_weights", "nasr_engine_beam_hypothesis_lm")
ARPA = ROOT / "tests" / "golden" / "lm_tiny.arpa"
LN10 = math.log(10.0)
BOS, EOS = lm_ref.BOS, lm_ref.EOS


def test_lm_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
    L = capi.lib()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in capi.EXPORTS
        assert getattr(L, name).argtypes is not None
    assert L.nasr_engine_set_lm.argtypes[1] == C.POINTER(capi.LmDesc)
    assert L.nasr_engine_set_lm_weights.argtypes[1:] == [C.c_float, C.c_float]
    assert len(L.nasr_engine_beam_hypothesis_lm.argtypes) == 7 and L.nasr_engine_beam_hypothesis_lm.argtypes[3] == C.POINTER(C.c_double)
    for name in ("set_lm", "set_lm_weights", "beam_hypothesis_lm"):
        assert callable(getattr(capi.Engine, name))
    assert list(inspect.signature(capi.Engine.set_lm).parameters)[1:6] == ["ngrams", "order", "unk_logprob", "weight", "token_bonus"]
    assert "lm" in inspect.signature(capi.Engine.transcribe_beam_mel).parameters and "lm" in inspect.signature(capi.Engine.transcribe_beam).parameters
    assert (capi.LM_MAX_ORDER, capi.LM_BOS, capi.LM_EOS) == (5, 1025, 1026)
    for macro, val in (("NASR_LM_MAX_ORDER", 5), ("NASR_LM_BOS", 1025), ("NASR_LM_EOS", 1026)):
        assert re.search(rf"#define {macro} {val}\b", header)
    rules = (PKG / "csrc" / "nasr_lm.h").read_text()
    assert re.search(r"MAX_ORDER = 5, N_TOKENS = 1024, BLANK_ID = 1024, BOS = 1025, EOS = 1026", rules)
    beam = (PKG / "csrc" / "nasr_beam.h").read_text()
    assert "does not propose" in beam and "does not propose" in header and "prune_allowed" in beam


def test_desc_layout_as_the_c_compiler_sees_it(tmp_path):
    fields = ["order", "flags", "n_ngrams", "lengths", "tokens", "logprob", "backoff", "unk_logprob", "weight", "token_bonus", "reserved"]
    assert [f[0] for f in capi.LmDesc._fields_] == fields
    assert C.sizeof(capi.LmDesc) == 64
    assert [getattr(capi.LmDesc, f).offset for f in fields] == [0, 4, 8, 16, 24, 32, 40, 48, 52, 56, 60]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nemotron_asr_amd.h"\nint main(void) { printf("%zu", sizeof(nasr_lm_desc));\n'
                   + "".join(f'printf(" %zu", offsetof(nasr_lm_desc, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", f"-I{ROOT / 'include'}", "-o", str(exe), str(src)])       # the header is C
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(v) for v in out] == [64, 0, 4, 8, 16, 24, 32, 40, 48, 52, 56, 60]


DRIVER = r"""
#include "lm_arpa.h"
#include "nasr_lm.h"
#include <cstdio>
// <arpa> <pieces file, one per line> [token ..]: "ok order has_unk unk skipped n" + one line per n-gram, then the terms of the token sequence
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    std::vector<std::string> pieces;
    {
        FILE *f = fopen(argv[2], "rb");
        if (!f) return 2;
        std::string cur;
        for (int c; (c = fgetc(f)) != EOF;) { if (c == '\n') { pieces.push_back(cur); cur.clear(); } else cur.push_back((char)c); }
        fclose(f);
    }
    lm_arpa::Model m;
    const std::string err = lm_arpa::parse_file(argv[1], pieces, m);
    if (!err.empty()) { printf("error: %s\n", err.c_str()); return 0; }
    printf("ok %d %d %.9g %lld %zu\n", m.order, (int)m.has_unk, m.unk_logprob, m.skipped_unk, m.lengths.size());
    size_t at = 0;
    for (size_t i = 0; i < m.lengths.size(); at += (size_t)m.lengths[i], i++) {
        for (int j = 0; j < m.lengths[i]; j++) printf("%d ", m.tokens[at + (size_t)j]);
        printf("| %.9g %.9g\n", m.logprob[i], m.backoff[i]);
    }
    nasr_lm::Model lm;
    std::string why;
    if (nasr_lm::build(m.order, (long long)m.lengths.size(), m.lengths.data(), m.tokens.data(), m.logprob.data(), m.backoff.data(), m.has_unk ? m.unk_logprob : -10.0f, lm, why)) {
        printf("build: %s\n", why.c_str());
        return 0;
    }
    const nasr_lm::View v = lm.view();
    int32_t st = v.start;
    printf("terms");
    for (int a = 3; a < argc; a++) printf(" %.17g", nasr_lm::lookup(v, st, atoi(argv[a]), &st));
    printf("\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("lm_arpa")
    src, exe, pieces = d / "driver.cpp", d / "driver", d / "pieces.txt"
    src.write_text(DRIVER)
    pieces.write_text("".join(p + "\n" for p in gguf_io.synthetic_vocab()), encoding="utf-8")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{PKG / 'host'}", f"-I{PKG / 'csrc'}",
                           "-o", str(exe), str(src)])
    return exe, pieces


def run(driver, path, *tokens):
    exe, pieces = driver
    r = subprocess.run([str(exe), str(path), str(pieces)] + [str(t) for t in tokens], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r.stdout.strip().splitlines()


def test_arpa_reader_on_the_golden_file(driver):
    f32 = lambda x: float(np.float32(x))
    want = {(BOS,): (-99, -0.30103), (EOS,): (-1.0, 0), (0,): (-0.5, -0.25), (1,): (-0.75, -0.125), (3,): (-1.25, 0.0625), (700,): (-1.5, -0.5),
            (BOS, 0): (-0.25, -0.125), (0, 1): (-0.5, -0.25), (1, EOS): (-0.625, 0), (3, 700): (-0.875, 0), (1, 3): (-0.375, 0.03125),
            (BOS, 0, 1): (-0.125, 0), (0, 1, EOS): (-0.0625, 0), (0, 1, 3): (-0.1875, 0)}
    seq = [0, 1, 3, 700, 5, 0, 1, EOS]
    lines = run(driver, ARPA, *seq)
    assert lines[0].split()[:3] == ["ok", "3", "1"] and lines[0].split()[4:] == ["0", "14"]
    assert abs(float(lines[0].split()[3]) - (-2.5 * LN10)) <= 1e-6
    got = {}
    for ln in lines[1:15]:
        toks, vals = ln.split("|")
        got[tuple(int(t) for t in toks.split())] = tuple(f32(v) for v in vals.split())          # 9 digits give the float32 back
    assert list(got) == list(want)                                          # the file's order
    for k, (lp, bo) in want.items():
        assert got[k] == (f32(f32(lp) * LN10), f32(f32(bo) * LN10)), k    # log10 as float32, converted in double, rounded to float32
    ref = lm_ref.RefLM({k: v for k, v in got.items()}, 3, f32(-2.5 * LN10))
    assert ref.has_eos and not ref.all_nonpositive
    terms = [float(v) for v in lines[15].split()[1:]]
    hist, exp = ref.start(), []
    for k in seq:
        exp.append(ref.term(hist, k))
        hist += (k,)
    assert lines[15].startswith("terms") and terms == exp
    assert terms[0] == got[(BOS, 0)][0] and terms[1] == got[(BOS, 0, 1)][0] and terms[4] == got[(700,)][1] + ref.unk      # an unknown token backs off to unk


def test_arpa_reader_reports_malformed_files_by_line(driver, tmp_path):
    good = ARPA.read_text(encoding="utf-8")

    def err(text):
        p = tmp_path / "bad.arpa"
        p.write_text(text, encoding="utf-8")
        out = run(driver, p)
        assert out[0].startswith("error: line "), out[0]
        return out[0]

    assert "line 9:" in err(good.replace("-2.5\t<unk>", "x2.5\t<unk>")) and "log-probability" in err(good.replace("-2.5\t<unk>", "x2.5\t<unk>"))
    assert "line 10:" in err(good.replace("-0.5\t▁t0\t-0.25", "-0.5\t▁t0\tnan")) and "back-off" in err(good.replace("-0.5\t▁t0\t-0.25", "-0.5\t▁t0\tnan"))
    assert "line 11:" in err(good.replace("-0.75\tt1\t", "0.75\tt1\t")) and "above 0" in err(good.replace("-0.75\tt1\t", "0.75\tt1\t"))
    assert "not a piece" in err(good.replace("-1.25\t▁t3", "-1.25\tzebra")) and "line 12:" in err(good.replace("-1.25\t▁t3", "-1.25\tzebra"))
    assert "ids:1024" not in good and "0 .. 1023" in err(good.replace("ids:700\t-0.5", "ids:1024\t-0.5"))
    assert "malformed literal id" in err(good.replace("ids:700\t-0.5", "ids:7x\t-0.5"))
    assert "line 16:" in err(good.replace("-0.25\t<s> ▁t0\t-0.125", "-0.25\t▁t0 <s>\t-0.125")) and "<s> inside" in err(good.replace("-0.25\t<s> ▁t0\t-0.125", "-0.25\t▁t0 <s>\t-0.125"))
    assert "</s> before the end" in err(good.replace("-0.625\tt1 </s>", "-0.625\t</s> t1"))
    assert "words" in err(good.replace("-0.875\t▁t3 ids:700", "-0.875\t▁t3"))
    assert "announced 7" in err(good.replace("-1.0\t</s>\n", "")) and "line 14:" in err(good.replace("-1.0\t</s>\n", ""))
    assert "announced 6" in err(good.replace("ngram 2=5", "ngram 2=6"))
    assert "ngram N=count" in err(good.replace("ngram 3=3", "ngram three"))
    assert "outside 1 .. 5" in err(good.replace("ngram 3=3", "ngram 6=3"))
    assert "out of order" in err(good.replace("\\2-grams:", "\\3-grams:", 1))
    assert "unknown section" in err(good.replace("\\2-grams:", "\\two-grams:"))
    assert "no \\end\\" in err(good.replace("\\end\\\n", ""))
    assert "before \\data\\" in err(good.replace("\\data\\", "data")) and "no \\data\\" in err("just text\n")
    assert "not announced" in err(good.replace("ngram 3=3\n", ""))
    # an n-gram whose context is missing passes the reader (it only reads) and fails the builder, which names it
    p = tmp_path / "ctx.arpa"
    p.write_text(good.replace("ngram 2=5", "ngram 2=4").replace("-0.5\t▁t0 t1\t-0.25\n", ""), encoding="utf-8")
    out = run(driver, p)
    assert out[0].startswith("ok") and out[-1].startswith("build: ") and "context" in out[-1]
