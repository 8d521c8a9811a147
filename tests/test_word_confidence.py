"""host/word_confidence.h compiled under AddressSanitizer / UBSan (no GPU): words are cut where tokens_to_text cuts them,
a word's confidence is exp(min ln P of its tokens), ids outside the vocabulary are skipped, NaN (the token has left the
engine's ring) makes the word NaN, empty input gives nothing."""
import json
import math
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "nemotron-asr.cpp_amd" / "host"
SP = "▁"
VOCAB = [SP + "he", "llo", SP + "wor", "l", "d", SP, "!", SP + "a"]

DRIVER = r"""
#include "word_confidence.h"
#include <cstdlib>
#include <cstring>
// the first overload of tokens_to_text in nemo_amd.cpp, restated (that file needs the engine library); the test compares the cuts
static std::string tokens_to_text(const std::vector<int> &tokens, const std::vector<std::string> &vocab) {
    std::string out;
    for (int id : tokens) {
        if (id < 0 || id >= (int)vocab.size()) continue;
        const std::string &piece = vocab[(size_t)id];
        if (piece.compare(0, 3, "\xe2\x96\x81") == 0) { out += ' '; out.append(piece, 3, std::string::npos); }
        else out += piece;
    }
    return out;
}
// argv: n_vocab piece... n_tokens (id lp)...   lp "nan" allowed, "-" = no value (shorter list)
int main(int argc, char **argv) {
    int a = 1;
    const int nv = atoi(argv[a++]);
    std::vector<std::string> vocab;
    for (int i = 0; i < nv; i++) vocab.push_back(argv[a++]);
    const int nt = atoi(argv[a++]);
    std::vector<int> toks;
    std::vector<float> lps;
    for (int i = 0; i < nt; i++) {
        toks.push_back(atoi(argv[a++]));
        const char *v = argv[a++];
        if (strcmp(v, "-")) lps.push_back(!strcmp(v, "nan") ? NAN : (float)atof(v));
    }
    (void)argc;
    const std::vector<word_conf::Word> ws = word_conf::words(toks, lps, vocab);
    std::string joined;
    for (const auto &w : ws) { if (w.opens) joined += ' '; joined += w.text; }
    printf("{\"same_text\": %s, \"annotated\": \"%s\", \"words\": [", joined == tokens_to_text(toks, vocab) ? "true" : "false", word_conf::annotate(ws).c_str());
    for (size_t k = 0; k < ws.size(); k++)
        printf("%s[\"%s\", %d, %d, %d, %s%.9g%s]", k ? ", " : "", ws[k].text.c_str(), ws[k].opens ? 1 : 0, ws[k].first_token, ws[k].n_tokens,
               std::isnan(ws[k].confidence) ? "\"" : "", (double)ws[k].confidence, std::isnan(ws[k].confidence) ? "\"" : "");
    printf("]}\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("wc")
    (d / "drv.cpp").write_text(DRIVER)
    exe = d / "wc"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{HOST}", str(d / "drv.cpp"), "-o", str(exe)])

    def call(tokens, lps):
        args = [str(len(VOCAB)), *VOCAB, str(len(tokens))]
        for i, t in enumerate(tokens):
            args += [str(t), "-" if i >= len(lps) else ("nan" if isinstance(lps[i], float) and math.isnan(lps[i]) else repr(float(lps[i])))]
        r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return json.loads(r.stdout)
    return call


def test_words_are_cut_where_tokens_to_text_cuts_and_take_the_min(run):
    toks = [0, 1, 2, 3, 4, 6, 7]                        # " hello" " world!" " a"
    lps = [-0.1, -0.7, -0.2, -0.05, -1.5, -0.3, -0.01]
    got = run(toks, lps)
    assert got["same_text"]
    words = got["words"]
    assert [w[0] for w in words] == ["hello", "world!", "a"]
    assert [w[2] for w in words] == [0, 2, 6] and [w[3] for w in words] == [2, 4, 1]
    for w, want in zip(words, [math.exp(-0.7), math.exp(-1.5), math.exp(-0.01)]):
        assert abs(w[4] - want) < 1e-6
    assert got["annotated"] == " hello[0.50] world![0.22] a[0.99]"


def test_pieces_before_the_first_marker_and_bare_marker(run):
    got = run([1, 3, 5, 0], [-0.2, -0.4, -0.6, -0.8])   # "llol" + " " + " he"
    assert got["same_text"]
    assert [w[0] for w in got["words"]] == ["llol", "", "he"]
    assert [w[1] for w in got["words"]] == [0, 1, 1]
    assert abs(got["words"][0][4] - math.exp(-0.4)) < 1e-6


def test_out_of_range_ids_are_skipped(run):
    got = run([0, 99, -3, 1, 2], [-0.1, -9.0, -9.0, -0.3, -0.2])
    assert got["same_text"]
    assert [w[0] for w in got["words"]] == ["hello", "wor"]
    assert got["words"][0][3] == 2 and abs(got["words"][0][4] - math.exp(-0.3)) < 1e-6      # the skipped ids' values do not count
    assert got["words"][1][2] == 4


def test_nan_makes_the_word_nan(run):
    got = run([0, 1, 2, 3], [float("nan"), -0.1, -0.2, -0.3])
    assert got["words"][0][4] == "nan" and abs(got["words"][1][4] - math.exp(-0.3)) < 1e-6
    assert got["annotated"] == " hello[nan] worl[0.74]"
    got = run([0, 1, 2], [-0.1, float("nan"), -0.5])
    assert got["words"][0][4] == "nan"
    got = run([0, 1, 2], [-0.1])                        # fewer values than tokens: the rest count as NaN
    assert got["words"][0][4] == "nan" and got["words"][1][4] == "nan"


def test_empty_input(run):
    got = run([], [])
    assert got["same_text"] and got["words"] == [] and got["annotated"] == ""
