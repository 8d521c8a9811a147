"""host/boost_phrases.h compiled under AddressSanitizer / UBSan (no GPU): words are segmented by greedy longest match against the
vocabulary's pieces starting from their U+2581-prefixed form, `ids:` phrases are taken literally, a phrase that cannot be covered
is reported by line number and skipped, and a boost file is `phrase<TAB>bonus` per line with the bonus optional."""
import json
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "nemotron-asr.cpp_amd" / "host"
SP = "▁"
#         0          1      2     3    4    5        6          7     8    9     10         11
VOCAB = [SP + "he", "llo", "l", "o", SP, SP + "hel", SP + "w", "or", "ld", "w", SP + "hello", "he"]

DRIVER = r"""
#include "boost_phrases.h"
#include <cstring>
// argv: <file with the boost file's content> <default bonus> n_vocab piece...   -> JSON {"phrases": [[line, bonus, [ids]]...], "problems": [...]}
// with "-" as the file: phrases from the list form, remaining argv = n_phrases (text bonus|-)...
static void dump(const boost_phrases::Result &r) {
    printf("{\"phrases\": [");
    for (size_t i = 0; i < r.phrases.size(); i++) {
        printf("%s[%d, %.9g, [", i ? ", " : "", r.phrases[i].line, (double)r.phrases[i].bonus);
        for (size_t k = 0; k < r.phrases[i].tokens.size(); k++) printf("%s%d", k ? ", " : "", r.phrases[i].tokens[k]);
        printf("]]");
    }
    printf("], \"problems\": [");
    for (size_t i = 0; i < r.problems.size(); i++) {
        std::string q;
        for (char c : r.problems[i]) { if (c == '"' || c == '\\') q += '\\'; q += c; }
        printf("%s\"%s\"", i ? ", " : "", q.c_str());
    }
    printf("]}\n");
}
int main(int argc, char **argv) {
    int a = 1;
    const char *path = argv[a++];
    const float def = (float)atof(argv[a++]);
    const int nv = atoi(argv[a++]);
    std::vector<std::string> vocab;
    for (int i = 0; i < nv; i++) vocab.push_back(argv[a++]);
    if (strcmp(path, "-")) {
        boost_phrases::Result r;
        if (!boost_phrases::parse_file(path, vocab, def, r)) { printf("{\"unreadable\": true}\n"); return 0; }
        dump(r);
        return 0;
    }
    const int np = atoi(argv[a++]);
    std::vector<std::string> texts;
    std::vector<float> bonus;
    for (int i = 0; i < np && a + 1 < argc + 1; i++) {
        texts.push_back(argv[a++]);
        const char *b = argv[a++];
        if (strcmp(b, "-")) bonus.push_back((float)atof(b));
    }
    dump(boost_phrases::from_list(texts, bonus, vocab, def));
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("bp")
    (d / "drv.cpp").write_text(DRIVER)
    prog = d / "bp"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{HOST}", str(d / "drv.cpp"), "-o", str(prog)])
    return prog, d


def parse(exe, content, default=4.0, vocab=VOCAB):
    prog, d = exe
    (d / "boost.txt").write_bytes(content.encode() if isinstance(content, str) else content)
    r = subprocess.run([str(prog), str(d / "boost.txt"), repr(default), str(len(vocab)), *vocab], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return json.loads(r.stdout)


def from_list(exe, items, default=4.0, vocab=VOCAB):
    prog, _ = exe
    args = [str(len(items))]
    for text, b in items:
        args += [text, "-" if b is None else repr(b)]
    r = subprocess.run([str(prog), "-", repr(default), str(len(vocab)), *vocab, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_greedy_longest_match_from_the_marked_form(exe):
    got = parse(exe, "hello world\nhel\nhelo\nwow\nhehe\n")
    assert got["problems"] == []
    ids = [p[2] for p in got["phrases"]]
    assert ids[0] == [10, 6, 7, 8]              # "▁hello" beats "▁hel" + "l" + "o" and "▁he" + "llo"; "▁w" "or" "ld"
    assert ids[1] == [5]                        # "▁hel" beats "▁he" + "l"
    assert ids[2] == [5, 3]                     # "▁hel" + "o"
    assert ids[3] == [6, 3, 9]                  # "▁w" + "o" + "w": the unmarked "w" only inside the word
    assert ids[4] == [0, 11]                    # "▁he" + "he"
    assert [p[0] for p in got["phrases"]] == [1, 2, 3, 4, 5] and all(p[1] == 4.0 for p in got["phrases"])


def test_bare_marker_piece_is_used_when_no_marked_piece_fits(exe):
    got = parse(exe, "old\n")
    assert got["problems"] == [] and got["phrases"][0][2] == [4, 3, 8]      # "▁" + "o" + "ld"
    without = [p for p in VOCAB if p != SP]
    got = parse(exe, "old\nhello\n", vocab=without)
    assert len(got["problems"]) == 1 and got["problems"][0].startswith("line 1:") and '"old"' in got["problems"][0]
    assert [p[0] for p in got["phrases"]] == [2]


def test_ids_form_is_literal_and_checked(exe):
    got = parse(exe, "ids:12,55,9\nids: 3 , 1023\nids:1024\nids:\nids:4,,5\nids:7,x\nids:-2\nids:5,\n")
    assert [p[2] for p in got["phrases"]] == [[12, 55, 9], [3, 1023]]
    assert [q.split(":")[0] for q in got["problems"]] == [f"line {n}" for n in (3, 4, 5, 6, 7, 8)]
    assert "1024" in got["problems"][0]


def test_uncoverable_empty_and_too_long_phrases_are_reported_by_line(exe):
    long_ok = " ".join(["hello"] * 32)
    too_long = " ".join(["hello"] * 33)
    got = parse(exe, f"hello\nhexlo\n\n# a comment\nhello z\n{long_ok}\n{too_long}\n\t2.0\nhel")
    assert [p[0] for p in got["phrases"]] == [1, 6, 9]                    # blank and comment lines are counted, not reported
    assert len(got["phrases"][1][2]) == 32 and got["phrases"][2][2] == [5]  # a last line without a newline
    lines = [q.split(":")[0] for q in got["problems"]]
    assert lines == ["line 2", "line 5", "line 7", "line 8"]
    assert '"hexlo"' in got["problems"][0] and '"z"' in got["problems"][1] and "33 tokens" in got["problems"][2] and "empty" in got["problems"][3]


def test_bonus_column_default_and_rejects(exe):
    got = parse(exe, "hello\t2.5\nhel\nhelo\t1e4\nhello\t0\nhello\t-1\nhello\tnan\nhello\tinf\nhello\tabc\nhello\t3 x\nhello\t20000\nhel\t 7.25 \r\n", default=1.5)
    assert [(p[0], p[1]) for p in got["phrases"]] == [(1, 2.5), (2, 1.5), (3, 1e4), (11, 7.25)]
    assert [q.split(":")[0] for q in got["problems"]] == [f"line {n}" for n in range(4, 11)]
    assert parse(exe, "hello\n", default=0.0)["phrases"] == []            # a bad default bonus gives no phrase either


def test_list_form_and_unreadable_file(exe):
    got = from_list(exe, [("hello world", 3.0), ("qq", 2.0), ("hel", -1.0), ("ids:1,2", None)], default=6.0)
    assert got["phrases"] == [[1, 3.0, [10, 6, 7, 8]], [4, 6.0, [1, 2]]]               # a bonus list shorter than the phrases: the default for the rest
    assert [q.split(":")[0] for q in got["problems"]] == ["line 2", "line 3"]
    prog, d = exe
    r = subprocess.run([str(prog), str(d / "no_such_file"), "4.0", "1", "a"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and json.loads(r.stdout) == {"unreadable": True}


def test_first_of_duplicate_pieces_and_blank_row_are_handled(exe):
    vocab = ["a", SP + "a", SP + "a", "b"] + ["x%d" % i for i in range(1020)] + [SP + "zz"]      # id 1024 is the blank's row: never used
    got = parse(exe, "a\nzz\n", vocab=vocab)
    assert got["phrases"] == [[1, 4.0, [1]]]
    assert got["problems"][0].startswith("line 2:")
