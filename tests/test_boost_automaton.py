"""nasr_boost.h (the phrase automaton of engine option "phrase_boost": builder, table layout, lookups), compiled with g++ under
AddressSanitizer / UBSan -- no GPU.

The definition (include/nemotron_asr_amd.h): for an emitted history h, bonus(v) = max w_i over phrases i and 0 <= k < len(p_i) with
p_i[0:k] a suffix of h and p_i[k] == v, else 0; the automaton's state is the longest suffix of h that is a prefix of some phrase.
brute() below evaluates exactly that, by comparing slices of h with slices of the phrases -- it knows nothing of tries or failure
links -- and the tables must agree with it for EVERY vocabulary entry, after every prefix of random histories, bit for bit (a bonus
is one of the w_i, no arithmetic happens to it)."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"
COLS, BLANK, MAXLEN = 1040, 1024, 32
OK, ERR_ARGUMENT, ERR_LENGTH, ERR_TOKEN, ERR_BONUS, ERR_CAPACITY = range(6)

DRIVER = r"""
#include "nasr_boost.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
using namespace nasr_boost;
// in:  "capacity n_phrases" / per phrase "len bonus tok..." / "n_hist" / per history "len tok..."
// out: i32 status, bad_phrase, n_states; depth[n_states]; path[n_states][32]; then for every history and every prefix of it (the empty one
//      first): i32 state, f32 bonus[COLS], i32 next[COLS] -- all read through the lookup functions the kernels use
static void put(FILE *f, const void *p, size_t n) { if (fwrite(p, 1, n, f) != n) abort(); }
int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "null")) {                 // null arguments, and an error leaves the previous automaton alone
        Automaton a;
        const int32_t t0[2] = {3, 4};
        const int32_t *tp[1] = {t0};
        const int32_t len[1] = {2};
        const float w[1] = {1.5f};
        int rc[8], bad = 7;
        rc[0] = build(1, tp, len, w, 16, a, &bad);
        const Automaton keep = a;
        rc[1] = build(1, nullptr, len, w, 16, a);
        rc[2] = build(1, tp, nullptr, w, 16, a);
        rc[3] = build(1, tp, len, nullptr, 16, a);
        rc[4] = build(-1, tp, len, w, 16, a);
        const int32_t *np[1] = {nullptr};
        rc[5] = build(1, np, len, w, 16, a);
        rc[6] = build(1, tp, len, w, 3, a);                      // needs 4 states
        rc[7] = build(1, tp, len, w, 1, a);
        const bool same = a.n_states == keep.n_states && a.bonus == keep.bonus && a.next == keep.next && a.depth == keep.depth;
        printf("%d %d %d %d %d %d %d %d %d %d\n", rc[0], rc[1], rc[2], rc[3], rc[4], rc[5], rc[6], rc[7], same ? 1 : 0, bad);
        return 0;
    }
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int capacity, n;
    if (fscanf(in, "%d %d", &capacity, &n) != 2) return 2;
    std::vector<std::vector<int32_t>> toks((size_t)n);
    std::vector<int32_t> lens((size_t)n);
    std::vector<float> w((size_t)n);
    for (int i = 0; i < n; i++) {
        char wb[64];
        if (fscanf(in, "%d %63s", &lens[(size_t)i], wb) != 2) return 2;
        w[(size_t)i] = strtof(wb, nullptr);                      // "nan", "inf", "-inf" included
        toks[(size_t)i].resize((size_t)(lens[(size_t)i] > 0 ? lens[(size_t)i] : 0) + 1);   // + 1: a pointer to hand over for an empty phrase
        for (int k = 0; k < lens[(size_t)i]; k++) if (fscanf(in, "%d", &toks[(size_t)i][(size_t)k]) != 1) return 2;
    }
    std::vector<const int32_t *> ptr((size_t)n);
    for (int i = 0; i < n; i++) ptr[(size_t)i] = toks[(size_t)i].data();
    Automaton a;
    int bad = -2;
    const int32_t status = build(n, ptr.data(), lens.data(), w.data(), capacity, a, &bad);
    const int32_t head[3] = {status, bad, a.n_states};
    put(out, head, sizeof(head));
    if (status != OK) { fclose(out); return 0; }
    if (a.bonus.size() != table_elems(a.n_states) || a.next.size() != table_elems(a.n_states) || a.n_states > capacity) return 3;
    // every index the layout functions produce, on vectors of exactly table_elems(n_states): ASan guards the bounds
    double touched = 0;
    for (int s = 0; s < a.n_states; s++) {
        for (int v = 0; v < COLS; v++) touched += bonus_of(a.bonus.data(), s, v) + next_of(a.next.data(), s, v);
        for (int nt = 0; nt < 65; nt++)
            for (int q = 0; q < 4; q++) {
                const Bonus4 b = bonus4_of(a.bonus.data(), s, nt * 16 + q * 4);
                const float *row = a.bonus.data() + table_index(s, nt * 16 + q * 4);
                if (b.x != row[0] || b.y != row[1] || b.z != row[2] || b.w != row[3]) return 4;
            }
    }
    for (int t = 0; t < VOCAB; t++) if (raw_part_of(t, 65) != t / 16 || raw_part_of(t, 17) != t / 64 || raw_part_of(t, 65) >= 65 || raw_part_of(t, 17) >= 17) return 5;
    // a state's prefix: a trie edge is a transition that gains one in depth (any other lands on a proper suffix: depth <= the state's)
    std::vector<int32_t> path((size_t)a.n_states * 32, -1), order{STATE_ROOT};
    for (size_t h = 0; h < order.size(); h++) {
        const int s = order[h];
        for (int v = 0; v < BLANK; v++) {
            const int c = next_of(a.next.data(), s, v);
            if (a.depth[(size_t)c] == a.depth[(size_t)s] + 1) {
                for (int k = 0; k < a.depth[(size_t)s]; k++) path[(size_t)c * 32 + k] = path[(size_t)s * 32 + k];
                path[(size_t)c * 32 + a.depth[(size_t)s]] = v;
                order.push_back(c);
            }
        }
    }
    if ((int)order.size() != a.n_states - 1) return 6;            // every state but the disabled one is reached exactly once
    put(out, a.depth.data(), a.depth.size() * 4);
    put(out, path.data(), path.size() * 4);
    int nh;
    if (fscanf(in, "%d", &nh) != 1) return 2;
    for (int i = 0; i < nh; i++) {
        int len;
        if (fscanf(in, "%d", &len) != 1) return 2;
        int32_t s = STATE_ROOT, off = STATE_OFF;
        for (int k = 0; k <= len; k++) {
            put(out, &s, 4);
            put(out, a.bonus.data() + table_index(s, 0), COLS * 4);
            put(out, a.next.data() + table_index(s, 0), COLS * 4);
            if (k == len) break;
            int t;
            if (fscanf(in, "%d", &t) != 1) return 2;
            s = next_of(a.next.data(), s, t);
            off = next_of(a.next.data(), off, t);
            if (off != STATE_OFF) return 7;                       // the disabled state is absorbing
        }
    }
    fclose(out);
    fclose(in);
    return touched == touched ? 0 : 8;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("boost")
    (d / "drv.cpp").write_text(DRIVER)
    out = d / "boost"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{CSRC}", str(d / "drv.cpp"), "-o", str(out)])
    return out, d


def run(exe, phrases, bonus, capacity, hists=()):
    prog, d = exe
    lines = [f"{capacity} {len(phrases)}"]
    for p, w in zip(phrases, bonus):
        lines.append(" ".join([str(len(p)), w if isinstance(w, str) else float(np.float32(w)).hex()] + [str(t) for t in p]))
    lines.append(str(len(hists)))
    for h in hists:
        lines.append(" ".join([str(len(h))] + [str(t) for t in h]))
    (d / "in.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(prog), str(d / "in.txt"), str(d / "out.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    raw = (d / "out.bin").read_bytes()
    status, bad, n_states = struct.unpack_from("<3i", raw, 0)
    if status != OK:
        return dict(status=status, bad=bad)
    o = 12
    depth = np.frombuffer(raw, np.int32, n_states, o); o += 4 * n_states
    path = np.frombuffer(raw, np.int32, n_states * 32, o).reshape(n_states, 32); o += 4 * 32 * n_states
    recs = []
    for h in hists:
        for k in range(len(h) + 1):
            s = struct.unpack_from("<i", raw, o)[0]; o += 4
            b = np.frombuffer(raw, np.float32, COLS, o); o += 4 * COLS
            nx = np.frombuffer(raw, np.int32, COLS, o); o += 4 * COLS
            recs.append((list(h[:k]), s, b, nx))
    assert o == len(raw)
    return dict(status=status, n_states=n_states, depth=depth, path=path, recs=recs)


def brute(phrases, bonus, h):
    """the definition: (bonus of every v, the longest suffix of h + [v] that is a prefix of a phrase for every v, the longest suffix of h that is)"""
    b = np.zeros(BLANK, np.float32)
    nxt = np.zeros(BLANK, np.int64)                         # length of the longest matching suffix of h + [v]
    here = 0
    for p, w in zip(phrases, bonus):
        for k in range(len(p) + 1):
            if k <= len(h) and list(h[len(h) - k:]) == list(p[:k]):      # p[0:k] is a suffix of h (k = 0: the empty suffix)
                here = max(here, k)
                if k < len(p):
                    v = p[k]
                    b[v] = max(b[v], np.float32(w))
                    nxt[v] = max(nxt[v], k + 1)
    return b, nxt, here


def check(got, phrases, bonus, vocab_used):
    depth, path = got["depth"], got["path"]
    prefixes = {tuple(p[:k]) for p in phrases for k in range(1, len(p) + 1)}
    assert got["n_states"] == 2 + len(prefixes)
    assert {tuple(path[s, :depth[s]]) for s in range(2, got["n_states"])} == prefixes
    n = 0
    for h, s, b, nx in got["recs"]:
        wb, wn, here = brute(phrases, bonus, h)
        assert depth[s] == here and list(path[s, :here]) == h[len(h) - here:], (h, s)
        assert b[:BLANK].tobytes() == wb.tobytes(), (h, np.flatnonzero(b[:BLANK] != wb))
        assert not b[BLANK:].any() and (nx[BLANK:] == s).all()               # blank and the padding: no bonus, no move
        assert (depth[nx[:BLANK]] == wn).all(), h
        for v in vocab_used:                                                  # the identity of the next state, not only its depth
            d = int(wn[v])
            assert list(path[nx[v], :d]) == (h + [v])[len(h) + 1 - d:], (h, v)
        n += 1
    return n


def random_set(rng, n_phrases, alphabet, max_len):
    phrases = [[int(t) for t in rng.choice(alphabet, size=int(rng.integers(1, max_len + 1)))] for _ in range(n_phrases)]
    bonus = [float(np.float32(rng.uniform(0.05, 12.0))) for _ in range(n_phrases)]
    return phrases, bonus


@pytest.mark.parametrize("seed", range(8))
def test_small_alphabet_every_entry_after_every_prefix(exe, seed):
    """three or four symbols: overlaps, shared prefixes, phrases inside phrases, repeated tokens and duplicates with other bonuses are the rule"""
    rng = np.random.default_rng(100 + seed)
    alphabet = [5, 6, 700, 1023][:3 + seed % 2]
    phrases, bonus = random_set(rng, int(rng.integers(1, 14)), alphabet, 6 if seed < 6 else MAXLEN)
    phrases.append(list(phrases[0][:1]) * 3)                                                       # a repeated token
    bonus.append(2.5)
    phrases.append(list(phrases[0]))                                                               # a duplicate with another bonus
    bonus.append(bonus[0] + 1.0)
    hists = [[int(t) for t in rng.choice(alphabet + [9], size=40)] for _ in range(12)]             # 9: a token no phrase has
    hists += [list(p) + list(q) for p in phrases[:4] for q in phrases[:4]]
    got = run(exe, phrases, bonus, 4096, hists)
    assert got["status"] == OK
    assert check(got, phrases, bonus, alphabet + [9]) > 400


def test_real_sized_set_over_1024_ids(exe):
    rng = np.random.default_rng(7)
    stems = [[int(t) for t in rng.integers(0, BLANK, size=3)] for _ in range(20)]
    phrases, bonus = [], []
    for i in range(120):                                                                           # about 100 phrases, several hundred states
        tail = [int(t) for t in rng.integers(0, BLANK, size=int(rng.integers(1, 6)))]
        phrases.append((stems[i % 20] if i % 3 else []) + tail)
        bonus.append(float(np.float32(rng.uniform(0.5, 8.0))))
    hists = []
    for _ in range(30):
        h = []
        while len(h) < 30:
            h += phrases[int(rng.integers(len(phrases)))][:int(rng.integers(1, 8))] if rng.random() < 0.7 else [int(rng.integers(0, BLANK))]
        hists.append(h)
    got = run(exe, phrases, bonus, 4096, hists)
    assert got["status"] == OK and 300 < got["n_states"] < 700
    used = sorted({t for p in phrases for t in p})[:64]
    assert check(got, phrases, bonus, used) > 900
    exact = run(exe, phrases, bonus, got["n_states"], [])                                          # the capacity counts the two fixed states
    assert exact["status"] == OK and exact["n_states"] == got["n_states"]
    assert run(exe, phrases, bonus, got["n_states"] - 1, [])["status"] == ERR_CAPACITY


def test_empty_set_is_all_zero_and_disabled_state_absorbs(exe):
    got = run(exe, [], [], 2, [[1, 2, 3, 1023, 0]])
    assert got["status"] == OK and got["n_states"] == 2
    for h, s, b, nx in got["recs"]:
        assert s == 1 and not b.any() and (nx[:BLANK] == 1).all()
    # the driver walks the disabled state beside every history and fails if it ever leaves 0; with phrases too:
    got = run(exe, [[1, 2], [2, 3, 4]], [3.0, 1.0], 16, [[1, 2, 3, 4, 1, 2]])
    assert got["status"] == OK and got["n_states"] == 7 and list(got["depth"][:2]) == [0, 0]


@pytest.mark.parametrize("phrase,bonus,want", [
    ([], 1.0, ERR_LENGTH), (list(range(33)), 1.0, ERR_LENGTH), (list(range(32)), 1.0, OK),
    ([BLANK], 1.0, ERR_TOKEN), ([3, 1025], 1.0, ERR_TOKEN), ([-1], 1.0, ERR_TOKEN), ([1023], 1.0, OK),
    ([3], 0.0, ERR_BONUS), ([3], -1.0, ERR_BONUS), ([3], "nan", ERR_BONUS), ([3], "inf", ERR_BONUS), ([3], "-inf", ERR_BONUS),
    ([3], 1.0001e4, ERR_BONUS), ([3], 1.0e4, OK), ([3], 1e-30, OK),
])
def test_invalid_input_is_rejected_and_names_the_phrase(exe, phrase, bonus, want):
    got = run(exe, [[7, 8], phrase], [1.0, bonus], 64, [])
    assert got["status"] == want
    if want != OK:
        assert got["bad"] == 1


def test_null_arguments_capacity_and_untouched_output(exe):
    prog, _ = exe
    r = subprocess.run([str(prog), "null"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    rc = [int(x) for x in r.stdout.split()]
    assert rc[0] == OK and rc[1:6] == [ERR_ARGUMENT] * 5 and rc[6:8] == [ERR_CAPACITY] * 2
    assert rc[8] == 1                                         # the automaton built first is still what `out` holds
    assert rc[9] == -1                                        # no phrase blamed after a success
