"""nasr_endpoint.h (the endpoint detector over per-frame blank log-probabilities), compiled with g++ under AddressSanitizer / UBSan into a
stand-alone program and run against a Python restatement of its rules -- no GPU."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"

DRIVER = r"""
#include "nasr_endpoint.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
// <min_blank_logprob | "-inf" | "default"> <idle> <after_speech> <max_len> <first_frame> ; stdin: "lp tokens" per frame, a line "reset" starts
// a new sequence.  Prints "frame utt_start rule tokens" per event, "--" at every reset and at the end.
int main(int argc, char **argv) {
    if (argc < 6) return 1;
    nasr_endpoint::Config cfg;
    if (strcmp(argv[1], "default")) {
        cfg.min_blank_logprob = !strcmp(argv[1], "-inf") ? -INFINITY : (float)atof(argv[1]);
        cfg.silence_frames_idle = atoi(argv[2]); cfg.silence_frames_after_speech = atoi(argv[3]); cfg.max_utterance_frames = atoi(argv[4]);
    } else {
        printf("defaults %d %d %d %d\n", cfg.min_blank_logprob == -INFINITY, cfg.silence_frames_idle, cfg.silence_frames_after_speech, cfg.max_utterance_frames);
    }
    const long long first = atoll(argv[5]);
    nasr_endpoint::State st;
    st.utt_start = first;
    long long frame = first;
    char line[128];
    while (fgets(line, sizeof line, stdin)) {
        if (!strncmp(line, "reset", 5)) { printf("--\n"); st = nasr_endpoint::State(); st.utt_start = first; frame = first; continue; }
        float lp; int tok;
        if (sscanf(line, "%f %d", &lp, &tok) != 2) return 3;
        nasr_endpoint::Event ev;
        if (nasr_endpoint::advance(st, cfg, frame, lp, tok, &ev)) printf("%lld %lld %d %d\n", (long long)ev.frame, (long long)ev.utt_start, ev.rule, ev.tokens);
        frame++;
    }
    printf("--\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("ep")
    (d / "drv.cpp").write_text(DRIVER)
    out = d / "ep"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{CSRC}", str(d / "drv.cpp"), "-o", str(out)])
    return out


def restate(seq, thr, idle, after, max_len, first=0):
    """the rules of nasr_endpoint.h, restated: seq = [(lp_blank f32, tokens_on_frame)], frames numbered from `first`"""
    events, utt_start, tokens, trailing = [], first, 0, 0
    for i, (lp, tok) in enumerate(seq):
        frame = first + i
        silent = tok == 0 and np.float32(lp) >= np.float32(thr)
        trailing = trailing + 1 if silent else 0
        tokens += tok
        rule = 0
        if after > 0 and tokens > 0 and trailing >= after:
            rule = 2
        elif idle > 0 and tokens == 0 and trailing >= idle:
            rule = 1
        elif max_len > 0 and frame - utt_start + 1 >= max_len:
            rule = 3
        if rule:
            events.append((frame, utt_start, rule, tokens))
            utt_start, tokens, trailing = frame + 1, 0, 0
    return events


def run(exe, seqs, thr, idle, after, max_len, first=0):
    text = "reset\n".join("".join(f"{float(np.float32(lp))!r} {tok}\n" for lp, tok in seq) for seq in seqs)
    thr_s = "-inf" if thr == -np.inf else repr(float(np.float32(thr)))
    r = subprocess.run([str(exe), thr_s, str(idle), str(after), str(max_len), str(first)], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr
    out, cur = [], []
    for ln in r.stdout.splitlines():
        if ln == "--":
            out.append(cur); cur = []
        else:
            cur.append(tuple(int(v) for v in ln.split()))
    assert len(out) == len(seqs)
    return out


def random_seqs(n, frames, seed):
    rng = np.random.default_rng(seed)
    seqs = []
    for _ in range(n):
        p_tok = rng.choice([0.02, 0.1, 0.4])                     # sparse, ordinary and dense speech
        tok = (rng.random(frames) < p_tok) * rng.integers(1, 4, frames)
        burst = rng.integers(0, frames, 3)
        for b in burst:
            tok[b:b + rng.integers(5, 40)] = 0                   # stretches of silence long enough for every rule
        lp = -rng.exponential(1.0, frames).astype(np.float32)
        seqs.append(list(zip(lp.tolist(), tok.astype(int).tolist())))
    return seqs


@pytest.mark.parametrize("thr", [-np.inf, -0.7])
def test_random_sequences_match_the_restated_rules(exe, thr):
    seqs = random_seqs(200, 400, 11)
    got = run(exe, seqs, thr, 6, 3, 20)
    want = [restate(s, thr, 6, 3, 20) for s in seqs]
    assert got == want
    rules = {e[2] for ev in want for e in ev}
    assert rules == {1, 2, 3}, rules                             # the sequences reach every rule
    assert sum(len(e) for e in want) > 2000


@pytest.mark.parametrize("limits", [(0, 3, 20), (6, 0, 20), (6, 3, 0), (-1, -1, -1)])
def test_each_rule_disabled_in_turn(exe, limits):
    seqs = random_seqs(40, 400, 5)
    got = run(exe, seqs, -0.7, *limits)
    want = [restate(s, -0.7, *limits) for s in seqs]
    assert got == want
    rules = {e[2] for ev in want for e in ev}
    off = {i + 1 for i, v in enumerate((limits[0], limits[1], limits[2])) if v <= 0}
    assert not (rules & off)
    if limits == (-1, -1, -1):
        assert not rules


def test_token_on_the_very_frame_a_rule_would_fire(exe):
    # idle rule 1 at 6 frames: the token on the sixth frame resets the run, and rule 2 then needs 3 silent frames after it
    seq = [(-0.1, 0)] * 5 + [(-0.1, 1)] + [(-0.1, 0)] * 3
    assert run(exe, [seq], -np.inf, 6, 3, 20) == [[(8, 0, 2, 1)]]
    # rule 2 at 3 frames: a token on the third frame after speech keeps the utterance open and joins it
    seq = [(-0.1, 2)] + [(-0.1, 0)] * 2 + [(-0.1, 1)] + [(-0.1, 0)] * 3
    assert run(exe, [seq], -np.inf, 6, 3, 20) == [[(6, 0, 2, 3)]]
    # rule 3 at 20 frames fires on a frame that carries a token: the token belongs to the utterance that ends there
    seq = [(-0.1, 1), (-0.1, 0)] * 9 + [(-0.1, 0), (-0.1, 4)] + [(-0.1, 0)] * 6
    assert run(exe, [seq], -np.inf, 6, 3, 20) == [[(19, 0, 3, 13), (25, 20, 1, 0)]] == [restate(seq, -np.inf, 6, 3, 20)]


def test_back_to_back_idle_events_in_long_silence(exe):
    seq = [(-0.01, 0)] * 25
    assert run(exe, [seq], -np.inf, 6, 3, 20) == [[(5, 0, 1, 0), (11, 6, 1, 0), (17, 12, 1, 0), (23, 18, 1, 0)]]
    # frames numbered from elsewhere than 0 (a getter window): events carry absolute frames
    assert run(exe, [seq[:13]], -np.inf, 6, 3, 20, first=1000) == [[(1005, 1000, 1, 0), (1011, 1006, 1, 0)]]


def test_threshold(exe):
    # -inf: every token-less frame is silent, however improbable blank was (a 10-cap frame far below -ln 1025, even -inf itself)
    seq = [(-3.0, 1)] + [(-50.0, 0), (-np.inf, 0), (-1e30, 0)]
    assert run(exe, [seq], -np.inf, 6, 3, 20) == [[(3, 0, 2, 1)]]
    # a finite threshold: a token-less frame below it is not silent and restarts the run; equality counts as silent
    seq = [(-0.1, 1), (-0.2, 0), (-0.9, 0), (-0.5, 0), (-0.5, 0), (-0.5, 0)]
    assert run(exe, [seq], -0.5, 6, 3, 20) == [[(5, 0, 2, 1)]]
    # with max_utterance only, nothing but length ends an utterance when no frame is silent
    seq = [(-2.0, 0)] * 45
    assert run(exe, [seq], -0.5, 6, 3, 20) == [[(19, 0, 3, 0), (39, 20, 3, 0)]]


def test_defaults_follow_the_80_ms_convention(exe):
    r = subprocess.run([str(exe), "default", "0", "0", "0", "0"], input="", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr
    assert r.stdout.splitlines()[0] == "defaults 1 30 15 250"
