#!/usr/bin/env python3
"""What engine option "lm_fusion" costs a step: ms per step with the option off, and on with a 3-gram model of about 10^5 n-grams attached
and non-zero weights in both forms of the bias-row refresh -- "fold": extra workgroups of k_dec_pred (the form kept), "own": a launch of its
own per decode iteration (engine option "lm_refresh_fold" = 0); and "relook": the folded refresh with k_dec_commit looking the emitted token up
again instead of reading the next-state row (engine option "lm_commit_lookup" = 1) -- alternating in one process, at 1 stream x R = 0 synchronous and
pipeline = 4, 64 and 512 streams x R = 13 (pipeline 4), and for the offline 64 x 20 s call (24 layers, bf16, speech checkpoint, PCM resident
in HBM, driven through capi.py).  Also the time of one nasr_engine_set_lm with the option on (tables built on the host, uploaded, every row
recomputed).

    python tests/micro/greedy_lm_cost.py [--out FILE.json] [--other-root TREE] [--rounds 3]

Regions and the --other-root protocol are those of tests/micro/phrase_boost_cost.py: 8 untimed steps, then K timed calls and a device
synchronise, host clock; a second built tree (the commit before the option existed) is timed with the option off by a child process of its
own.  The model is random (seeded): it exercises the hash probes and the back-off walk; the transcript changes with it and the symbols
emitted per arm are printed, since a step's decode work grows with them.  Table for profiles/greedy_lm.md on stdout."""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
CONFIGS = [dict(name="1 x R=0 sync", B=1, R=0, K=300, pipeline=0), dict(name="1 x R=0 pipeline 4", B=1, R=0, K=300, pipeline=4),
           dict(name="64 x R=13", B=64, R=13, K=40, pipeline=4), dict(name="512 x R=13", B=512, R=13, K=12, pipeline=4)]
PRIME = 8
WEIGHT, BONUS = 0.3, 1.5


def big_lm(seed=7, n_bi=33000, n_tri=66000):
    """a seeded random 3-gram set of about 10^5 n-grams: every unigram, n_bi bigrams, n_tri trigrams whose context is one of the bigrams"""
    rng = np.random.default_rng(seed)
    items = [((t,), float(-rng.random() * 8.0 - 0.5), float(-rng.random())) for t in range(1024)]
    bi = sorted({(int(a), int(b)) for a, b in rng.integers(0, 1024, size=(n_bi, 2))})
    items += [(k, float(-rng.random() * 5.0 - 0.1), float(-rng.random() * 0.5)) for k in bi]
    tri = sorted({bi[int(i)] + (int(c),) for i, c in zip(rng.integers(0, len(bi), size=n_tri), rng.integers(0, 1024, size=n_tri))})
    items += [(k, float(-rng.random() * 3.0 - 0.05), 0.0) for k in tri]
    return items


class Arm:
    def __init__(self, capi, synth, W, layers, B, R, pcms, mode, pipeline, lm):
        self.capi, self.B = capi, B
        self.eng = capi.Engine(W, n_layers=layers, dtype=capi.DTYPE_BF16, max_streams=B)
        self.set_lm_ms = None
        if mode in ("fold", "own", "relook"):                  # None: a build without the option; "off": the option off
            self.eng.set_option("lm_fusion", 1)
            self.eng.set_option("lm_refresh_fold", 0 if mode == "own" else 1)
            self.eng.set_option("lm_commit_lookup", 1 if mode == "relook" else 0)      # "relook": folded refresh, the commit looks the token up again
            self.eng.synchronize()
            t0 = time.perf_counter()
            self.eng.set_lm(lm, order=3, unk_logprob=-12.0)
            self.set_lm_ms = (time.perf_counter() - t0) * 1e3
            self.eng.set_greedy_lm_weights(WEIGHT, BONUS)
        self.eng.set_option("pipeline", pipeline)
        self.streams = [self.eng.stream(R) for _ in range(B)]
        self.n_step = synth.shift_samples(R)
        self.n_avail = pcms[0].size // self.n_step
        self.dev = [self.eng.upload(p) for p in pcms]
        self.L = capi.lib()
        self.handles = (C.c_void_p * B)(*[s.h for s in self.streams])
        cap = 16 * (1 + R)
        self.bufs = [np.zeros(cap, np.int32) for _ in range(B)]
        self.tptrs = (C.c_void_p * B)(*[b.ctypes.data for b in self.bufs])
        self.caps = (C.c_int32 * B)(*([cap] * B))
        self.ntok = (C.c_int32 * B)()
        self.ns = (C.c_int32 * B)(*([self.n_step] * B))
        self.ptrs = [(C.c_void_p * B)(*[self.dev[s] + 2 * k * self.n_step for s in range(B)]) for k in range(self.n_avail)]
        self.k = self.tokens = 0

    def step(self):
        rc = self.L.nasr_engine_step(self.eng.h, self.handles, self.B, self.ptrs[self.k % self.n_avail], self.ns, self.tptrs, self.caps,
                                     self.ntok, self.capi.FLAG_PCM_DEVICE)
        if rc < 0:
            raise RuntimeError(self.L.nasr_last_error().decode())
        self.k += 1
        self.tokens += sum(self.ntok[b] for b in range(self.B))

    def region(self, K):
        self.eng.synchronize()
        for _ in range(PRIME):
            self.step()
        t0 = time.perf_counter()
        for _ in range(K):
            self.step()
        self.eng.synchronize()
        return (time.perf_counter() - t0) * 1e3 / K

    def close(self):
        for s in self.streams:
            s.destroy()
        self.eng.close()


def offline_call(capi, synth, W, layers, mode, lm, rounds):
    """ms per nasr_engine_transcribe call of 64 utterances of 20 s (host PCM, as a file transcriber gives it)"""
    eng = capi.Engine(W, n_layers=layers, dtype=capi.DTYPE_BF16, max_streams=1)
    if mode in ("fold", "own", "relook"):
        eng.set_option("lm_fusion", 1)
        eng.set_option("lm_refresh_fold", 0 if mode == "own" else 1)
        eng.set_option("lm_commit_lookup", 1 if mode == "relook" else 0)
        eng.set_lm(lm, order=3, unk_logprob=-12.0)
        eng.set_greedy_lm_weights(WEIGHT, BONUS)
    base = [synth.make_speech_pcm(s, 20.0)[0] for s in range(8)]
    pcms = [base[b % 8] for b in range(64)]
    toks = eng.transcribe(pcms)[0]                             # warm-up: buffers grown
    ms = []
    for _ in range(rounds):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.transcribe(pcms)
        ms.append((time.perf_counter() - t0) * 1e3)
    eng.close()
    return ms, sum(len(t) for t in toks)


def child(args):
    sys.path.insert(0, str(Path(args.root).resolve()))
    import __graft_entry__ as ge
    ge.load_package()
    from nemotron_asr_amd import capi, synth
    W = synth.make_weights(args.layers, margins="speech")
    has_option = "nasr_stream_set_lm" in capi.EXPORTS
    modes = ["off" if has_option else None] + (["fold", "own", "relook"] if has_option and not args.off_only else [])
    lm = big_lm() if len(modes) > 1 else None
    out = []
    for cfg in CONFIGS:
        if args.only and args.only not in cfg["name"]:
            continue
        B, R, K = cfg["B"], cfg["R"], max(2, int(cfg["K"] * args.scale))
        n = synth.shift_samples(R)
        n_steps_audio = max(2, int(20.0 * 16000) // n)
        base = [synth.make_speech_pcm(s, n_steps_audio * n / 16000 + 0.01)[0][:n_steps_audio * n] for s in range(min(B, 64))]
        pcms = [base[b % len(base)] for b in range(B)]
        arms = {m or "off": Arm(capi, synth, W, args.layers, B, R, pcms, m, cfg["pipeline"], lm) for m in modes}
        ms = {k: [] for k in arms}
        for k in arms:                                         # warm-up: every graph captured, every shape run
            arms[k].region(max(2, K // 4))
        for _ in range(args.rounds):
            for k in arms:
                ms[k].append(arms[k].region(K))
        rec = dict(config=cfg["name"], B=B, R=R, K=K, ms_per_step=ms, tokens={k: a.tokens for k, a in arms.items()},
                   set_lm_ms={k: a.set_lm_ms for k, a in arms.items()})
        if "own" in arms:
            assert arms["own"].tokens == arms["fold"].tokens == arms["relook"].tokens   # the refresh and commit forms: the same transcript
        for a in arms.values():
            a.close()
        out.append(rec)
        print(json.dumps(rec), flush=True)
    if not args.only or args.only in "offline 64 x 20 s":
        ms, tokens = {}, {}
        for m in modes:
            ms[m or "off"], tokens[m or "off"] = offline_call(capi, synth, W, args.layers, m, lm, args.rounds)
        rec = dict(config="offline 64 x 20 s (ms per call)", ms_per_step=ms, tokens=tokens, set_lm_ms={})
        out.append(rec)
        print(json.dumps(rec), flush=True)
    Path(args.child_out).write_text(json.dumps(out))


def summarise(x):
    med = statistics.median(x)
    return dict(median=med, min=min(x), max=max(x), spread=(max(x) - min(x)) / med, n=len(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bench_out/greedy_lm_cost.json")
    ap.add_argument("--other-root", default=None)
    ap.add_argument("--root", default=str(ROOT))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the timed steps per region")
    ap.add_argument("--only", default=None, help="substring of one configuration's name")
    ap.add_argument("--passes", type=int, default=2, help="child processes per build, alternating between the builds")
    ap.add_argument("--child-out", default=None)
    ap.add_argument("--off-only", action="store_true")
    args = ap.parse_args()
    if args.child_out:
        return child(args)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    runs = {"this": [], "other": []}
    for p in range(args.passes if args.other_root else 1):
        for which in (("this", "other") if args.other_root else ("this",)):
            tmp = out.with_suffix(f".{which}{p}.json")
            cmd = [sys.executable, __file__, "--child-out", str(tmp), "--rounds", str(args.rounds), "--layers", str(args.layers), "--scale", str(args.scale)]
            if args.only:
                cmd += ["--only", args.only]
            if which == "other":
                cmd += ["--off-only", "--root", args.other_root]
            subprocess.run(cmd, check=True, timeout=1100)      # a fresh process per build: the library is loaded once per process
            runs[which].append(json.loads(tmp.read_text()))
    table = []
    for i, rec in enumerate(runs["this"][0]):
        row = dict(config=rec["config"])
        for arm in ("off", "fold", "own", "relook"):
            xs = [v for r in runs["this"] for v in r[i]["ms_per_step"].get(arm, [])]
            if xs:
                row[arm] = summarise(xs)
        xs = [v for r in runs["other"] for v in r[i]["ms_per_step"]["off"]]
        if xs:
            row["other_off"] = summarise(xs)
        row["tokens"], row["set_lm_ms"] = rec.get("tokens"), rec.get("set_lm_ms")
        table.append(row)
    out.write_text(json.dumps(dict(table=table, runs=runs), indent=1))
    print("| configuration | other build, off: ms (min .. max) | this build, off | fused, refresh folded | folded / other off | fused, refresh launch of its own | own / other off | folded, commit looks up again | / other off |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in table:
        f = lambda s: f"{s['median']:.3f} ({s['min']:.3f} .. {s['max']:.3f}, spread {100 * s['spread']:.1f} %)" if s else "-"      # noqa: E731
        ref = r.get("other_off") or r.get("off")
        q = lambda a: f"{r[a]['median'] / ref['median']:.4f}" if a in r else "-"      # noqa: E731
        print(f"| {r['config']} | {f(r.get('other_off'))} | {f(r.get('off'))} | {f(r.get('fold'))} | {q('fold')} | {f(r.get('own'))} | {q('own')} | {f(r.get('relook'))} | {q('relook')} |")
        print(f"    tokens {r['tokens']} set_lm ms {r['set_lm_ms']}")


if __name__ == "__main__":
    main()
