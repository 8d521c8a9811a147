#!/usr/bin/env python3
"""What engine option "token_entropy" costs a step: ms per step with the option off, on at alpha = 0.333 and on at alpha = 1, and beside
them "token_logprobs" alone (the LP kernels the option's kernels are forms of), alternating in one process, at
  the headline shape      1 stream x R = 0, "pipeline" = 4 (BASELINE configs[1], what bench.py times)
  a synchronous step      1 stream x R = 0, no pipeline: the decode sits on the step's critical path
  64 streams x R = 13     "pipeline" = 4 (BASELINE configs[2]; 896 rows: the tiled joint kernel)
24 layers, bf16, speech checkpoint, PCM resident in HBM, driven through capi.py like tests/micro/token_logprobs_cost.py, whose Arm
this script extends.

    python tests/micro/token_entropy_cost.py [--out FILE.json] [--other-root TREE] [--rounds 3] [--passes 2]

Every region: 8 untimed steps, then K timed calls and a device synchronise, host clock, graph replay.  Regions alternate over the arms
(off, lp, 333, 1000, off, ...); the spread of an arm is (max - min) / median over its regions of all passes.
--other-root: a second built tree of the project (the parent commit) is timed with every option off by child processes of its own, the
children alternating with this tree's: this tree's "off" has to sit inside the other's spread.
Device time: nasr_engine_profile (HIP events around every launch class; profiling steps are eager launches) over P steps of the
synchronous arms; the class "k_dec_iter" holds the decode iterations (LSTM x 2, pred, joint, commit), whose only launches that differ
between the "lp" and the entropy arms are the joint and the commit.  Table for profiles/token_entropy.md on stdout."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
from token_logprobs_cost import Arm  # noqa: E402

CONFIGS = [dict(name="1 x R=0, pipeline 4", B=1, R=0, K=300, P=0, pipeline=4), dict(name="1 x R=0, synchronous", B=1, R=0, K=300, P=100, pipeline=0),
           dict(name="64 x R=13, pipeline 4", B=64, R=13, K=40, P=0, pipeline=4), dict(name="64 x R=13, synchronous (device time only)", B=64, R=13, K=8, P=20, pipeline=0)]
ARMS = {"off": (), "lp": (("token_logprobs", 1),), "333": (("token_entropy", 333),), "1000": (("token_entropy", 1000),)}


class EntArm(Arm):
    """Arm's step() / region() on an engine with the given options, pipelined or not"""

    def __init__(self, capi, synth, W, layers, B, R, pcms, options, pipeline):
        import ctypes as C
        self.capi, self.B = capi, B
        self.eng = capi.Engine(W, n_layers=layers, dtype=capi.DTYPE_BF16, max_streams=B)
        for k, v in options:
            self.eng.set_option(k, v)
        if pipeline:
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
        self.ptrs = [(C.c_void_p * B)(*[self.dev[s] + 2 * i * self.n_step for s in range(B)]) for i in range(self.n_avail)]
        self.k = self.tokens = 0

    def profiled(self, P):
        """ms per step of the decode class and of all classes, from P eager steps under nasr_engine_profile"""
        self.eng.synchronize()
        self.eng.profile(True)
        for _ in range(P):
            self.step()
        self.eng.synchronize()
        stats = self.eng.profile_read()
        self.eng.profile(False)
        return sum(s["total_ms"] for s in stats if s["name"] == "k_dec_iter") / P, sum(s["total_ms"] for s in stats) / P


def child(args):
    sys.path.insert(0, str(Path(args.root).resolve()))
    import __graft_entry__ as ge
    ge.load_package()
    from nemotron_asr_amd import capi, synth
    W = synth.make_weights(args.layers, margins="speech")
    has_option = "nasr_stream_get_token_entropies" in capi.EXPORTS
    names = ["off"] if args.off_only or not has_option else list(ARMS)
    out = []
    for cfg in CONFIGS:
        if args.only and args.only not in cfg["name"]:
            continue
        if args.off_only and cfg["P"] and cfg["B"] > 1:
            continue
        B, R, K, P = cfg["B"], cfg["R"], max(2, int(cfg["K"] * args.scale)), cfg["P"]
        n = synth.shift_samples(R)
        n_steps_audio = max(2, int(20.0 * 16000) // n)
        base = [synth.make_speech_pcm(s, n_steps_audio * n / 16000 + 0.01)[0][:n_steps_audio * n] for s in range(min(B, 64))]
        pcms = [base[b % len(base)] for b in range(B)]
        arms = {k: EntArm(capi, synth, W, args.layers, B, R, pcms, ARMS[k], cfg["pipeline"]) for k in names}
        ms = {k: [] for k in arms}
        for k in arms:                                         # warm-up: every graph captured, every shape run
            arms[k].region(max(2, K // 4))
        for _ in range(args.rounds):
            for k in arms:
                ms[k].append(arms[k].region(K))
        rec = dict(config=cfg["name"], B=B, R=R, K=K, P=P, ms_per_step=ms, tokens={k: a.tokens for k, a in arms.items()})
        if P and not args.off_only:
            prof = {k: arms[k].profiled(P) for k in arms}
            rec["decode_ms"] = {k: prof[k][0] for k in arms}
            rec["profiled_ms"] = {k: prof[k][1] for k in arms}
        for k in ("333", "1000"):                              # the values are there and sane
            if k in arms:
                h = arms[k].streams[0].token_entropies(max(arms[k].streams[0].stats().tokens - 64, 0), 64)
                rec[f"h_stream0_{k}"] = dict(n=int(h.size), min=float(h.min()) if h.size else None, max=float(h.max()) if h.size else None)
                assert np.isfinite(h).all() and (h >= 0).all() and (h <= 6.9324484).all()
        assert len({a.tokens for a in arms.values()}) == 1     # the same decode in every arm
        for a in arms.values():
            a.close()
        out.append(rec)
        print(json.dumps(rec), flush=True)
    Path(args.child_out).write_text(json.dumps(out))


def summarise(x):
    med = statistics.median(x)
    return dict(median=med, min=min(x), max=max(x), spread=(max(x) - min(x)) / med, n=len(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bench_out/token_entropy_cost.json")
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
    for p in range(args.passes):
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
    for rec in runs["this"][0]:
        same = lambda rs: [r for run in rs for r in run if r["config"] == rec["config"]]      # noqa: E731
        row = dict(config=rec["config"])
        for arm in ARMS:
            xs = [v for r in same(runs["this"]) for v in r["ms_per_step"].get(arm, [])]
            if xs:
                row[arm] = summarise(xs)
        xs = [v for r in same(runs["other"]) for v in r["ms_per_step"]["off"]]
        if xs:
            row["other_off"] = summarise(xs)
        if "decode_ms" in rec:
            row["decode_ms"] = {k: statistics.median(r["decode_ms"][k] for r in same(runs["this"])) for k in rec["decode_ms"]}
            row["profiled_ms"] = {k: statistics.median(r["profiled_ms"][k] for r in same(runs["this"])) for k in rec["profiled_ms"]}
        table.append(row)
    out.write_text(json.dumps(dict(table=table, runs=runs), indent=1))
    f = lambda s: f"{s['median']:.3f} ({s['min']:.3f} .. {s['max']:.3f}, {100 * s['spread']:.1f} %)" if s else "-"      # noqa: E731
    print("| configuration | parent commit, off | off | token_logprobs | token_entropy 333 | token_entropy 1000 | 333 / off | 1000 / off |")
    print("|---|---|---|---|---|---|---|---|")
    for r in table:
        ratio = lambda k: f"{r[k]['median'] / r['off']['median']:.4f}" if k in r else "-"      # noqa: E731
        print(f"| {r['config']} | {f(r.get('other_off'))} | {f(r.get('off'))} | {f(r.get('lp'))} | {f(r.get('333'))} | {f(r.get('1000'))} | {ratio('333')} | {ratio('1000')} |")
    print("\n| configuration | decode ms per step (profiled, eager): off | token_logprobs | token_entropy 333 | token_entropy 1000 | 333 - lp | 1000 - lp |")
    print("|---|---|---|---|---|---|---|")
    for r in table:
        d = r.get("decode_ms")
        if d and "lp" in d:
            print(f"| {r['config']} | {d['off']:.4f} | {d['lp']:.4f} | {d['333']:.4f} | {d['1000']:.4f} | {d['333'] - d['lp']:+.4f} | {d['1000'] - d['lp']:+.4f} |")


if __name__ == "__main__":
    main()
