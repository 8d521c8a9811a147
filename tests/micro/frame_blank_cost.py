#!/usr/bin/env python3
"""What engine option "frame_blank_logprobs" costs a step: ms per step with both options off, "token_logprobs" = 1 alone, this option
alone, and both, alternating in one process, at 1 stream x R = 0 (synchronous and pipeline = 4) and 64 streams x R = 13 (pipeline = 4)
(24 layers, bf16, speech checkpoint, PCM resident in HBM -- the shapes bench.py times, driven through capi.py).

    python tests/micro/frame_blank_cost.py [--out FILE.json] [--other-root TREE] [--rounds 3]

Every region: 8 untimed steps (refill the step pipeline, replay every graph), then K timed calls and a device synchronise, host clock.
Regions alternate over the arms; the spread of an arm is (max - min) / median over its regions.  --other-root: a second built tree of the
project (the commit before the option existed) is timed with the options off by a child process of its own, alternating with this tree's:
its "off" has to sit inside the spread of this tree's "off".  Table for profiles/frame_blank.md on stdout."""
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
CONFIGS = [dict(name="1 x R=0 synchronous", B=1, R=0, K=200, pipeline=0), dict(name="1 x R=0 pipeline 4", B=1, R=0, K=300, pipeline=4),
           dict(name="64 x R=13 pipeline 4", B=64, R=13, K=40, pipeline=4)]
ARMS = {"off": (0, 0), "token_logprobs": (1, 0), "frame_blank": (0, 1), "both": (1, 1)}
PRIME = 8


class Arm:
    def __init__(self, capi, synth, W, layers, B, R, pcms, pipeline, lp, fb):
        self.capi, self.B = capi, B
        self.eng = capi.Engine(W, n_layers=layers, dtype=capi.DTYPE_BF16, max_streams=B)
        if lp:
            self.eng.set_option("token_logprobs", 1)
        if fb:
            self.eng.set_option("frame_blank_logprobs", 1)
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


def child(args):
    sys.path.insert(0, str(Path(args.root).resolve()))
    import __graft_entry__ as ge
    ge.load_package()
    from nemotron_asr_amd import capi, synth
    W = synth.make_weights(args.layers, margins="speech")
    has_option = "nasr_stream_get_frame_blank_logprobs" in capi.EXPORTS
    out = []
    for cfg in CONFIGS:
        if args.only and args.only not in cfg["name"]:
            continue
        B, R, K = cfg["B"], cfg["R"], max(2, int(cfg["K"] * args.scale))
        n = synth.shift_samples(R)
        n_steps_audio = max(2, int(20.0 * 16000) // n)
        base = [synth.make_speech_pcm(s, n_steps_audio * n / 16000 + 0.01)[0][:n_steps_audio * n] for s in range(min(B, 64))]
        pcms = [base[b % len(base)] for b in range(B)]
        names = list(ARMS) if has_option and not args.off_only else ["off"]
        arms = {k: Arm(capi, synth, W, args.layers, B, R, pcms, cfg["pipeline"], *ARMS[k]) for k in names}
        ms = {k: [] for k in arms}
        for k in arms:                                         # warm-up: every graph captured, every shape run
            arms[k].region(max(2, K // 4))
        for _ in range(args.rounds):
            for k in arms:
                ms[k].append(arms[k].region(K))
        rec = dict(config=cfg["name"], B=B, R=R, K=K, ms_per_step=ms, tokens={k: a.tokens for k, a in arms.items()})
        if "frame_blank" in arms:                              # the values are there and sane; the options change no token
            st = arms["frame_blank"].streams[0]
            total = capi._chk(capi.lib().nasr_stream_get_frame_blank_logprobs(st.h, 0, 0, None))
            v = st.frame_blank_logprobs(max(total - 4096, 0))
            rec["blank_stream0"] = dict(frames=int(total), read=int(v.size), min=float(v.min()), max=float(v.max()), mean_p=float(np.exp(v).mean()))
            assert np.isfinite(v).all() and (v <= 0).all()
            assert len(set(rec["tokens"].values())) == 1, rec["tokens"]
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
    ap.add_argument("--out", default="bench_out/frame_blank_cost.json")
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
        for arm in ARMS:
            xs = [v for r in runs["this"] for v in r[i]["ms_per_step"].get(arm, [])]
            if xs:
                row[arm] = summarise(xs)
        xs = [v for r in runs["other"] for v in r[i]["ms_per_step"]["off"]]
        if xs:
            row["other_off"] = summarise(xs)
        row["blank_stream0"] = rec.get("blank_stream0")
        table.append(row)
    out.write_text(json.dumps(dict(table=table, runs=runs), indent=1))
    print("| configuration | off ms/step (min .. max) | token_logprobs | frame_blank_logprobs | both | frame_blank / off | other build, off |")
    print("|---|---|---|---|---|---|---|")
    for r in table:
        f = lambda s: f"{s['median']:.3f} ({s['min']:.3f} .. {s['max']:.3f}, spread {100 * s['spread']:.1f} %)" if s else "-"      # noqa: E731
        ratio = f"{r['frame_blank']['median'] / r['off']['median']:.4f}" if "frame_blank" in r else "-"
        print(f"| {r['config']} | {f(r.get('off'))} | {f(r.get('token_logprobs'))} | {f(r.get('frame_blank'))} | {f(r.get('both'))} | {ratio} | {f(r.get('other_off'))} |")


if __name__ == "__main__":
    main()
