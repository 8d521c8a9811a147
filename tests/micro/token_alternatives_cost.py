#!/usr/bin/env python3
"""What engine option "token_alternatives" costs: the decode share and the whole step with the option at 0, 4 and 8, alternating in
one process, SYNCHRONOUS steps (no "pipeline": the decode sits on the step's critical path, so its price shows undiluted), at
1 stream x R = 0, 64 streams x R = 13 and (--with-512) 512 streams x R = 13 -- 24 layers, bf16, speech checkpoint, PCM resident in
HBM, driven through capi.py like tests/micro/token_logprobs_cost.py, whose Arm this script shares.

    python tests/micro/token_alternatives_cost.py [--out FILE.json] [--rounds 3] [--with-512]

Whole step: per region 8 untimed steps, then K timed calls and a device synchronise, host clock, graph replay; regions alternate
0, 4, 8, 0, 4, 8, ...; the spread of an arm is (max - min) / median over its regions.
Decode share: nasr_engine_profile (HIP events around every launch class; profiling steps are eager launches) over P steps; the
class "k_dec_iter" holds the decode iterations (LSTM x 2, pred, joint, commit), and the share is its time over the sum of all classes.
Table for profiles/token_alternatives.md on stdout."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
from token_logprobs_cost import Arm  # noqa: E402

CONFIGS = [dict(name="1 x R=0", B=1, R=0, K=300, P=100), dict(name="64 x R=13", B=64, R=13, K=40, P=20),
           dict(name="512 x R=13", B=512, R=13, K=12, P=8)]
KS = (0, 4, 8)


class AltArm(Arm):
    """Arm's step() / region() on an engine that stays synchronous and has "token_alternatives" = k"""

    def __init__(self, capi, synth, B, R, pcms, eng, k):
        self.capi, self.B, self.eng = capi, B, eng
        eng.set_option("token_alternatives", k)
        self.streams = [eng.stream(R) for _ in range(B)]
        self.n_step = synth.shift_samples(R)
        self.n_avail = pcms[0].size // self.n_step
        self.dev = [eng.upload(p) for p in pcms]
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
        dec = sum(s["total_ms"] for s in stats if s["name"] == "k_dec_iter")
        return dec / P, sum(s["total_ms"] for s in stats) / P


def make_arm(capi, synth, W, layers, B, R, pcms, k):
    return AltArm(capi, synth, B, R, pcms, capi.Engine(W, n_layers=layers, dtype=capi.DTYPE_BF16, max_streams=B), k)


def summarise(x):
    med = statistics.median(x)
    return dict(median=med, min=min(x), max=max(x), spread=(max(x) - min(x)) / med, n=len(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bench_out/token_alternatives_cost.json")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the timed steps per region")
    ap.add_argument("--with-512", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    ge.load_package()
    from nemotron_asr_amd import capi, synth
    W = synth.make_weights(args.layers, margins="speech")
    table = []
    for cfg in CONFIGS:
        if cfg["B"] == 512 and not args.with_512:
            continue
        B, R, K, P = cfg["B"], cfg["R"], max(2, int(cfg["K"] * args.scale)), cfg["P"]
        n = synth.shift_samples(R)
        n_steps_audio = max(2, int(20.0 * 16000) // n)
        base = [synth.make_speech_pcm(s, n_steps_audio * n / 16000 + 0.01)[0][:n_steps_audio * n] for s in range(min(B, 64))]
        pcms = [base[b % len(base)] for b in range(B)]
        arms = {k: make_arm(capi, synth, W, args.layers, B, R, pcms, k) for k in KS}
        ms = {k: [] for k in KS}
        for k in KS:                                           # warm-up: every graph captured, every shape run
            arms[k].region(max(2, K // 4))
        for _ in range(args.rounds):
            for k in KS:
                ms[k].append(arms[k].region(K))
        prof = {k: arms[k].profiled(P) for k in KS}
        rec = dict(config=cfg["name"], B=B, R=R, K=K, P=P, step={k: summarise(ms[k]) for k in KS}, raw_ms={k: ms[k] for k in KS},
                   decode_ms={k: prof[k][0] for k in KS}, profiled_ms={k: prof[k][1] for k in KS}, tokens={k: arms[k].tokens for k in KS})
        for k in KS[1:]:                                       # the rows are there and sane
            ids, lps = arms[k].streams[0].token_alternatives(max(arms[k].streams[0].stats().tokens - 64, 0), 64)
            assert ids.shape[1] == k and np.isfinite(lps).all() and (lps <= 0).all() and (np.diff(lps, axis=1) <= 0).all()
        assert len({arms[k].tokens for k in KS}) == 1          # the same decode in every arm
        for a in arms.values():
            a.close()
        table.append(rec)
        print(json.dumps(rec), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(table, indent=1))
    print("| configuration | K | whole step ms (min .. max, spread) | vs 0 | decode ms per step (profiled, eager) | decode share | vs 0 |")
    print("|---|---|---|---|---|---|---|")
    for r in table:
        for k in KS:
            s = r["step"][k]
            print(f"| {r['config']} | {k} | {s['median']:.3f} ({s['min']:.3f} .. {s['max']:.3f}, {100 * s['spread']:.1f} %) | "
                  f"{s['median'] / r['step'][0]['median']:.4f} | {r['decode_ms'][k]:.4f} | {100 * r['decode_ms'][k] / r['profiled_ms'][k]:.1f} % | "
                  f"{r['decode_ms'][k] / r['decode_ms'][0]:.3f} |")


if __name__ == "__main__":
    main()
