#!/usr/bin/env python3
"""What engine option "f32_split" (k_gemm_f32_split: f32 GEMMs as three bf16 MFMA products of split operands) buys and costs.  Three parts, each a
process of its own, each writing DIR/f32_split_<part>.json; `report` turns what is there into profiles/f32_split.md.

    python tests/micro/f32_split_cost.py kernels [--dir DIR]     kernel alone: k_gemm_f32_mfma against the split kernel (its rule and each forced tile form)
                                                                 at 896 and 7 168 rows x the N x K of W1, W2, QKV and pw1, one launch per fresh upload of
                                                                 the operands (tests/helpers/libgemm_harness.so), kernel time from rocprofv3 --kernel-trace
    python tests/micro/f32_split_cost.py engine  [--dir DIR]     F32 engine, 64 streams x R = 13, 24 layers, synthetic weights: ms per synchronous and per
                                                                 pipelined ("pipeline" = 4) step, option off and on alternating in one process
    python tests/micro/f32_split_cost.py error   [--dir DIR]     last layer's output of the f32, f32_split and bf16 engines against the F32 oracle (max and
                                                                 mean absolute error) on both synthetic checkpoints, 24 layers, 8 streams x R = 13, and the
                                                                 token agreement per stream (reported, not asserted).  --oracle FILE.npz: the oracle's
                                                                 outputs are read from / written to FILE (they need no GPU)
    python tests/micro/f32_split_cost.py report  [--dir DIR] [--out profiles/f32_split.md]
"""
import argparse
import csv
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
SHAPES = {"W1": (4096, 1024), "W2": (1024, 4096), "QKV": (3072, 1024), "pw1": (2048, 1024)}
ROWS = (896, 7168)
VARIANTS = {"f32_mfma": 0, "split (rule)": 2, "split 128x128": 18, "split 64x128": 34, "split 64x64": 50}
REPS = 3


def _load():
    import __graft_entry__ as ge
    ge.load_package()
    from nemotron_asr_amd import capi, synth
    return capi, synth


def kernels_child(args):
    _load()
    from tests import test_gpu_gemm_kernels as G
    L = G.harness()
    labels = []
    for name, (N, K) in SHAPES.items():
        for M in ROWS:
            for var, tile in VARIANTS.items():
                case = G.Case(None, M, N, K, epi=G.PART, f32=True, opts=G._o(f32_fma_tile=tile))
                for _ in range(REPS):
                    G.launch(L, case, "exact")
                    labels.append(dict(shape=name, M=M, N=N, K=K, variant=var))
    Path(args.child_out).write_text(json.dumps(labels))


def kernels(args):
    d = Path(args.dir)
    trace, lab = d / "f32_split_trace", d / "f32_split_labels.json"
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", str(trace), "--", sys.executable, __file__, "kernels", "--child-out", str(lab)],
                   check=True, timeout=900)
    rows = []
    for f in sorted(trace.rglob("*kernel_trace.csv")):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh) if "k_gemm_f32_mfma" in r["Kernel_Name"] or "k_gemm_f32_split" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    labels = json.loads(lab.read_text())
    assert len(rows) == len(labels), (len(rows), len(labels))
    out = {}
    for r, l in zip(rows, labels):
        key = (l["shape"], l["M"], l["variant"])
        rec = out.setdefault(key, dict(l, kernel=r["Kernel_Name"].split("(")[0].replace("void nasr::", ""), us=[]))
        rec["us"].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    (d / "f32_split_kernels.json").write_text(json.dumps(list(out.values()), indent=1))
    for rec in out.values():
        print(rec["shape"], rec["M"], rec["variant"], rec["kernel"], [round(u, 1) for u in rec["us"]])


def _f32_arm(capi, synth, W, layers, B, R, pcms, split, pipeline):
    """token_logprobs_cost.Arm's step() / region() / close() on an F32 engine with the option off or on"""
    import ctypes as C
    from token_logprobs_cost import Arm
    a = Arm.__new__(Arm)
    a.capi, a.B = capi, B
    a.eng = capi.Engine(W, n_layers=layers, dtype=capi.DTYPE_F32, max_streams=B)
    a.eng.set_option("f32_split", split)
    a.eng.set_option("pipeline", pipeline)
    a.streams = [a.eng.stream(R) for _ in range(B)]
    a.n_step = synth.shift_samples(R)
    a.n_avail = pcms[0].size // a.n_step
    a.dev = [a.eng.upload(p) for p in pcms]
    a.L = capi.lib()
    a.handles = (C.c_void_p * B)(*[s.h for s in a.streams])
    cap = 16 * (1 + R)
    a.bufs = [np.zeros(cap, np.int32) for _ in range(B)]
    a.tptrs = (C.c_void_p * B)(*[b.ctypes.data for b in a.bufs])
    a.caps, a.ntok, a.ns = (C.c_int32 * B)(*([cap] * B)), (C.c_int32 * B)(), (C.c_int32 * B)(*([a.n_step] * B))
    a.ptrs = [(C.c_void_p * B)(*[a.dev[s] + 2 * i * a.n_step for s in range(B)]) for i in range(a.n_avail)]
    a.k = a.tokens = 0
    return a


def engine(args):
    capi, synth = _load()
    W = synth.make_weights(args.layers)
    B, R = 64, 13
    n = synth.shift_samples(R)
    n_steps = max(2, int(20.0 * 16000) // n)
    pcms = [synth.make_pcm(s, n_steps * n / 16000 + 0.01)[:n_steps * n] for s in range(B)]
    out = []
    for name, pipeline in (("synchronous", 0), ("pipelined (pipeline = 4)", 4)):
        arms = {arm: _f32_arm(capi, synth, W, args.layers, B, R, pcms, v, pipeline) for arm, v in (("off", 0), ("on", 1))}
        for a in arms.values():          # warm-up: every graph captured, every shape run
            a.region(4)
        ms = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k in arms:
                ms[k].append(arms[k].region(args.steps))
        out.append(dict(config=f"64 x R=13, {args.layers} layers, f32, {name}", K=args.steps, ms_per_step=ms, tokens={k: a.tokens for k, a in arms.items()}))
        print(json.dumps(out[-1]), flush=True)
        for a in arms.values():
            a.close()
    (Path(args.dir) / "f32_split_engine.json").write_text(json.dumps(out, indent=1))


def error(args):
    capi, synth = _load()
    from oracle import binding as ob
    B, R, T, n_steps, L = 8, 13, 14, 5, args.layers
    piece = synth.shift_samples(R)
    cache = Path(args.oracle) if args.oracle else None
    ref = dict(np.load(cache)) if cache and cache.exists() else {}
    out = []
    for ck in ("speech", "random"):
        W = synth.make_weights(L, margins=ck)
        pcms = [synth.make_speech_pcm(b, n_steps * piece / 16000.0 + 0.1)[0][:n_steps * piece] for b in range(B)]
        if f"{ck}_enc" not in ref:
            om = ob.OracleModel(W, L)
            encs, toks = [], []
            for b in range(B):
                ost = ob.OracleStream(om, R)
                _, lay = ost.enable_taps()
                e, t = [], []
                for k in range(n_steps):
                    t += ost.process(pcms[b][k * piece:(k + 1) * piece])
                    if k:                                  # the first push completes no chunk, every later one completes one
                        assert ost.total_chunks == k
                        e.append(lay[L - 1].copy())
                t += ost.finalize()
                encs.append(np.stack(e))
                toks.append(np.array(t + [-1] * (400 - len(t)), np.int32))
            ref[f"{ck}_enc"], ref[f"{ck}_tok"] = np.stack(encs), np.stack(toks)
            if cache:
                np.savez(cache, **ref)
        if args.oracle_only:
            continue
        for arm, dtype, opt in (("f32", capi.DTYPE_F32, 0), ("f32_split", capi.DTYPE_F32, 1), ("bf16", capi.DTYPE_BF16, 0)):
            eng = capi.Engine(W, n_layers=L, dtype=dtype, max_streams=B)
            eng.set_option("f32_split", opt)
            eng.set_debug(True)
            sts = [eng.stream(R) for _ in range(B)]
            toks, encs = [[] for _ in range(B)], [[] for _ in range(B)]
            for k in range(n_steps):
                for b, t in enumerate(eng.step(sts, [p[k * piece:(k + 1) * piece] for p in pcms])):
                    toks[b] += t
                if k:
                    for b, s in enumerate(sts):
                        encs[b].append(s.tap(capi.TAP_LAYER_OUT, L - 1).reshape(T, 1024).copy())
            for b, t in enumerate(eng.finalize(sts)):
                toks[b] += t
            eng.close()
            err = np.abs(np.stack([np.stack(e) for e in encs]).astype(np.float64) - ref[f"{ck}_enc"])
            want = [[int(x) for x in row if x >= 0] for row in ref[f"{ck}_tok"]]
            rec = dict(checkpoint=ck, engine=arm, max_abs=float(err.max()), mean_abs=float(err.mean()), ref_rms=float(np.sqrt((ref[f"{ck}_enc"].astype(np.float64) ** 2).mean())),
                       streams_token_exact=sum(toks[b] == want[b] for b in range(B)), streams=B, ref_tokens=sum(len(w) for w in want))
            out.append(rec)
            print(json.dumps(rec), flush=True)
    if not args.oracle_only:
        (Path(args.dir) / "f32_split_error.json").write_text(json.dumps(out, indent=1))


def report(args):
    d, lines = Path(args.dir), ["# f32_split: measurements (tests/micro/f32_split_cost.py, MI355X)", ""]
    s = lambda x: f"{statistics.median(x):.3f} ({min(x):.3f} .. {max(x):.3f}, {100 * (max(x) - min(x)) / statistics.median(x):.1f} %)"      # noqa: E731
    if (d / "f32_split_kernels.json").exists():
        recs = json.loads((d / "f32_split_kernels.json").read_text())
        lines += ["## Kernel alone, us per launch (median of %d, each after a fresh upload of its operands; rocprofv3 kernel trace)" % REPS, "",
                  "| GEMM | rows | N x K | " + " | ".join(VARIANTS) + " | rule takes | f32_mfma / split (rule) | split TFLOP/s |", "|---|---|---|" + "---|" * (len(VARIANTS) + 3)]
        for name, (N, K) in SHAPES.items():
            for M in ROWS:
                by = {r["variant"]: r for r in recs if r["shape"] == name and r["M"] == M}
                med = {v: statistics.median(by[v]["us"]) for v in VARIANTS}
                lines.append(f"| {name} | {M} | {N} x {K} | " + " | ".join(f"{med[v]:.1f}" for v in VARIANTS) + f" | {by['split (rule)']['kernel']} | "
                             f"{med['f32_mfma'] / med['split (rule)']:.2f} | {2.0 * M * N * K / med['split (rule)'] / 1e6:.0f} |")
        lines.append("")
    if (d / "f32_split_engine.json").exists():
        lines += ["## F32 engine step, ms (median (min .. max, spread) over alternating regions of one process)", "", "| configuration | off | on | off / on |", "|---|---|---|---|"]
        for r in json.loads((d / "f32_split_engine.json").read_text()):
            off, on = r["ms_per_step"]["off"], r["ms_per_step"]["on"]
            lines.append(f"| {r['config']} | {s(off)} | {s(on)} | {statistics.median(off) / statistics.median(on):.2f} |")
        lines.append("")
    if (d / "f32_split_error.json").exists():
        lines += ["## Last layer's output against the F32 oracle (24 layers, 8 streams x R = 13, 4 chunks each)", "",
                  "| checkpoint | engine | max abs error | mean abs error | rms of the reference | streams whose tokens equal the oracle's |", "|---|---|---|---|---|---|"]
        for r in json.loads((d / "f32_split_error.json").read_text()):
            lines.append(f"| {r['checkpoint']} | {r['engine']} | {r['max_abs']:.3e} | {r['mean_abs']:.3e} | {r['ref_rms']:.3f} | {r['streams_token_exact']} of {r['streams']} ({r['ref_tokens']} tokens) |")
        lines.append("")
    Path(args.out).write_text("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernels", "engine", "error", "report"])
    ap.add_argument("--dir", default="bench_out")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "f32_split.md"))
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--oracle", default=None)
    ap.add_argument("--oracle-only", action="store_true")
    ap.add_argument("--child-out", default=None)
    args = ap.parse_args()
    Path(args.dir).mkdir(parents=True, exist_ok=True)
    if args.part == "kernels" and args.child_out:
        return kernels_child(args)
    t0 = time.time()
    dict(kernels=kernels, engine=engine, error=error, report=report)[args.part](args)
    print(f"{args.part}: {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
