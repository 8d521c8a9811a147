#!/usr/bin/env python3
"""What engine option "f32_split_planes" (k_gemm_f32_split_planes: the split GEMM on pre-split bf16 hi / lo weight planes) buys.  Two parts, each writing
DIR/f32_split_planes_<part>.json; `report` turns what is there into profiles/f32_split_planes.md.

    python tests/micro/f32_split_planes_cost.py kernels [--dir DIR]   kernel alone, kind 2 (k_gemm_f32_split) against kind 3 at 896 and 7 168 rows x the N x K of W1, W2,
                                                                     QKV, pw1 and Wo: one process, every pair of launches after a fresh upload of its operands
                                                                     (tests/helpers/libgemm_planes_harness.so), kind 2 first and kind 3 first alternating, kernel time
                                                                     from rocprofv3 --kernel-trace
    python tests/micro/f32_split_planes_cost.py step    [--dir DIR]   bench.py --batch 64 --right-context 13 --dtype f32 --checkpoint random with f32_split = 1 and
                                                                     f32_split_attn_stream = 1, without and with f32_split_planes = 1: one process per run, in the order
                                                                     off / on / off / on, pipelined and --sync-steps
    python tests/micro/f32_split_planes_cost.py report  [--dir DIR] [--out profiles/f32_split_planes.md]
"""
import argparse
import csv
import ctypes as C
import json
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
SHAPES = {"W1": (4096, 1024), "W2": (1024, 4096), "QKV": (3072, 1024), "pw1": (2048, 1024), "Wo": (1024, 1024)}
ROWS = (896, 7168)
REPS = 6          # launches per arm: three with kind 2 first, three with kind 3 first
BENCH = ["--gpus", "1", "--steps", "100", "--warmup", "10", "--batch", "64", "--right-context", "13", "--dtype", "f32", "--checkpoint", "random",
         "--engine-option", "f32_split=1", "--engine-option", "f32_split_attn_stream=1", "--no-grouped", "--no-b512", "--no-f32-engine", "--no-host-pcm",
         "--no-cpu-baseline", "--no-profile-pass", "--no-buffered", "--no-extra-configs"]


def kernels_child(args):
    import __graft_entry__ as ge
    ge.load_package()
    from nemotron_asr_amd import capi
    C.CDLL(str(capi.LIB_PATH), mode=C.RTLD_GLOBAL)
    L = C.CDLL(str(ROOT / "tests" / "helpers" / "libgemm_planes_harness.so"))
    L.gemm_planes_run.argtypes = [C.c_int] + [C.c_void_p] * 2 + [C.c_int] * 5 + [C.c_void_p] * 3
    rng, labels = np.random.default_rng(26), []
    for name, (N, K) in SHAPES.items():
        W = rng.uniform(-np.sqrt(3.0 / K), np.sqrt(3.0 / K), (N, K)).astype(np.float32)
        plane = np.empty(N * K, np.float32)
        for M in ROWS:
            A = rng.standard_normal((M, K), dtype=np.float32)
            o2, o3 = np.empty((M, N), np.float32), np.empty((M, N), np.float32)
            for rep in range(REPS):
                first3 = rep & 1          # bit 2 of the harness's form argument: kind 3 is launched first
                assert L.gemm_planes_run(0, A.ctypes.data, W.ctypes.data, M, N, K, K, 4 * first3, o2.ctypes.data, o3.ctypes.data, plane.ctypes.data) == 0
                assert np.array_equal(o2.view(np.uint32), o3.view(np.uint32))
                labels.append(dict(shape=name, M=M, N=N, K=K, first=3 if first3 else 2))
    Path(args.child_out).write_text(json.dumps(labels))


def kernels(args):
    d = Path(args.dir)
    trace, lab = d / "f32_split_planes_trace", d / "f32_split_planes_labels.json"
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", str(trace), "--", sys.executable, __file__, "kernels", "--child-out", str(lab)],
                   check=True, timeout=900)
    rows = []
    for f in sorted(trace.rglob("*kernel_trace.csv")):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh) if "k_gemm_f32_split" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    labels = json.loads(lab.read_text())
    assert len(rows) == 2 * len(labels), (len(rows), len(labels))
    out = {}
    for i, l in enumerate(labels):
        rec = out.setdefault((l["shape"], l["M"]), dict(shape=l["shape"], M=l["M"], N=l["N"], K=l["K"], kernel="", us2=[], us3=[], first=[]))
        for r in rows[2 * i:2 * i + 2]:
            planes = "k_gemm_f32_split_planes" in r["Kernel_Name"]
            rec["us3" if planes else "us2"].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            if planes:
                rec["kernel"] = r["Kernel_Name"].split("(")[0].replace("void nasr::", "")
        rec["first"].append(l["first"])
        assert len(rec["us2"]) == len(rec["us3"])
    (d / "f32_split_planes_kernels.json").write_text(json.dumps(list(out.values()), indent=1))
    for rec in out.values():
        print(rec["shape"], rec["M"], rec["kernel"], "kind 2", [round(u, 1) for u in rec["us2"]], "kind 3", [round(u, 1) for u in rec["us3"]], flush=True)


def step(args):
    d, out = Path(args.dir), []
    for mode, extra in (("pipelined", []), ("synchronous (--sync-steps)", ["--sync-steps"])):
        rec = dict(mode=mode, off=[], on=[], lines=[])
        for arm in ("off", "on", "off", "on"):
            cmd = [sys.executable, str(ROOT / "bench.py")] + BENCH + extra + ["--details", str(d / "f32_split_planes_bench_details.json")]
            if arm == "on":
                cmd += ["--engine-option", "f32_split_planes=1"]
            p = subprocess.run(cmd, check=True, timeout=600, capture_output=True, text=True, cwd=str(ROOT))
            line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            rec["lines"].append(dict(arm=arm, result=line))
            rec[arm].append(line)
            print(mode, arm, json.dumps(line)[:400], flush=True)
            (d / "f32_split_planes_step.json").write_text(json.dumps(out + [rec], indent=1))
        out.append(rec)


def report(args):
    d, lines = Path(args.dir), ["# f32_split_planes: measurements (tests/micro/f32_split_planes_cost.py, MI355X)", ""]
    s = lambda x: f"{statistics.median(x):.1f} ({min(x):.1f}-{max(x):.1f})"      # noqa: E731
    if (d / "f32_split_planes_kernels.json").exists():
        lines += ["## Kernel alone, us per launch: median (min-max) of %d launches per arm, operands freshly uploaded, arms alternating (rocprofv3 kernel trace)" % REPS, "",
                  "| GEMM | rows | N x K | kernel | kind 2 `k_gemm_f32_split` | kind 3 `k_gemm_f32_split_planes` | kind 2 / kind 3 | gain above kind 2's range |", "|---|---|---|---|---|---|---|---|"]
        for r in json.loads((d / "f32_split_planes_kernels.json").read_text()):
            m2, m3 = statistics.median(r["us2"]), statistics.median(r["us3"])
            lines.append(f"| {r['shape']} | {r['M']} | {r['N']} x {r['K']} | `{r['kernel'].replace('k_gemm_f32_split_planes', '')}` | {s(r['us2'])} | {s(r['us3'])} | {m2 / m3:.3f} | "
                         f"{'yes' if m2 - m3 > max(r['us2']) - min(r['us2']) else 'no'} |")
        lines.append("")
    if (d / "f32_split_planes_step.json").exists():
        lines += ["## Whole step: `bench.py " + " ".join(BENCH[:18]) + "` (headline only), one process per run, in the order off / on / off / on", "",
                  "| step | off, ms per step | on, ms per step | audio-s/s off -> on | gain above the off arm's range |", "|---|---|---|---|---|"]
        for r in json.loads((d / "f32_split_planes_step.json").read_text()):
            off, on = [x["ms_per_step"] for x in r["off"]], [x["ms_per_step"] for x in r["on"]]
            lines.append(f"| {r['mode']} | {', '.join(f'{v:.3f}' for v in off)} | {', '.join(f'{v:.3f}' for v in on)} | "
                         f"{statistics.mean(x['value'] for x in r['off']):.0f} -> {statistics.mean(x['value'] for x in r['on']):.0f} | "
                         f"{'yes' if min(off) - max(on) > max(off) - min(off) else 'no'} |")
        lines.append("")
    Path(args.out).write_text("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernels", "step", "report"])
    ap.add_argument("--dir", default=str(ROOT / "bench_out"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "f32_split_planes.md"))
    ap.add_argument("--child-out", default=None)
    args = ap.parse_args()
    Path(args.dir).mkdir(parents=True, exist_ok=True)
    if args.part == "kernels" and args.child_out:
        return kernels_child(args)
    dict(kernels=kernels, step=step, report=report)[args.part](args)


if __name__ == "__main__":
    main()
