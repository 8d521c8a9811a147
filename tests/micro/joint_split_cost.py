#!/usr/bin/env python3
"""What engine option "joint_split" (k_dec_joint_split: the joint's output layer as three bf16 MFMA products of split operands) buys.  Three parts, each writing
DIR/joint_split_<part>.json; `report` turns what is there into profiles/joint_split.md.

    python tests/micro/joint_split_cost.py kernels [--dir DIR]   the joint launch alone at 112, 896 and 16 064 rows, plain and with the softmax parts: one process,
                                                                 PAIRS pairs of launches per case through tests/helpers/libjoint_split_harness.so (out_planes null / set, the
                                                                 order alternating, operands resident as in a decode iteration), kernel time from rocprofv3 --kernel-trace;
                                                                 the first pair of a case is warm-up and is dropped
    python tests/micro/joint_split_cost.py offline [--dir DIR]   tests/micro/offline_probe.py's call -- one nasr_engine_transcribe of 64 x 20 s, 24 layers, bf16 engine fed
                                                                 Q8_0 tensors -- on two engines of one process, option off / on alternating, wall time of the call
    python tests/micro/joint_split_cost.py step    [--dir DIR]   bench.py headline (--batch 1) and --batch 64 --right-context 13, one process per run, off / on / off / on
    python tests/micro/joint_split_cost.py report  [--dir DIR] [--out profiles/joint_split.md]
"""
import argparse
import csv
import ctypes as C
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
CASES = [(B, T, form) for B, T in ((8, 14), (64, 14), (64, 251)) for form in ("plain", "LP")]
PAIRS = 11
BENCH = ["--gpus", "1", "--steps", "100", "--warmup", "10", "--no-grouped", "--no-b512", "--no-f32-engine", "--no-host-pcm", "--no-cpu-baseline", "--no-profile-pass",
         "--no-buffered", "--no-extra-configs"]


def kernels_child(args):
    import __graft_entry__ as ge
    ge.load_package()
    from nemotron_asr_amd import capi
    from tests import decode_kernel_cases as K
    from tests import test_gpu_joint_split as TJ
    C.CDLL(str(capi.LIB_PATH), mode=C.RTLD_GLOBAL)
    L, w = C.CDLL(str(TJ.HELPER)), K.bounded_weights()
    L.joint_split_error.restype = C.c_char_p
    L.joint_split_run.argtypes = [C.c_int, C.POINTER(TJ.JsCase)] + [C.c_void_p] * 16
    for B, T, form in CASES:
        st = K.joint_case(B, T, B * T, False, pool=B + 3)
        BT = B * T
        case = TJ.JsCase(B, T, st["pool"], BT, len(st["boost_bonus"]), 4, int(form == "LP"), 0, 0, 0, 0, PAIRS, 1.0 / 3)
        ins = [np.ascontiguousarray(a) for a in (st["rows"], st["encproj"], st["predg"], w["out_w"], w["out_b"], st["rowmap"], st["boost_bonus"], st["boost_state"], st["lm_row"])]
        outs = [np.zeros(n, np.uint8) for n in (65 * 20 * 2048, 2 * BT * 8, 2 * BT * 17 * 8, 2 * BT * 17 * 32, 2 * BT * 17 * 4, 2 * BT * 17 * 4)]
        assert L.joint_split_run(0, C.byref(case), *(a.ctypes.data for a in ins), *(a.ctypes.data for a in outs), None) == 0, L.joint_split_error()
    Path(args.child_out).write_text(json.dumps([dict(rows=B * T, form=form) for B, T, form in CASES]))


def kernels(args):
    d = Path(args.dir)
    trace, lab = d / "joint_split_trace", d / "joint_split_labels.json"
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", str(trace), "--", sys.executable, __file__, "kernels", "--child-out", str(lab)],
                   check=True, timeout=900)
    rows = []
    for f in sorted(trace.rglob("*kernel_trace.csv")):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh) if "k_dec_joint_tiled" in r["Kernel_Name"] or "k_dec_joint_split" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    labels = json.loads(lab.read_text())
    assert len(rows) == 2 * PAIRS * len(labels), (len(rows), len(labels))
    out = []
    for i, l in enumerate(labels):
        rec = dict(l, off=[], on=[])
        for r in rows[2 * PAIRS * i + 2:2 * PAIRS * (i + 1)]:          # the first pair warms the case up
            rec["on" if "k_dec_joint_split" in r["Kernel_Name"] else "off"].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        assert len(rec["off"]) == len(rec["on"]) == PAIRS - 1
        out.append(rec)
        print(l, "off", [round(u, 1) for u in rec["off"]], "on", [round(u, 1) for u in rec["on"]], flush=True)
    (d / "joint_split_kernels.json").write_text(json.dumps(out, indent=1))


def offline(args):
    import __graft_entry__ as ge
    ge.load_package()
    from nemotron_asr_amd import capi, synth
    WQ = synth.quantize_weights(synth.make_weights(24, margins="speech"), "q8_0")[0]
    pcms = [synth.make_speech_pcm(s, 20.0)[0] for s in range(64)]
    engs, rec = {}, dict(off=[], on=[], same_tokens=None)
    for arm in ("off", "on"):
        engs[arm] = capi.Engine(WQ, n_layers=24, dtype=capi.DTYPE_BF16, max_streams=1)
        engs[arm].set_option("joint_split", int(arm == "on"))
    toks = {arm: e.transcribe(pcms) for arm, e in engs.items()}          # warm-up: position table, buffers
    rec["same_tokens"] = toks["off"] == toks["on"]
    for _ in range(4):
        for arm in ("off", "on"):
            t0 = time.perf_counter()
            engs[arm].transcribe(pcms)
            rec[arm].append((time.perf_counter() - t0) * 1e3)
    print(rec, flush=True)
    (Path(args.dir) / "joint_split_offline.json").write_text(json.dumps(rec, indent=1))


def step(args):
    d, out = Path(args.dir), []
    for name, extra in (("headline (1 stream, R = 0)", []), ("64 streams x R = 13", ["--batch", "64", "--right-context", "13"])):
        rec = dict(config=name, off=[], on=[])
        for arm in ("off", "on", "off", "on"):
            cmd = [sys.executable, str(ROOT / "bench.py")] + BENCH + extra + ["--details", str(d / "joint_split_bench_details.json")] + (["--engine-option", "joint_split=1"] if arm == "on" else [])
            p = subprocess.run(cmd, check=True, timeout=600, capture_output=True, text=True, cwd=str(ROOT))
            rec[arm].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1]))
            print(name, arm, json.dumps(rec[arm][-1])[:300], flush=True)
            (d / "joint_split_step.json").write_text(json.dumps(out + [rec], indent=1))
        out.append(rec)


def report(args):
    d, lines = Path(args.dir), ["# joint_split: measurements (tests/micro/joint_split_cost.py, MI355X)", ""]
    s = lambda x: f"{statistics.median(x):.1f} ({min(x):.1f}-{max(x):.1f})"      # noqa: E731
    gain = lambda off, on: "yes" if statistics.median(off) - statistics.median(on) > max(off) - min(off) else "no"      # noqa: E731
    if (d / "joint_split_kernels.json").exists():
        lines += [f"## (a) The joint launch alone, us: median (min-max) of {PAIRS - 1} launches per arm, arms alternating, operands resident (rocprofv3 kernel trace)", "",
                  "| rows | form | off `k_dec_joint_tiled` | on `k_dec_joint_split` | off / on | gain above the off arm's range |", "|---|---|---|---|---|---|"]
        for r in json.loads((d / "joint_split_kernels.json").read_text()):
            lines.append(f"| {r['rows']} | {r['form']} | {s(r['off'])} | {s(r['on'])} | {statistics.median(r['off']) / statistics.median(r['on']):.2f} | {gain(r['off'], r['on'])} |")
        lines.append("")
    if (d / "joint_split_offline.json").exists():
        r = json.loads((d / "joint_split_offline.json").read_text())
        lines += ["## (b) One offline greedy call, 64 x 20 s, 24 layers, bf16 engine (wall ms of the call, two engines of one process, off / on alternating)", "",
                  f"off {s(r['off'])}, on {s(r['on'])}; gain above the off arm's range: {gain(r['off'], r['on'])}; same tokens: {r['same_tokens']}", ""]
    if (d / "joint_split_step.json").exists():
        lines += ["## (c) `bench.py`, one process per run, in the order off / on / off / on", "", "| configuration | off, ms per step | on, ms per step | gain above the off arm's range |", "|---|---|---|---|"]
        for r in json.loads((d / "joint_split_step.json").read_text()):
            off, on = [x["ms_per_step"] for x in r["off"]], [x["ms_per_step"] for x in r["on"]]
            lines.append(f"| {r['config']} | {', '.join(f'{v:.3f}' for v in off)} | {', '.join(f'{v:.3f}' for v in on)} | {'yes' if min(off) - max(on) > max(off) - min(off) else 'no'} |")
        lines.append("")
    Path(args.out).write_text("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernels", "offline", "step", "report"])
    ap.add_argument("--dir", default=str(ROOT / "bench_out"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "joint_split.md"))
    ap.add_argument("--child-out", default=None)
    args = ap.parse_args()
    Path(args.dir).mkdir(parents=True, exist_ok=True)
    if args.part == "kernels" and args.child_out:
        return kernels_child(args)
    dict(kernels=kernels, offline=offline, step=step, report=report)[args.part](args)


if __name__ == "__main__":
    main()
