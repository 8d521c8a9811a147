#!/usr/bin/env python3
"""What engine option "f32_split_attn" (k_off_attn_f32_split: the offline attention of an F32 engine as three bf16 MFMA products of split operands) buys
and costs.  Three parts, each a process of its own, each writing DIR/f32_split_attn_<part>.json; `report` turns what is there into profiles/f32_split_attn.md.

    python tests/micro/f32_split_attn_cost.py kernel [--dir DIR]   kernel alone: 1-layer F32 engine, 8 utterances of T in {256, 1024, 2048} frames, ms per
                                                                   launch of the attention from the engine's profile (device events), k_off_attn_f32
                                                                   (option off: the launch of the previous build) and k_off_attn_f32_split alternating
    python tests/micro/f32_split_attn_cost.py call   [--dir DIR]   one whole offline call (transcribe_mel, host clock around the synchronous call), F32,
                                                                   24 layers, "f32_split" = 1 in both arms, utterances of 2040, 1024, 512 and 256 frames,
                                                                   option off and on alternating in one process
    python tests/micro/f32_split_attn_cost.py error  [--dir DIR]   last layer's output of one 40 s utterance, 24 layers, against tests/offline_ref.py (the F32
                                                                   oracle): f32, f32_split_attn, f32_split and both
    python tests/micro/f32_split_attn_cost.py report [--dir DIR] [--out profiles/f32_split_attn.md]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
KERNEL_T, KERNEL_B, CALL_T = (256, 1024, 2048), 8, (2040, 1024, 512, 256)
NAMES = {"off": "k_off_attention", "on": "k_off_attention_split"}


def _load():
    import __graft_entry__ as ge
    ge.load_package()
    from nemotron_asr_amd import capi, synth
    return capi, synth


def mel_frames_for(T):
    n = 8 * (T - 3)
    while (((n // 2 + 1) // 2 + 1) // 2 + 1) < T:
        n += 1
    return n


def _engines(capi, W, layers, gemm):
    out = {}
    for arm, v in (("off", 0), ("on", 1)):
        out[arm] = capi.Engine(W, n_layers=layers, dtype=capi.DTYPE_F32, max_streams=1)
        out[arm].set_option("f32_split", gemm)
        out[arm].set_option("f32_split_attn", v)
    return out


def kernel(args):
    capi, synth = _load()
    engs = _engines(capi, synth.make_weights(1), 1, 0)
    rng, out = np.random.default_rng(0), []
    for T in KERNEL_T:
        mels = [rng.standard_normal((mel_frames_for(T), 128)).astype(np.float32) for _ in range(KERNEL_B)]
        ms = {k: [] for k in engs}
        for e in engs.values():          # warm-up of this shape: position table, buffers, code objects
            e.transcribe_mel(mels)
        for _ in range(args.rounds):
            for k, e in engs.items():
                e.profile(True)
                for _ in range(args.steps):
                    e.transcribe_mel(mels)
                a = {p["name"]: p for p in e.profile_read()}[NAMES[k]]
                e.profile(False)
                assert a["launches"] == args.steps
                ms[k].append(a["total_ms"] / a["launches"])
        out.append(dict(T=T, B=KERNEL_B, ms_per_launch=ms, useful_flop=KERNEL_B * 8 * 6.0 * T * T * 128))
        print(json.dumps(out[-1]), flush=True)
    (Path(args.dir) / "f32_split_attn_kernel.json").write_text(json.dumps(out, indent=1))


def call(args):
    capi, synth = _load()
    engs = _engines(capi, synth.make_weights(args.layers, margins="speech"), args.layers, 1)
    rng = np.random.default_rng(1)
    mels = [rng.standard_normal((mel_frames_for(T), 128)).astype(np.float32) for T in CALL_T]
    ms, toks = {k: [] for k in engs}, {}
    for k, e in engs.items():
        toks[k] = e.transcribe_mel(mels)[0]
    for _ in range(args.rounds):
        for k, e in engs.items():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                e.transcribe_mel(mels)
            ms[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
    e = engs["on"]
    e.profile(True)
    e.transcribe_mel(mels)
    prof = sorted(({"name": p["name"], "launches": p["launches"], "ms": round(p["total_ms"], 3)} for p in e.profile_read()), key=lambda r: -r["ms"])[:6]
    out = dict(config=f"F32, {args.layers} layers, f32_split = 1, utterances of {CALL_T} frames", ms_per_call=ms, same_tokens=toks["off"] == toks["on"],
               profile_on=prof)
    print(json.dumps(out), flush=True)
    (Path(args.dir) / "f32_split_attn_call.json").write_text(json.dumps(out, indent=1))


def error(args):
    capi, synth = _load()
    from oracle import binding as ob
    from tests import offline_ref as orf
    L = args.layers
    W = synth.make_weights(L, margins="speech")
    pcm = synth.make_speech_pcm(0, 40.0)[0]
    om = ob.OracleModel(W, L)
    ref = orf.encode(om, W, ob.OraclePreproc(W["preprocessor.featurizer.fb"], W["preprocessor.featurizer.window"]).process(pcm), L)[2]
    want, out = orf.greedy(om, ref), []
    for arm, gemm, attn in (("f32", 0, 0), ("f32_split_attn", 0, 1), ("f32_split", 1, 0), ("f32_split + f32_split_attn", 1, 1)):
        eng = capi.Engine(W, n_layers=L, dtype=capi.DTYPE_F32, max_streams=1)
        eng.set_option("f32_split", gemm)
        eng.set_option("f32_split_attn", attn)
        eng.set_debug(True)
        toks, frames = eng.transcribe([pcm])
        err = np.abs(eng.offline_tap(capi.TAP_ENCODER_OUT, 0).astype(np.float64) - ref)
        eng.close()
        out.append(dict(engine=arm, frames=int(ref.shape[0]), max_abs=float(err.max()), mean_abs=float(err.mean()), ref_rms=float(np.sqrt((ref.astype(np.float64) ** 2).mean())),
                        tokens_equal=(toks[0], frames[0]) == want, ref_tokens=len(want[0])))
        print(json.dumps(out[-1]), flush=True)
    (Path(args.dir) / "f32_split_attn_error.json").write_text(json.dumps(out, indent=1))


def report(args):
    d, lines = Path(args.dir), ["# f32_split_attn: measurements (tests/micro/f32_split_attn_cost.py, MI355X)", ""]
    spread = lambda x: (max(x) - min(x)) / statistics.median(x)      # noqa: E731
    s = lambda x: f"{statistics.median(x):.3f} ({min(x):.3f} .. {max(x):.3f}, {100 * spread(x):.1f} %)"      # noqa: E731
    if (d / "f32_split_attn_kernel.json").exists():
        lines += ["## Attention launch alone, ms (1-layer F32 engine, 8 utterances of T frames; median (min .. max, spread) over alternating regions)", "",
                  "| T | k_off_attn_f32 (option off) | k_off_attn_f32_split | off / on | split, useful TFLOP/s | faster by more than the off arm's spread |", "|---|---|---|---|---|---|"]
        for r in json.loads((d / "f32_split_attn_kernel.json").read_text()):
            off, on = r["ms_per_launch"]["off"], r["ms_per_launch"]["on"]
            lines.append(f"| {r['T']} | {s(off)} | {s(on)} | {statistics.median(off) / statistics.median(on):.1f} | {r['useful_flop'] / statistics.median(on) / 1e9:.1f} | "
                         f"{'yes' if max(on) < min(off) and statistics.median(off) - statistics.median(on) > max(off) - min(off) else 'NO'} |")
        lines.append("")
    if (d / "f32_split_attn_call.json").exists():
        r = json.loads((d / "f32_split_attn_call.json").read_text())
        off, on = r["ms_per_call"]["off"], r["ms_per_call"]["on"]
        lines += ["## One whole offline call, ms (host clock around the synchronous call; alternating regions of one process)", "", "| configuration | off | on | off / on | same tokens |",
                  "|---|---|---|---|---|", f"| {r['config']} | {s(off)} | {s(on)} | {statistics.median(off) / statistics.median(on):.2f} | {r['same_tokens']} |", "",
                  "Largest profile entries of one call with the option on: " + ", ".join(f"{p['name']} {p['ms']} ms" for p in r["profile_on"]) + ".  k_dec_iter is the greedy",
                  "decode, the same in both arms (random mel makes it emit at every frame); the difference between the arms is the 24 attention launches.", ""]
    if (d / "f32_split_attn_error.json").exists():
        lines += ["## Last layer's output against the F32 oracle (offline call, one utterance, 24 layers)", "",
                  "| engine | frames | max abs error | mean abs error | rms of the reference | tokens and frames equal the oracle's |", "|---|---|---|---|---|---|"]
        for r in json.loads((d / "f32_split_attn_error.json").read_text()):
            lines.append(f"| {r['engine']} | {r['frames']} | {r['max_abs']:.3e} | {r['mean_abs']:.3e} | {r['ref_rms']:.3f} | {r['tokens_equal']} ({r['ref_tokens']} tokens) |")
        lines.append("")
    Path(args.out).write_text("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernel", "call", "error", "report"])
    ap.add_argument("--dir", default="bench_out")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "f32_split_attn.md"))
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    Path(args.dir).mkdir(parents=True, exist_ok=True)
    t0 = time.time()
    dict(kernel=kernel, call=call, error=error, report=report)[args.part](args)
    print(f"{args.part}: {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
