#!/usr/bin/env python3
"""What engine option "f32_split_attn_stream" (k_attention_f32_split: the streaming attention of an F32 engine as three bf16 MFMA products of split
operands) buys.  A process of its own, writing DIR/f32_split_attn_stream_kernel.json:

    python tests/micro/f32_split_attn_stream_cost.py kernel [--dir DIR] [--shapes 64x13,64x0]
        24-layer F32 engines with "f32_split" = 1, B streams at right context R (T = 1 + R new rows per stream and step), random audio; ms per attention
        launch from the engine's profile (device events around every launch, steps not pipelined), k_attention<false> (option off: the launch of the
        previous build) and k_attention_f32_split alternating: per round the mean over steps x 24 launches, reported as the median and the range of rounds.

The whole step is bench.py's: --batch 64 --right-context 13 --dtype f32 --checkpoint random --engine-option f32_split=1, with and without
--engine-option f32_split_attn_stream=1, one process per run (profiles/f32_split_attn_stream.md)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
NAMES = {"off": "k_attention", "on": "k_attention_split"}


def kernel(args):
    import __graft_entry__ as ge
    ge.load_package()
    from nemotron_asr_amd import capi, synth
    W, out = synth.make_weights(args.layers), []
    for B, R in [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]:
        piece, T, KV = synth.shift_samples(R), 1 + R, 70 + 1 + R
        rng = np.random.default_rng(B + R)
        ms = {k: [] for k in NAMES}
        engs = {}
        for arm, v in (("off", 0), ("on", 1)):
            e = engs[arm] = capi.Engine(W, n_layers=args.layers, dtype=capi.DTYPE_F32, max_streams=B)
            e.set_option("f32_split", 1)
            e.set_option("f32_split_attn_stream", v)
            e.set_option("pipeline", 0)
        sts = {k: [e.stream(R) for _ in range(B)] for k, e in engs.items()}
        pcm = lambda: [(3000 * rng.standard_normal(piece)).astype(np.int16) for _ in range(B)]
        for k, e in engs.items():          # fill the caches: every later step is a full 70 + T window
            for _ in range(80 // T + 6):
                e.step(sts[k], pcm())
        for _ in range(args.rounds):
            for k, e in engs.items():
                e.profile(True)
                for _ in range(args.steps):
                    e.step(sts[k], pcm())
                a = {p["name"]: p for p in e.profile_read()}[NAMES[k]]
                e.profile(False)
                ms[k].append(a["total_ms"] / a["launches"])
        # useful work of one launch: 3 products of 2 B 8 T KV 128 flop (f32-equivalent); K, V and the position table read once, q read and ctx written
        row = dict(B=B, R=R, T=T, ms_per_launch=ms, useful_flop=3 * 2.0 * B * 8 * T * KV * 128, bytes=4.0 * 1024 * (B * (2 * KV + 2 * T) + KV + T - 1))
        for k in NAMES:
            row[k] = dict(median_ms=statistics.median(ms[k]), min_ms=min(ms[k]), max_ms=max(ms[k]))
        out.append(row)
        print(json.dumps(row), flush=True)
        for e in engs.values():
            e.close()
    Path(args.dir).mkdir(parents=True, exist_ok=True)
    (Path(args.dir) / "f32_split_attn_stream_kernel.json").write_text(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernel"])
    ap.add_argument("--dir", default=str(ROOT / "bench_out"))
    ap.add_argument("--shapes", default="64x13,64x0")
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    kernel(ap.parse_args())
