#!/usr/bin/env python3
"""What a stream fork and a tail preview cost (24 layers, bf16, right_context 13, PCM resident in HBM, driven through capi.py):

  * the device time of k_stream_fork from the engine's own profile (nasr_engine_profile: events around the launch on the engine's stream)
    against the bytes the plan moves, at 16, 64, 128 and 256 KiB per workgroup (engine option "fork_piece_kb"), alternating;
  * the host time of one nasr_stream_fork call;
  * the wall time of one nasr_engine_preview of 1 stream and of 16 streams, each with 0.6 s of audio waiting for its right context;
  * the time of a synchronous step of the same streams, in this tree and -- --other-root TREE, a built tree of the parent commit, timed by
    a child process of its own, alternating with this tree's -- on the parent commit.

    python tests/micro/stream_fork_cost.py [--out FILE.json] [--other-root TREE] [--rounds 3] [--layers 24]

Every timed region: untimed calls first (every graph captured and replayed), then K timed calls that end in a device synchronise, host
clock; regions alternate over what they compare, and min .. max over the regions is printed beside the median.  Table for
profiles/stream_fork.md on stdout."""
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
R, MAX_STREAMS, PRIME = 13, 33, 8
KBS = (16, 64, 128, 256)          # 256 KiB ships (nasr_fork::PIECE_BYTES): every segment one piece


class Steps:
    """B streams stepped one chunk per call from device PCM, as bench.py does"""

    def __init__(self, capi, synth, eng, B, pcms):
        self.capi, self.eng, self.B = capi, eng, B
        self.streams = [eng.stream(R) for _ in range(B)]
        self.n_step = synth.shift_samples(R)
        self.n_avail = pcms[0].size // self.n_step
        self.dev = [eng.upload(p) for p in pcms[:B]]
        self.L = capi.lib()
        self.handles = (C.c_void_p * B)(*[s.h for s in self.streams])
        cap = 16 * (1 + R)
        self.bufs = [np.zeros(cap, np.int32) for _ in range(B)]
        self.tptrs = (C.c_void_p * B)(*[b.ctypes.data for b in self.bufs])
        self.caps = (C.c_int32 * B)(*([cap] * B))
        self.ntok = (C.c_int32 * B)()
        self.k = 0

    def step(self, n=None):
        n = n or self.n_step
        ns = (C.c_int32 * self.B)(*([n] * self.B))
        at = (self.k % (self.n_avail - 1)) * self.n_step
        ptrs = (C.c_void_p * self.B)(*[d + 2 * at for d in self.dev])
        if self.L.nasr_engine_step(self.eng.h, self.handles, self.B, ptrs, ns, self.tptrs, self.caps, self.ntok, self.capi.FLAG_PCM_DEVICE) < 0:
            raise RuntimeError(self.L.nasr_last_error().decode())
        self.k += 1

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


def fork_stat(eng):
    for s in eng.profile_read():
        if s["name"] == "k_stream_fork":
            return s
    return dict(launches=0, total_ms=0.0, bytes=0.0)


def child(args):
    sys.path.insert(0, str(Path(args.root).resolve()))
    import __graft_entry__ as ge
    ge.load_package()
    from nemotron_asr_amd import capi, synth
    has_fork = "nasr_stream_fork" in capi.EXPORTS
    W = synth.make_weights(args.layers)
    eng = capi.Engine(W, n_layers=args.layers, dtype=capi.DTYPE_BF16, max_streams=MAX_STREAMS)
    n = synth.shift_samples(R)
    pcms = [synth.make_pcm(s, 12 * n / 16000 + 0.01) for s in range(16)]
    out = dict(root=str(args.root), has_fork=has_fork, step_ms={}, fork={}, preview_ms={})
    for B, K in ((1, 200), (16, 60)):
        st = Steps(capi, synth, eng, B, pcms)
        st.region(max(8, K // 4))
        out["step_ms"][str(B)] = [st.region(K) for _ in range(args.rounds)]
        if has_fork and not args.steps_only:
            st.step(n + 9600)                                            # 0.6 s waiting for its right context on every stream
            eng.synchronize()
            for _ in range(PRIME):
                eng.preview(st.streams)
            ms = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                for _ in range(K):
                    eng.preview(st.streams)                              # the call synchronises
                ms.append((time.perf_counter() - t0) * 1e3 / K)
            out["preview_ms"][str(B)] = ms
            out.setdefault("preview_tokens", {})[str(B)] = sum(len(t) for t in eng.preview(st.streams))
        if has_fork and not args.steps_only and B == 1:
            src, F = st.streams[0], 200
            for kb in KBS:
                out["fork"][str(kb)] = dict(device_us=[], host_us=[])
            for _ in range(args.rounds + 1):                             # the first round warms up and is dropped
                for kb in KBS:
                    eng.set_option("fork_piece_kb", kb)
                    eng.profile(True)
                    before = fork_stat(eng)
                    t0 = time.perf_counter()
                    for _ in range(F):
                        src.fork().destroy()                             # destroy synchronises the engine's stream
                    host = (time.perf_counter() - t0) * 1e6 / F
                    after = fork_stat(eng)
                    eng.profile(False)
                    rec = out["fork"][str(kb)]
                    rec["device_us"].append((after["total_ms"] - before["total_ms"]) * 1e3 / (after["launches"] - before["launches"]))
                    rec["host_us"].append(host)
                    rec["bytes_moved"] = (after["bytes"] - before["bytes"]) / (after["launches"] - before["launches"]) / 2      # the profile counts read + write
            for kb in KBS:
                out["fork"][str(kb)]["device_us"] = out["fork"][str(kb)]["device_us"][1:]
                out["fork"][str(kb)]["host_us"] = out["fork"][str(kb)]["host_us"][1:]
            eng.set_option("fork_piece_kb", 0)
        st.close()
        print(json.dumps({k: v for k, v in out.items() if k != "root"}), flush=True)
    eng.close()
    Path(args.child_out).write_text(json.dumps(out))


def spread(x):
    return f"{statistics.median(x):.3f} ({min(x):.3f} .. {max(x):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bench_out/stream_fork_cost.json")
    ap.add_argument("--other-root", default=None)
    ap.add_argument("--root", default=str(ROOT))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--passes", type=int, default=1, help="child processes per build, alternating between the builds")
    ap.add_argument("--child-out", default=None)
    ap.add_argument("--steps-only", action="store_true")
    args = ap.parse_args()
    if args.child_out:
        return child(args)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    runs = {"this": [], "other": []}
    for p in range(args.passes):
        for which in (("this", "other") if args.other_root else ("this",)):
            tmp = out.with_suffix(f".{which}{p}.json")
            cmd = [sys.executable, __file__, "--child-out", str(tmp), "--rounds", str(args.rounds), "--layers", str(args.layers)]
            if which == "other":
                cmd += ["--steps-only", "--root", args.other_root]
            subprocess.run(cmd, check=True, timeout=1100)                # a fresh process per build: the library is loaded once per process
            runs[which].append(json.loads(tmp.read_text()))
    out.write_text(json.dumps(runs, indent=1))
    this = runs["this"]
    print("| workgroup moves at most | k_stream_fork device us (min .. max) | MB moved | GB/s | nasr_stream_fork + destroy, host us |")
    print("|---|---|---|---|---|")
    for kb in (str(k) for k in KBS):
        dev = [v for r in this for v in r["fork"][kb]["device_us"]]
        host = [v for r in this for v in r["fork"][kb]["host_us"]]
        mb = this[0]["fork"][kb]["bytes_moved"] / 1e6
        print(f"| {kb} KiB | {spread(dev)} | {mb:.2f} | {2 * mb / 1e3 / (statistics.median(dev) * 1e-6):.0f} read + written | {spread(host)} |")
    print()
    print("| streams | synchronous step ms, this tree | parent commit | preview ms | preview / step |")
    print("|---|---|---|---|---|")
    for B in ("1", "16"):
        step = [v for r in this for v in r["step_ms"][B]]
        other = [v for r in runs["other"] for v in r["step_ms"][B]]
        prev = [v for r in this for v in r["preview_ms"][B]]
        print(f"| {B} | {spread(step)} | {spread(other) if other else 'not measured'} | {spread(prev)} | {statistics.median(prev) / statistics.median(step):.2f} |")


if __name__ == "__main__":
    main()
