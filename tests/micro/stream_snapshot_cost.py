#!/usr/bin/env python3
"""What a stream snapshot costs (24 layers, right_context 13, one chunk pushed, driven through capi.py):

  * nasr_stream_save and nasr_stream_restore of one bf16 stream: the wall time of the call, and between the engine's own events
    (nasr_engine_profile) the pack launch, the device-to-host copy of payload + checksum partials, the unpack launch; host work = the rest;
  * THE ALTERNATIVE the design bets against, built here only: the same segments fetched with one hipMemcpyAsync each into pinned memory and
    checksummed on the host (the formula of csrc/nasr_snapshot.h in C, compiled by this script with the host compiler at -O2);
  * the blob size at bf16 and f32;
  * the time of a synchronous step of 1 and 16 streams, in this tree and -- --other-root TREE, a built tree of the parent commit, timed by a
    child process of its own, alternating with this tree's -- on the parent commit.

    python tests/micro/stream_snapshot_cost.py [--out FILE.json] [--other-root TREE] [--rounds 3] [--passes 2] [--layers 24]

Every timed region: untimed calls first, then K timed calls that end in a device synchronise, host clock; regions alternate over what they
compare, and min .. max over the regions is printed beside the median.  Tables for profiles/stream_snapshot.md on stdout."""
import argparse
import ctypes as C
import json
import shutil
import statistics
import struct
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(HERE))
from stream_fork_cost import MAX_STREAMS, R, Steps, spread  # noqa: E402

HOST_SUM = r"""
#include <stdint.h>
#include <string.h>
static inline uint32_t fmix32(uint32_t h) { h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; return h ^ (h >> 16); }
extern "C" uint64_t host_sum(const uint8_t *p, int64_t bytes, uint32_t word0) {
    uint64_t sum = 0;
    for (int64_t i = 0; i < bytes / 4; i++) { uint32_t w; memcpy(&w, p + 4 * i, 4); sum += fmix32(w ^ (uint32_t)((word0 + (uint32_t)i) * 0x9E3779B1u)); }
    return sum;
}
"""


def stat(eng, name):
    for s in eng.profile_read():
        if s["name"] == name:
            return s
    return dict(launches=0, total_ms=0.0, bytes=0.0)


def segments(n_layers, esz, mel_frames, abuf_cnt):
    """byte sizes of the plan's segments for a stream whose rings have not wrapped, every read-out option off (csrc/nasr_fork_plan.h restated)"""
    segs = []
    for _ in range(n_layers):
        segs += [70 * 1024 * esz, 70 * 1024 * esz, 2 * 8 * 1024 * 4]
    segs += [mel_frames * 128 * 4, -(-abuf_cnt * 4 // 16) * 16, 4, 2 * 193 * 4, 48, 4 * 640 * 4, 4 * 640 * 4, 640 * 4, 4096 * 4, 4096 * 4]
    return [s for s in segs if s]


def alternative(capi, eng, blob, out_dir, n_layers, rounds, K):
    """one hipMemcpyAsync per segment + a host checksum; us per save, median and range over the rounds"""
    mirror_bytes, device_bytes = struct.unpack_from("<QQ", blob, 104)
    abuf_cnt, _, _, mel_count = struct.unpack_from("<4i", blob, 144 + 8)
    segs = segments(n_layers, 2, mel_count, abuf_cnt)
    padded = sum(-(-s // 16) * 16 for s in segs)
    assert padded == device_bytes, (padded, device_bytes)
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        return dict(skipped="no host compiler for the checksum")
    (out_dir / "host_sum.cpp").write_text(HOST_SUM)
    subprocess.check_call([cxx, "-O2", "-shared", "-fPIC", "-o", str(out_dir / "libhost_sum.so"), str(out_dir / "host_sum.cpp")])
    hs = C.CDLL(str(out_dir / "libhost_sum.so")).host_sum
    hs.restype, hs.argtypes = C.c_uint64, [C.c_void_p, C.c_int64, C.c_uint32]
    hip = C.CDLL("libamdhip64.so")
    hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipHostFree.argtypes = [C.c_void_p]
    pinned = C.c_void_p()
    assert hip.hipHostMalloc(C.byref(pinned), device_bytes, 0) == 0
    # the segments lie apart on the device as they do in the pools: every one at a stride of twice its size
    src = eng.upload(np.frombuffer(np.random.default_rng(1).bytes(2 * device_bytes + 64), np.int16))
    copy_us, sum_us, value = [], [], 0
    for r in range(rounds + 1):
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            at_dev = at_host = 0
            for s in segs:
                assert hip.hipMemcpyAsync(pinned.value + at_host, src + at_dev, s, 2, None) == 0          # 2 = device to host
                at_dev += 2 * -(-s // 16) * 16
                at_host += -(-s // 16) * 16
            assert hip.hipStreamSynchronize(None) == 0
        t1 = time.perf_counter()
        for _ in range(K):
            value = hs(pinned, device_bytes, 0)
        t2 = time.perf_counter()
        if r:                                                        # the first round warms up and is dropped
            copy_us.append((t1 - t0) * 1e6 / K)
            sum_us.append((t2 - t1) * 1e6 / K)
    hip.hipHostFree(pinned)
    return dict(segments=len(segs), copies_us=copy_us, host_checksum_us=sum_us, total_us=[a + b for a, b in zip(copy_us, sum_us)], checksum=value)


def child(args):
    sys.path.insert(0, str(Path(args.root).resolve()))
    import __graft_entry__ as ge
    ge.load_package()
    from nemotron_asr_amd import capi, synth
    has = "nasr_stream_save" in capi.EXPORTS
    W = synth.make_weights(args.layers)
    eng = capi.Engine(W, n_layers=args.layers, dtype=capi.DTYPE_BF16, max_streams=MAX_STREAMS)
    n = synth.shift_samples(R)
    pcms = [synth.make_pcm(s, 12 * n / 16000 + 0.01) for s in range(16)]
    out = dict(root=str(args.root), has_snapshot=has, step_ms={}, save={}, restore={})
    for B, K in ((1, 200), (16, 60)):
        st = Steps(capi, synth, eng, B, pcms)
        st.region(max(8, K // 4))
        out["step_ms"][str(B)] = [st.region(K) for _ in range(args.rounds)]
        if has and not args.steps_only and B == 1:
            src, F = st.streams[0], 100
            st.step(n + 9600)                                        # 0.6 s waiting for its right context
            eng.synchronize()
            blob = src.save()
            out["blob_bytes_bf16"], out["bound_bf16"] = len(blob), eng.snapshot_bound()
            out["device_bytes"] = struct.unpack_from("<Q", blob, 112)[0]
            keys = dict(save=("k_stream_pack", "snapshot_d2h"), restore=("k_stream_unpack",))
            for what in ("save", "restore"):
                out[what] = dict(wall_us=[], **{k: [] for k in keys[what]})
            for r in range(args.rounds + 1):                         # the first round warms up and is dropped
                for what in ("save", "restore"):
                    eng.profile(True)
                    before = {k: stat(eng, k) for k in keys[what]}
                    t0 = time.perf_counter()
                    for _ in range(F):
                        if what == "save":
                            src.save()
                        else:
                            eng.restore(blob).destroy()
                    wall = (time.perf_counter() - t0) * 1e6 / F
                    if what == "restore":                            # destroy's share: a stream created from nothing and destroyed costs a reset launch more, so it is measured on its own below
                        t0 = time.perf_counter()
                        for _ in range(F):
                            src.fork().destroy()
                        out.setdefault("fork_destroy_us", []).append((time.perf_counter() - t0) * 1e6 / F)
                    after = {k: stat(eng, k) for k in keys[what]}
                    eng.profile(False)
                    if r:
                        out[what]["wall_us"].append(wall)
                        for k in keys[what]:
                            out[what][k].append((after[k]["total_ms"] - before[k]["total_ms"]) * 1e3 / (after[k]["launches"] - before[k]["launches"]))
            tmp = Path(args.child_out).parent
            out["alternative"] = alternative(capi, eng, blob, tmp, args.layers, args.rounds, 20)
        st.close()
        print(json.dumps({k: v for k, v in out.items() if k != "root"}), flush=True)
    eng.close()
    if has and not args.steps_only:                                  # the f32 blob: its size only
        e32 = capi.Engine(W, n_layers=args.layers, dtype=capi.DTYPE_F32, max_streams=1)
        s32 = e32.stream(R)
        e32.step([s32], [pcms[0][:2 * n + 9600]])
        out["blob_bytes_f32"], out["bound_f32"] = len(s32.save()), e32.snapshot_bound()
        e32.close()
    Path(args.child_out).write_text(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bench_out/stream_snapshot_cost.json")
    ap.add_argument("--other-root", default=None)
    ap.add_argument("--root", default=str(ROOT))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--passes", type=int, default=2, help="child processes per build, alternating between the builds")
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
            if which == "this" and p > 0:
                cmd += ["--steps-only"]                              # the snapshot figures once; the step times in every pass
            subprocess.run(cmd, check=True, timeout=500)             # a fresh process per build: the library is loaded once per process
            runs[which].append(json.loads(tmp.read_text()))
    out.write_text(json.dumps(runs, indent=1))
    t = runs["this"][0]
    print(f"blob: {t['blob_bytes_bf16']} bytes at bf16 (bound {t['bound_bf16']}), {t['blob_bytes_f32']} bytes at f32 (bound {t['bound_f32']}); device section {t['device_bytes']} bytes")
    print()
    print("| | wall us per call (min .. max) | launch, device us | copy of payload + partials, device us |")
    print("|---|---|---|---|")
    print(f"| nasr_stream_save | {spread(t['save']['wall_us'])} | k_stream_pack {spread(t['save']['k_stream_pack'])} | {spread(t['save']['snapshot_d2h'])} |")
    print(f"| nasr_stream_restore + destroy | {spread(t['restore']['wall_us'])} | k_stream_unpack {spread(t['restore']['k_stream_unpack'])} | (inside the wall time) |")
    print(f"| nasr_stream_fork + destroy, for scale | {spread(t['fork_destroy_us'][1:])} | | |")
    alt = t["alternative"]
    if "skipped" not in alt:
        print(f"| the alternative: {alt['segments']} hipMemcpyAsync + host checksum | {spread(alt['total_us'])} | copies {spread(alt['copies_us'])} | host checksum {spread(alt['host_checksum_us'])} |")
    print()
    print("| streams | synchronous step ms, this tree | parent commit |")
    print("|---|---|---|")
    for B in ("1", "16"):
        step = [v for r in runs["this"] for v in r["step_ms"][B]]
        other = [v for r in runs["other"] for v in r["step_ms"][B]]
        print(f"| {B} | {spread(step)} | {spread(other) if other else 'not measured'} |")


if __name__ == "__main__":
    main()
