#!/usr/bin/env python3
"""bench.py -- RTFx (audio-seconds per wall-second) of the streaming forward path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--batch B --right-context R --dtype bf16] [--dump-outputs DIR] [--full]

A "step" is one pass of the hot path over one batch: every stream of the batch is pushed 1280*(1+R) new PCM samples
(80 ms * (1+R) of audio), which runs PCM->log-mel, one cached encoder chunk (24 layers) and the RNN-T greedy decode for
all B streams in one launch sequence.  Headline workload = BASELINE.json configs[1]: nemotron-0.6B, bf16, batch = 1
stream, 80 ms lookahead (R = 0), full-size seeded synthetic weights and PCM (no checkpoints / audio exist on the box).
PCM is resident in HBM before the timed region starts (NASR_FLAG_PCM_DEVICE); the hand-over of host buffers (H2D inside
the timed region) is reported beside it as `host_pcm`, never as `value`.

Timing: W untimed warm-up steps, then --regions regions of EXACTLY K steps each (one region by default, five with --full),
every region bracketed by a barrier + device synchronisation on both sides, max over ranks per region; `value` is the
median region.  The engine runs consecutive steps
side by side (`pipeline` = 4: a call returns the tokens of the step four calls back), so a region that starts on an idle
device first fills that pipeline and a device synchronise at its end drains it -- a fixed cost per REGION that made the
per-step figure depend on --steps (round 2: 0.49 ms at 20 steps, 0.43 at 200).  The timed interval therefore starts after
the barrier AND `PRIME` further untimed steps that refill the pipeline, and ends when the K-th timed call has returned (its
step-completion lag is the same as at the start): exactly K steps complete in the interval, at any K.  The literal
idle-to-idle figure (K steps from a synchronised device to a synchronised device) is in the line as `cold_ms_per_step`.

Workload data: the "speech" synthetic checkpoint and audio (synth.make_weights(margins="speech"), synth.make_speech_pcm: a
random encoder with trained-network-like residual scaling, a joint fitted to the audio's phone inventory) -- the checkpoint
on which the reduced-precision engines are token-exact against the F32 oracle (`token_agreement`); `--checkpoint random`
selects the near-tie stress checkpoint of rounds 1-2 (same shapes, same kernels, same step time).

A plain run (no --full) does only what the headline needs: set up, warm up, time the K steps, write the outputs
(--dump-outputs DIR: what the last timed step handed its caller, as float .npy files) and print the line.  Everything
below is measured only with --full.

Also in the line with --full (rank 0):
  * `configs`: the other single-GPU configurations BASELINE.json names -- configs[2] (Q8_0 tensors, 64 streams, 1.12 s
    lookahead; with --gpus N this is configs[3]: 64 streams per GPU) and configs[4] (the same + the diarization
    side-car), each with its own roofline;
  * `roofline` (dominant kernel; duration from HIP events on the engine's stream), `cpu_baseline` (the oracle, bounded
    sample) and `token_agreement` (engine tokens vs the F32 oracle on the same audio, with the oracle's top-2 margin at
    the first divergence).

Multi-GPU: `--gpus N` with N > 1 and no WORLD_SIZE in the environment starts N ranks of this script itself
(`python -m torch.distributed.run --nproc-per-node N`, one rank per GPU) BEFORE anything touches the GPU and exits with
their status.  Streams are independent units: rank r owns its own streams on GPU r with replicated weights -- weak
scaling, no data-path collective; torch.distributed (RCCL) only lines the ranks up (barrier) and takes
the max-over-ranks of the elapsed time.

Prints ONE JSON line on rank 0 (with --full ~4 KB: headline, `configs`, `roofline`, `cpu_baseline`, `f32_engine`,
`token_agreement` first; per-kernel tables, every region's time and the notes go to the --details file).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
MFMA_PEAK_TFLOPS = 2500.0      # dense bf16 (spec)
# measured-achievable (MI355X_MICROARCH.md: float4 copy 6.29 TB/s; tests/micro/peaks.py on this pool: hipBLASLt bf16 8192^3 1261 TFLOP/s)
HBM_MEASURED_GBS = 6290.0
MFMA_MEASURED_TFLOPS = 1261.0
REPEATS = 5
ENGINE_OPTIONS = []          # filled from --engine-option
SHM_DIRS = []                # /dev/shm directories of shared weights, removed when the first rank of the node exits


def store_weights(d: Path, W: dict):
    """name -> ndarray | (ggml type id, packed bytes, logical shape), one .npy per tensor + an index; written to a temporary
    directory and renamed, so a reader never sees half a set"""
    import shutil
    tmp = d.with_name(d.name + ".tmp")
    shutil.rmtree(tmp, ignore_errors=True)
    shutil.rmtree(d, ignore_errors=True)
    tmp.mkdir(parents=True)
    try:
        index = []
        for i, (name, v) in enumerate(W.items()):
            arr = v[1] if isinstance(v, tuple) else v
            np.save(tmp / f"{i}.npy", np.ascontiguousarray(arr))
            index.append([name, int(v[0]), list(v[2])] if isinstance(v, tuple) else [name, None, None])
        (tmp / "index.json").write_text(json.dumps(index))
        tmp.rename(d)
    except BaseException:
        shutil.rmtree(tmp, ignore_errors=True)      # RAM-backed files: never leave half a set behind
        raise


def remove_stale_shm(max_age_s=1800.0):
    """/dev/shm/nasr_bench_* left by a run that crashed or was killed (2.4-5 GB of RAM each; round-4 advisor): anything older
    than half an hour goes before this run parks its own"""
    import shutil
    now = time.time()
    for d in Path("/dev/shm").glob("nasr_bench_*"):
        try:
            if now - d.stat().st_mtime > max_age_s:
                shutil.rmtree(d, ignore_errors=True)
        except OSError:
            pass


def load_weights(d: Path) -> dict:
    out = {}
    for i, (name, tid, shape) in enumerate(json.loads((d / "index.json").read_text())):
        a = np.load(d / f"{i}.npy", mmap_mode="r")
        out[name] = a if tid is None else (tid, a, tuple(shape))
    return out


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1, help="streams per GPU")
    ap.add_argument("--right-context", type=int, default=0, choices=[0, 1, 6, 13])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--weights", default="f32", choices=["f32", "f16", "q8_0", "q4_0"],
                    help="GGUF tensor type of the encoder matrices handed to the engine (reference flavours, "
                         "scripts/convert_to_gguf.py:246-263); they are dequantised at upload (bf16 MFMA operands)")
    ap.add_argument("--chunks-per-step", type=int, default=1,
                    help="audio pushed per step, in chunks: > 1 = buffered / file transcription (several chunks of a stream "
                         "go through the layers as one launch sequence)")
    ap.add_argument("--sync-steps", action="store_true",
                    help="every step returns its own tokens before the next one starts (engine option pipeline = 0); default: "
                         "pipelined steps, the decode graph of step s runs on a second HIP stream beside the encoder graph of step s + 1")
    ap.add_argument("--pipeline-depth", type=int, default=4, choices=[1, 2, 3, 4, 8],
                    help="engine option pipeline = E: the encoder in E pieces of L / E layers, piece k of step s beside piece k + 1 of step "
                         "s - 1 ..., the decode of step s - E beside them (1: only the decode beside the next encoder; the engine runs at most as many "
                         "pieces as it finds HIP streams that truly overlap: 4 with the runtime's 4 hardware queues, the decode graphs then run behind the fourth piece)")
    ap.add_argument("--regions", type=int, default=None,
                    help=f"timed regions of K steps (the median is reported; default 1, with --full {REPEATS})")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline (cold / host-PCM / grouped / synchronous figures, the profile pass, "
                         "buffered audio, CPU baseline and token agreement, the f32 engine, the other BASELINE configurations) and write --details")
    ap.add_argument("--details", default="bench_out/bench_details.json",
                    help="--full: file for per-kernel tables, every region's time and the notes (relative: to the repository root)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step handed its caller to DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--checkpoint", default="speech", choices=["speech", "random"],
                    help="speech: joint fitted to the phone inventory of the synthetic speech audio (wide top-2 margins, token-exact "
                         "at reduced precision); random: the near-tie stress checkpoint (N(0, s^2) logits)")
    ap.add_argument("--no-grouped", action="store_true", help="skip the pipeline = 8 (grouped launches) leg of the headline workload")
    ap.add_argument("--no-b512", action="store_true", help="skip the 512- and 256-streams-on-one-GPU entries")
    ap.add_argument("--no-f32-engine", action="store_true", help="skip the f32-engine entry (the configuration that is exact in every bit of its tokens)")
    ap.add_argument("--no-host-pcm", action="store_true", help="skip the host-PCM (H2D inside the timed region) figure")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=60.0,
                    help="audio seconds of the CPU-baseline sample (~10-20 s of CPU work on 16 host threads)")
    ap.add_argument("--no-profile-pass", action="store_true")
    ap.add_argument("--no-buffered", action="store_true", help="skip the buffered-audio (file transcription) figure")
    ap.add_argument("--no-extra-configs", action="store_true", help="headline only: skip the configs[2] / configs[4] entries")
    ap.add_argument("--extra-steps", type=int, default=200, help="timed steps per region of the extra configurations")
    ap.add_argument("--diarize", action="store_true",
                    help="BASELINE config 5 on the HEADLINE workload too: also time the diarization side-car on each step's audio")
    ap.add_argument("--stream-offset", type=int, default=0,
                    help="first stream id of rank 0 (to re-run one rank's streams of an N-rank job in a single process: rank r owns offset + r B ...)")
    ap.add_argument("--share-device", type=int, default=-1, metavar="D",
                    help="rehearsal of the N > 1 path on a box with ONE GPU: every rank runs its engine on device D and the ranks meet over gloo "
                         "(RCCL refuses two ranks on one device); the line says so in config.parallelism")
    ap.add_argument("--engine-option", action="append", default=[], metavar="KEY=VALUE",
                    help="nasr_engine_set_option on every engine of the run before its first step (gemm_cores, persistent_gemm, f32_mfma, ...)")
    ap.add_argument("--master-port", type=int, default=0, help="rendezvous port of the ranks started by --gpus N (0: pick a free one)")
    ap.add_argument("--stub-engine", action="store_true",
                    help=argparse.SUPPRESS)   # launch-path test only (tests/test_bench_launch.py): no GPU, gloo, a sleeping stand-in
    return ap.parse_args(argv)


# ---- multi-rank launcher -------------------------------------------------------------------------------------------
def launch_ranks(args) -> int:
    """--gpus N without a torchrun environment: start N ranks of this script.  Runs before load_package(), torch.cuda or
    any HIP call in this process (a process that has initialised the GPU must neither fork ranks nor exec); the parent
    only waits and hands on the exit status."""
    port = args.master_port
    if not port:
        import socket
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
    argv = [a for a in sys.argv[1:]]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve())] + argv
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(args.gpus, 1))))
    return subprocess.run(cmd, env=env).returncode


# ---- a stand-in engine for the launch-path test (never the product path) -------------------------------------------
class _StubEngine:
    """sleeps instead of computing: exercises argument handling, the rank launcher, barriers and the JSON line on a box
    without a GPU.  Selected only by the hidden --stub-engine flag; the line it prints says so."""

    def __init__(self, B):
        self.B = B

    def step(self):
        time.sleep(0.0005)

    def synchronize(self):
        pass


def pmc_traffic(kernel_symbol_part, tag):
    """HBM bytes per launch of a kernel from the rocprofv3 --pmc passes committed under profiles/ for THIS build
    (profiles/r4_pmc_traffic_<tag>.json, written by tests/prof_r4.sh: FETCH_SIZE x 2 + WRITE_SIZE as
    MI355X_MICROARCH.md prescribes for gfx950).  PMC counters cannot be collected from inside this process; null when no
    summary for the configuration / kernel is committed."""
    f = next((c for c in (ROOT / "profiles" / f"r6_pmc_traffic_{tag}.json", ROOT / "profiles" / f"r5_pmc_traffic_{tag}.json", ROOT / "profiles" / f"r4_pmc_traffic_{tag}.json") if c.exists()), None)
    if f is None:
        return None
    try:
        ks = json.loads(f.read_text())["kernels"]
    except (ValueError, KeyError):
        return None
    tot, n = 0.0, 0                       # a HIP-event category can cover several kernel symbols (k_gemm_roles / k_gemm_t64 / k_gemm_tiled2): launch-weighted mean
    for name, rec in ks.items():
        if any(part in name for part in kernel_symbol_part) and "hbm_bytes_per_launch_corrected" in rec:
            tot += rec["hbm_bytes_per_launch_corrected"] * rec.get("launches_FETCH_SIZE", 1)
            n += rec.get("launches_FETCH_SIZE", 1)
    return round(tot / n) if n else None


def timed_regime_block(tag, depth, ms_per_step, sr):
    """The regime `value` is timed in (E lanes: pieces of consecutive steps side by side), with its own kernel-level evidence: the
    rocprofv3 --kernel-trace of the same command, reduced by tests/prof_r5.sh to profiles/r5_<tag>_pipelined_trace.json (sum of kernel
    durations per step over all lanes, the wall time those kernels cover, how many run at a time).  The whole-step fraction is what the
    headline stands for; the `roofline` block is the dominant kernel ALONE on the chip (synchronous regime)."""
    if not depth:
        return None
    out = dict(regime=f"pipelined, {depth} lanes", ms_per_step=ms_per_step, hbm_frac=sr["hbm_frac"], mfma_frac=sr["mfma_frac"])
    f = ROOT / "profiles" / f"r5_{tag}_pipelined_trace.json"
    if f.exists():
        try:
            t = json.loads(f.read_text())
            out.update(kernel_ms_per_step=t["kernel_ms_per_step"], avg_kernels_in_flight=t.get("avg_kernels_in_flight"), in_flight_share=t.get("in_flight_share"),
                       stamped_ms_per_step=t["ms_per_step"], dominant=t["dominant"], source=f"profiles/{f.name}")
        except (ValueError, KeyError):
            pass
    return out


_SYMBOL = {"k_fused_ln_gemm": ("k_fused_skinny<0,",), "k_fused_plain_gemm": ("k_fused_skinny<1,",), "k_fused_attn_gemm": ("k_fused_skinny<2,",),
           "k_fused_dwconv_gemm": ("k_fused_skinny<3,",), "k_gemm_tiled": ("k_gemm_roles", "k_gemm_tiled2", "k_gemm_t64"), "k_gemm_skinny": ("k_gemm_skinny",)}


class Run:
    """one engine + B streams + their PCM in HBM, stepped through the C ABI"""

    def __init__(self, capi, synth, engW, layers, dtype, B, R, device, stream_ids, chunks_per_step=1, pipeline=4, audio_s=60.0,
                 speech=True, log_streams=1):
        self.capi, self.synth = capi, synth
        self.B, self.R, self.T = B, R, 1 + R
        self.n_step = synth.shift_samples(R) * chunks_per_step
        self.eng = capi.Engine(engW, n_layers=layers, dtype=dtype, max_streams=B, device=device)
        for kv in ENGINE_OPTIONS:                  # --engine-option key=value (A/B runs: tests/micro/ab_b64.sh)
            k, v = kv.split("=", 1)
            self.eng.set_option(k, int(v))
        self.eng.set_option("pipeline", pipeline)
        self.streams = [self.eng.stream(R) for _ in range(B)]
        self.n_avail = max(2, int(audio_s * synth.SAMPLE_RATE) // self.n_step)       # steps of audio per stream before it wraps
        n_total = self.n_avail * self.n_step
        gen = (lambda sid, secs: synth.make_speech_pcm(sid, secs)[0]) if speech else synth.make_pcm
        self.pcm_host = [gen(sid, n_total / synth.SAMPLE_RATE + 0.01)[:n_total] for sid in stream_ids]
        self.pcm_dev = [self.eng.upload(p) for p in self.pcm_host]
        self.L = capi.lib()
        self.handles = (C.c_void_p * B)(*[s.h for s in self.streams])
        self.tok_cap = 16 * self.T * chunks_per_step
        self.tok_bufs = [np.zeros(self.tok_cap, np.int32) for _ in range(B)]
        self.tptrs = (C.c_void_p * B)(*[b.ctypes.data for b in self.tok_bufs])
        self.caps = (C.c_int32 * B)(*([self.tok_cap] * B))
        self.ntok = (C.c_int32 * B)()
        self.ns = (C.c_int32 * B)(*([self.n_step] * B))
        self.dev_ptrs = [(C.c_void_p * B)(*[self.pcm_dev[s] + 2 * k * self.n_step for s in range(B)]) for k in range(self.n_avail)]
        self.host_ptrs = [(C.c_void_p * B)(*[self.pcm_host[s].ctypes.data + 2 * k * self.n_step for s in range(B)]) for k in range(self.n_avail)]
        self.k = 0                       # steps pushed so far (audio position = k mod n_avail)
        self.tokens = 0
        self.n_log = min(log_streams, B)
        self.tok_log = [[] for _ in range(self.n_log)]      # token ids of the first streams, in order (token_agreement)
        self.audio_per_step = B * self.n_step / synth.SAMPLE_RATE
        self.local_regions = []

    def step(self, host=False):
        i = self.k % self.n_avail
        ptrs = self.host_ptrs[i] if host else self.dev_ptrs[i]
        rc = self.L.nasr_engine_step(self.eng.h, self.handles, self.B, ptrs, self.ns, self.tptrs, self.caps, self.ntok,
                                     0 if host else self.capi.FLAG_PCM_DEVICE)
        if rc < 0:
            raise RuntimeError(self.L.nasr_last_error().decode())
        self.k += 1
        self.tokens += sum(self.ntok[b] for b in range(self.B))
        for b in range(self.n_log):
            if self.ntok[b]:
                self.tok_log[b] += self.tok_bufs[b][:self.ntok[b]].tolist()

    def drain(self):
        out = self.eng.collect(self.streams)
        self.tokens += sum(len(t) for t in out)
        for b in range(self.n_log):
            self.tok_log[b] += out[b]

    def close(self):
        for s in self.streams:
            s.destroy()
        self.eng.close()


DUMP_STREAMS = 64       # streams whose encoder output --dump-outputs writes (a fixed, seeded sample of larger batches)


def dump_outputs(d: Path, run, capi):
    """--dump-outputs: what the last timed step handed its caller, as float arrays -- the token ids each stream's call returned
    (tokens.npy, B x max count, -1 past a stream's count; token_counts.npy) and the encoder output of the chunk that step pushed
    (encoder_out.npy, streams x frames x 1024, float32; encoder_out_streams.npy: which streams, all of them up to DUMP_STREAMS).
    Called after the timed region; the encoder-out tap completes the steps still in flight."""
    d.mkdir(parents=True, exist_ok=True)
    counts = np.array([run.ntok[b] for b in range(run.B)], np.float64)
    toks = np.full((run.B, max(1, int(counts.max()))), -1.0)
    for b in range(run.B):
        toks[b, :run.ntok[b]] = run.tok_bufs[b][:run.ntok[b]]
    frames = run.n_step // 1280                                    # encoder frames (80 ms) per push
    n_pick = max(1, min(run.B, DUMP_STREAMS, (48 << 20) // (frames * 1024 * 4)))      # the whole dump stays far below 64 MB
    pick = np.arange(run.B) if n_pick == run.B else np.sort(np.random.default_rng(0).choice(run.B, n_pick, replace=False))
    enc = np.stack([run.streams[b].tap(capi.TAP_ENCODER_OUT).reshape(-1, 1024) for b in pick]).astype(np.float32)
    np.save(d / "tokens.npy", toks)
    np.save(d / "token_counts.npy", counts)
    np.save(d / "encoder_out.npy", enc)
    np.save(d / "encoder_out_streams.npy", pick.astype(np.float64))


PRIME = 8      # untimed steps after a region's opening barrier: refill the (at most 5-deep) step pipeline, replay every graph once


def timed_regions(run, steps, barrier, max_over_ranks, host=False, repeats=REPEATS, prime=PRIME):
    """`repeats` regions of exactly `steps` steps -> list of elapsed seconds (max over ranks).  Each region: barrier + device
    synchronise, `prime` untimed steps, t0, `steps` timed calls, t1, barrier + device synchronise.  prime = 0 is the literal
    idle-to-idle bracket (t1 is then taken after the closing synchronise)."""
    out = []
    for _ in range(repeats):
        barrier()
        for _ in range(prime):
            run.step(host)
        t0 = time.perf_counter()
        for _ in range(steps):
            run.step(host)
        t1 = time.perf_counter()
        barrier()
        if not prime:
            t1 = time.perf_counter()
        if hasattr(run, "local_regions"):
            run.local_regions.append(t1 - t0)       # this rank's own clock (per_rank in the line); `out` holds the max over ranks
        out.append(max_over_ranks(t1 - t0))
    return out


def agreement_entry(ob, log, ref_tokens, ref_frames, got_tokens, got_frames, n_frames):
    """engine tokens vs the F32 oracle's over the frames both have decoded, compact: token-for-token equality, aligned ratio,
    the tokens that came out at another frame and the largest oracle margin among those decisions"""
    import difflib
    g = [(t, f) for t, f in zip(got_tokens, got_frames) if f < n_frames]
    r = [(t, f) for t, f in zip(ref_tokens, ref_frames) if f < n_frames]
    gt, gf, rt, rf = [t for t, _ in g], [f for _, f in g], [t for t, _ in r], [f for _, f in r]
    rep = ob.token_timing_report(log, rt, rf, gt, gf)
    div = rep["first_divergence"]
    return dict(frames=n_frames, oracle_tokens=len(rt), engine_tokens=len(gt), tokens_equal=rep["tokens_equal"],
                aligned_ratio=round(difflib.SequenceMatcher(None, rt, gt, autojunk=False).ratio(), 4),
                common_prefix=len(rt) if rep["tokens_equal"] else (div["index"] if div else len(rt)),
                timing_shifts=len(rep["shifts"]), max_shift_margin=round(max([x["margin"] for x in rep["shifts"]], default=0.0), 4),
                divergence_margin=None if rep["tokens_equal"] or not div else round(div["margin"], 4))


def profile_pass(run, n_steps, label, pmc_tag, restore_pipeline, bound=None):
    """Roofline of the dominant kernel, the kernel ALONE on the chip: a region of synchronous graph-replayed steps gives the
    step time of the un-overlapped launch chain, a per-kernel-class HIP-event pass (eager launches, events around every
    launch on the engine's stream) gives each kernel's share of it.  (In the pipelined timed region two or three launch
    chains share the chip and a kernel's own duration is longer while the chip does more: `step_roofline` in the line is the
    figure for that regime.)  -> (roofline, kernels, synchronous step seconds)"""
    eng = run.eng
    eng.set_option("pipeline", 0)
    for _ in range(3):
        run.step()                                   # builds the synchronous step graph
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_steps):
        run.step()
    eng.synchronize()
    step_s = (time.perf_counter() - t0) / n_steps
    sync_steps = True
    eng.profile(True)
    for _ in range(n_steps):
        run.step()
    kernels = eng.profile_read()
    eng.profile(False)
    eng.set_option("pipeline", restore_pipeline)
    dom = max((k for k in kernels if "gemm" in k["name"]), key=lambda k: k["total_ms"], default=None)
    if not dom or dom["total_ms"] <= 0:
        return None, kernels, step_s
    # Events bracket every launch of the (eager) profile pass, so each bracket also holds ~2 us of launch latency that a
    # graph replay does not pay.  The kernel's duration = its share of the bracketed time x the synchronous graph-replayed
    # step; this is what rocprofv3 reports for `bench.py --sync-steps` (profiles/).  The raw bracket average is kept beside it.
    ev_total = sum(k["total_ms"] for k in kernels if sync_steps or k["name"] != "k_dec_iter")
    share = dom["total_ms"] / ev_total
    per_step = dom["launches"] / n_steps
    avg_s = share * step_s / per_step
    avg_ev_us = 1e3 * dom["total_ms"] / dom["launches"]
    flops, nbytes = dom["flops"] / dom["launches"], dom["bytes"] / dom["launches"]
    tf, gbs = flops / avg_s / 1e12, nbytes / avg_s / 1e9
    # batch 1 / R = 0 streams every weight once with M = 1 (HBM-bound); 64 streams x R = 13 has M = 896 rows
    # per GEMM (MFMA-bound).  In between the larger of the two lower bounds decides.
    mfma_bound = bound == "mfma" if bound else flops / (MFMA_PEAK_TFLOPS * 1e12) > nbytes / (HBM_PEAK_GBS * 1e9)
    traffic = pmc_traffic(_SYMBOL.get(dom["name"], (dom["name"],)), pmc_tag)
    common = dict(kernel=dom["name"], avg_launch_us=round(avg_s * 1e6, 3), avg_launch_us_event_brackets=round(avg_ev_us, 3),
                  launches_per_step=per_step, share_of_step=round(share, 4), alg_bytes_per_launch=round(nbytes),
                  alg_flops_per_launch=round(flops), traffic=traffic, workload=label,
                  regime="synchronous", step_ms=round(step_s * 1e3, 4),
                  regime_note="kernel alone on the chip: synchronous graph-replayed steps (one launch chain; launches_per_step x avg_launch_us fits inside "
                              "step_ms, NOT inside the pipelined ms_per_step -- that regime is the `timed_regime` block)")
    if mfma_bound:
        roof = dict(bound="mfma", achieved=round(tf, 2), peak=MFMA_PEAK_TFLOPS, unit="TFLOP/s", frac=round(tf / MFMA_PEAK_TFLOPS, 4),
                    peak_measured=MFMA_MEASURED_TFLOPS, frac_of_measured=round(tf / MFMA_MEASURED_TFLOPS, 4),
                    hbm_frac=round(gbs / HBM_PEAK_GBS, 4), **common)
    else:
        roof = dict(bound="hbm", achieved=round(gbs, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(gbs / HBM_PEAK_GBS, 4),
                    peak_measured=HBM_MEASURED_GBS, frac_of_measured=round(gbs / HBM_MEASURED_GBS, 4),
                    mfma_frac=round(tf / MFMA_PEAK_TFLOPS, 6), **common)
    return roof, kernels, step_s


def step_roofline(layers, B, R, step_s, weight_bytes_per_param=2.0):
    """Whole-step roofline fractions: algorithmic FLOPs of a step (2 x MACs of the conformer GEMMs, attention,
    subsampling; decode excluded) and algorithmic bytes (every encoder weight once per step in the GGUF flavour's size + K/V
    window and conv cache per stream) over the measured step time, against the dense bf16 MFMA and the HBM peak."""
    T, KV = 1 + R, 70 + 1 + R
    mac_frame = layers * (24117248 + 3 * 1024 * KV + 9216)
    sub_chunk = {0: 29.4e6, 1: 40e6, 6: 95e6, 13: 168e6}[R]
    flops = 2.0 * B * (T * mac_frame + sub_chunk)
    wbytes = layers * 24117248 * weight_bytes_per_param + 13.4e6 * 4
    state = B * layers * (2 * 70 * 1024 * 2 + 2 * T * 1024 * 2 + 2 * 8 * 1024 * 4)
    nbytes = wbytes + state
    return dict(flops_per_step=round(flops), bytes_per_step=round(nbytes), tflops=round(flops / step_s / 1e12, 1),
                gbs=round(nbytes / step_s / 1e9, 1), mfma_frac=round(flops / step_s / 1e12 / MFMA_PEAK_TFLOPS, 4),
                hbm_frac=round(nbytes / step_s / 1e9 / HBM_PEAK_GBS, 4))


def summarize(regions, steps, audio_per_step, world):
    med = statistics.median(regions)
    return dict(value=round(world * audio_per_step * steps / med, 2), ms_per_step=round(1e3 * med / steps, 4),
                runs_ms_per_step=[round(1e3 * r / steps, 4) for r in regions])


def reference_cli_baseline(pcm, R):
    """BASELINE.md §3 hook: when the user supplies the reference's own CLI built against their ggml checkout
    ($NEMOTRON_REF_BIN, e.g. /path/to/nemotron-asr.cpp built with `make GGML_DIR=$GGML_DIR`) and a real checkpoint
    ($NEMOTRON_GGUF), time `<bin> <gguf> <pcm> 80 <R> --cpu` on the headline stream's audio and report its own
    'Real-time factor' line (src/transcribe_stream.cpp:263-267) inverted to RTFx.  Neither exists on the pool's boxes."""
    exe, gguf = os.environ.get("NEMOTRON_REF_BIN"), os.environ.get("NEMOTRON_GGUF")
    if not exe or not gguf or not Path(exe).exists() or not Path(gguf).exists():
        return None
    import re
    import tempfile
    with tempfile.NamedTemporaryFile(suffix=".pcm") as f:
        pcm.tofile(f.name)
        r = subprocess.run([exe, gguf, f.name, "80", str(R), "--cpu"], capture_output=True, text=True, timeout=3600)
    m = re.search(r"Real-time factor[^0-9]*([0-9.]+)", r.stderr + r.stdout)
    if r.returncode != 0 or not m or float(m.group(1)) <= 0:
        return dict(error=(r.stderr or r.stdout)[-300:])
    return dict(value=round(1.0 / float(m.group(1)), 3), unit="audio-s/s", kind="reference", cores="ggml default thread count",
                sample=f"{pcm.size / 16000:.1f} s of the headline stream through {exe} --cpu (real checkpoint {gguf}: other weights than the GPU run)")


def host_info():
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = os.cpu_count() or 1
    return dict(nproc=os.cpu_count(), affinity=aff, cpu_model=model)


def cpu_baseline_sample(ob, om, synth, p, R, n_step, cpu_seconds, passes=3):
    """The oracle (the CPU restatement of the reference's path; stands in for src/transcribe_stream.cpp:260-267's own RTF line, ggml
    being absent) on `passes` consecutive stretches of stream 0, each timed on its own: `value` is the MEDIAN pass, `runs` all of
    them, `best` the fastest.  Threads are pinned (OMP_PROC_BIND=close, OMP_PLACES=cores: set in main() before any OpenMP runtime
    loads) and the host is named in the entry -- round 4's figure moved 2 x between boxes with neither stated.
    -> (entry, oracle stream, its tokens so far, steps processed after the two warm-up pushes)"""
    ost = ob.OracleStream(om, R)
    ost.enable_decision_log()
    n_total = max(2 * passes, min(int(cpu_seconds * synth.SAMPLE_RATE / n_step), p.size // n_step - 2))
    n_pass = max(1, n_total // passes)
    ref_tokens = ost.process(p[:2 * n_step])            # warm-up: fills the first chunk
    c0 = ost.total_chunks
    times, k = [], 2
    for _ in range(passes):
        tc = time.perf_counter()
        for kk in range(k, k + n_pass):
            ref_tokens += ost.process(p[kk * n_step:(kk + 1) * n_step])
        times.append(time.perf_counter() - tc)
        k += n_pass
    audio_pass = n_pass * n_step / synth.SAMPLE_RATE
    vals = sorted(audio_pass / t for t in times)
    med = statistics.median(vals)
    entry = dict(value=round(med, 3), unit="audio-s/s", cores=ob.lib().orc_num_threads(), kind="port",
                 runs=[round(audio_pass / t, 3) for t in times], best=round(vals[-1], 3), spread=round((vals[-1] - vals[0]) / med, 3),
                 sample=f"{passes} x {audio_pass:.1f} s of stream 0 ({ost.total_chunks - c0} chunks, {sum(times):.1f} s of CPU work), oracle/nasr_oracle.c f32 + OpenMP",
                 omp=dict(proc_bind=os.environ.get("OMP_PROC_BIND"), places=os.environ.get("OMP_PLACES"), wait_policy=os.environ.get("OMP_WAIT_POLICY")),
                 host=host_info())
    return entry, ost, ref_tokens, passes * n_pass


def main():
    args = parse()
    audio_regions = REPEATS if args.regions is None else args.regions      # the PCM budget below: the same in plain and full runs
    if args.regions is None:
        args.regions = REPEATS if args.full else 1
    ENGINE_OPTIONS[:] = args.engine_option
    # the CPU baseline's threads: one per core, neighbours close (before torch / the oracle load an OpenMP runtime, which reads these once)
    os.environ.setdefault("OMP_PROC_BIND", "close")
    os.environ.setdefault("OMP_PLACES", "cores")
    # the CPU baseline's team is one thread per CPU the box gives the job, so its threads may spin between the oracle's many short parallel regions
    # (round 5 ran it "passive", which slows exactly that and moved the baseline in the GPU's favour: advisor, round 5; oracle/binding.py's own
    # default stays passive for the test suite, where teams can be oversubscribed); the entry reports what was in force
    os.environ.setdefault("OMP_WAIT_POLICY", "active")
    if args.gpus < 1:
        sys.exit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))                     # nothing above touches the GPU
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus} "
                 f"(or drop the torchrun environment and let --gpus start the ranks)")
    dist = None
    torch = None
    if world > 1 or os.environ.get("NASR_BENCH_FORCE_DIST"):      # the knob exercises the RCCL plumbing on a 1-GPU box
        import torch
        import torch.distributed as dist
        if "RANK" not in os.environ:                               # the knob without a torchrun environment: a world of one
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                free_port = sk.getsockname()[1]
            os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port))
        if args.stub_engine or args.share_device >= 0:
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    ge.load_package()
    from nemotron_asr_amd import capi, sharding, synth

    B, R = args.batch, args.right_context
    T = 1 + R
    red_dev = "cpu" if args.stub_engine or args.share_device >= 0 else "cuda"
    if args.share_device >= 0:
        local_rank = args.share_device          # every rank's engine on the one device there is

    def max_over_ranks(x):
        return sharding.max_over_ranks(dist, x, device=red_dev)

    if args.stub_engine:
        # ---- launch-path test: same control flow (ranks, barriers, max over ranks, one JSON line), no engine ----------
        stub = _StubEngine(B)

        class _R:
            audio_per_step = B * synth.shift_samples(R) / synth.SAMPLE_RATE

            def step(self, host=False):
                stub.step()
        run = _R()

        def barrier():
            sharding.barrier(dist, None)
        for _ in range(args.warmup):
            run.step()
        regions = timed_regions(run, args.steps, barrier, max_over_ranks, repeats=args.regions, prime=0)
        if rank == 0:
            s = summarize(regions, args.steps, run.audio_per_step, world)
            print(json.dumps({"metric": "RTFx (audio-sec/sec), nemotron-0.6B streaming forward path", "value": s["value"], "unit": "audio-s/s",
                              "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": s["ms_per_step"],
                              "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "none", "data": "none",
                              "stub": True, "config": {"workload": "STUB ENGINE (sleeps): launch-path test, not a measurement",
                                                       "ranks_seen": world, "stream_ids_rank0": sharding.stream_ids(rank, world, B)}}), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    t0 = time.time()
    speech = args.checkpoint == "speech" and args.layers == 24          # the fit belongs to the 24-layer encoder
    node_rank0 = int(os.environ.get("LOCAL_RANK", "0")) == 0
    if node_rank0:
        remove_stale_shm()

    def shared(tag, make):
        """N > 1: the node's first rank builds the tensors once and parks them in /dev/shm, the others map them read-only
        (round 3: every rank generated 2.4 GB of f32 weights + Q8_0 + dequantised copies of its own: ~5.5 GB x N on the host)."""
        if dist is None or world == 1:
            return make()
        d = Path("/dev/shm") / f"nasr_bench_{os.environ.get('MASTER_PORT', '0')}_{tag}"
        if node_rank0:
            SHM_DIRS.append(d)                  # the atexit hook removes it if anything below fails
            store_weights(d, make())
        dist.barrier()
        out = load_weights(d)
        dist.barrier()
        if node_rank0:                          # every rank has mapped the files: unlink them now (the mappings stay valid), so that a rank
            import shutil                       # that crashes or is killed later leaves nothing behind in RAM
            shutil.rmtree(d, ignore_errors=True)
        return out

    W = shared(f"f32_{args.layers}_{int(speech)}", lambda: synth.make_weights(n_layers=args.layers, margins="speech" if speech else "random"))
    t_weights = time.time() - t0
    dtype = capi.DTYPE_BF16 if args.dtype == "bf16" else capi.DTYPE_F32
    engW, Wcpu = W, W
    if args.weights != "f32":
        if world == 1:
            engW, Wcpu = synth.quantize_weights(W, args.weights)     # engine gets the packed blocks, the CPU baseline their values
        else:
            engW = shared(f"{args.weights}_{args.layers}_{int(speech)}", lambda: synth.quantize_weights(W, args.weights)[0])
    depth = 0 if args.sync_steps else args.pipeline_depth
    prime = PRIME if depth else 0
    prof_steps = 0 if args.no_profile_pass else min(args.steps, 50)
    # PCM per stream as a --full run with the same arguments budgets it (the stream's audio depends on its length): a plain run
    # feeds the headline the same audio
    need_s = (args.warmup + (audio_regions + 3) * (args.steps + prime) * 2 + prof_steps + 4) * synth.shift_samples(R) * args.chunks_per_step / synth.SAMPLE_RATE
    audio_s = min(max(need_s, args.cpu_seconds + 2.0), 120.0)
    if not args.full:
        prof_steps = 0
    run_ids = [args.stream_offset + i for i in sharding.stream_ids(rank, world, B)]
    run = Run(capi, synth, engW, args.layers, dtype, B, R, local_rank, run_ids, args.chunks_per_step,
              pipeline=depth, audio_s=audio_s, speech=speech)
    del engW
    details = {}

    def barrier_for(r):
        def barrier():
            sharding.barrier(dist, r.eng.synchronize)
            if dist is not None and red_dev == "cuda":
                torch.cuda.synchronize()        # torch's own stream (RCCL barrier); the engine's stream is synchronised above
        return barrier

    barrier = barrier_for(run)
    pcm0, n_step0 = run.pcm_host[0], run.n_step      # stream 0's audio (the CPU baseline's sample at N > 1, after `run` is closed)
    for _ in range(args.warmup):
        run.step()
    run.drain()                                # pipelined steps: the last warm-up step's tokens are not the timed region's
    run.tokens = 0
    regions = timed_regions(run, args.steps, barrier, max_over_ranks, repeats=args.regions, prime=prime)
    if args.dump_outputs and rank == 0:
        dump_outputs(Path(args.dump_outputs), run, capi)
    run.drain()
    tokens_timed, chunks_timed = run.tokens, run.streams[0].progress().chunks
    per_rank = None
    if dist is not None:                       # what every rank did in the same timed regions (N > 1: tokens must match a single-process run of the same streams)
        try:
            aff = sorted(os.sched_getaffinity(0))
        except (AttributeError, OSError):
            aff = []
        mine = dict(rank=rank, device=local_rank, stream_ids=dict(first=run_ids[0], stride=world, count=len(run_ids)), tokens_emitted=tokens_timed,
                    lanes=run.eng.counter("lanes"), cpu_affinity=((",".join(map(str, aff)) if len(aff) <= 8 else f"{len(aff)} CPUs in {aff[0]}..{aff[-1]}") if aff else None),
                    ms_per_step=round(1e3 * statistics.median(run.local_regions[-args.regions:]) / args.steps, 4) if getattr(run, "local_regions", None) else None)
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
        per_rank = gathered
    head = summarize(regions, args.steps, run.audio_per_step, world)
    cold = head if args.full else None         # synchronous steps: a region is idle-to-idle already
    if prime and args.full:
        cold = summarize(timed_regions(run, args.steps, barrier, max_over_ranks, repeats=min(3, args.regions), prime=0), args.steps, run.audio_per_step, world)
        run.drain()
    host_pcm = None
    if args.full and not args.no_host_pcm:
        host_regions = timed_regions(run, args.steps, barrier, max_over_ranks, host=True, repeats=min(3, args.regions), prime=prime)
        run.drain()
        host_pcm = summarize(host_regions, args.steps, run.audio_per_step, world)
    step_s = statistics.median(regions) / args.steps

    # the grouped pipeline (option pipeline = 8: 8 steps in flight, four steps per launch) on the same run, for the record
    grouped_ms = None
    if args.full and depth == 4 and B * T * args.chunks_per_step <= 2 and args.dtype == "bf16" and args.layers % 8 == 0 and not args.no_grouped:
        run.eng.set_option("pipeline", 8)
        for _ in range(12):
            run.step()
        gr = timed_regions(run, args.steps, barrier, max_over_ranks, repeats=min(3, args.regions), prime=12)
        run.drain()
        run.eng.set_option("pipeline", depth)
        grouped_ms = summarize(gr, args.steps, run.audio_per_step, world)["ms_per_step"]

    roofline, kernels = None, []
    label = f"batch={B} R={R} {args.dtype}" + (f" from {args.weights}" if args.weights != "f32" else "")
    sync_step_s = None
    if prof_steps:                               # on EVERY rank: a rank that skipped it would sit in the next barrier while rank 0 profiles
        roofline, kernels, sync_step_s = profile_pass(run, prof_steps, label, f"b{B}_R{R}", depth)
        run.drain()
    steps_pushed = run.k

    # ---- the same stream fed buffered audio (file transcription): 256 chunks per push share one launch sequence ----
    buffered = None
    tok_log_keep, frames_keep = list(run.tok_log[0]), (run.streams[0].token_frames() if rank == 0 else [])
    if args.full and rank == 0 and world == 1 and (B, args.chunks_per_step) == (1, 1) and not args.no_buffered:
        eng, L = run.eng, run.L
        G, n_push = 256, 8
        nb = synth.shift_samples(R) * G
        pb = synth.make_pcm(1000, (n_push + 1) * nb / synth.SAMPLE_RATE + 0.01)[:(n_push + 1) * nb]
        db = eng.upload(pb)
        eng2_stream = run.streams[0]
        eng2_stream.reset()                      # the timed region is over: reuse its slot
        hb = (C.c_void_p * 1)(eng2_stream.h)
        tb = np.zeros(16 * T * G, np.int32)
        tpb = (C.c_void_p * 1)(tb.ctypes.data)
        cb = (C.c_int32 * 1)(tb.size)
        nbb = (C.c_int32 * 1)(nb)
        ntb = (C.c_int32 * 1)()
        eng.set_option("pipeline", 0)            # pushes of 20 s of audio: one synchronous launch sequence each

        def push(k):
            ptr = (C.c_void_p * 1)(db + 2 * k * nb)
            if L.nasr_engine_step(eng.h, hb, 1, ptr, nbb, tpb, cb, ntb, capi.FLAG_PCM_DEVICE) < 0:
                raise RuntimeError(L.nasr_last_error().decode())
        push(0)                                  # the first push builds the graph
        eng.synchronize()
        tq = time.perf_counter()
        for k in range(1, n_push + 1):
            push(k)
        eng.synchronize()
        tsum = time.perf_counter() - tq
        buffered = dict(chunks_per_push=G, ms_per_push=round(1e3 * tsum / n_push, 3), value=round(n_push * nb / synth.SAMPLE_RATE / tsum, 1))
        # the same pushes with pipelined steps (a file transcription does not need its tokens in the same call): the pieces of push
        # k + 1 .. k + 3 run beside push k's.  Timed like the headline: priming pushes, then call-to-call time of the timed ones.
        eng.synchronize()
        eng2_stream.reset()
        eng.set_option("pipeline", args.pipeline_depth if args.pipeline_depth in (2, 3, 4) else 4)
        n_prime, n_timed = 8, 16
        for k in range(n_prime):
            push(k % (n_push + 1))
        tq = time.perf_counter()
        for k in range(n_timed):
            push((n_prime + k) % (n_push + 1))
        tsum = time.perf_counter() - tq
        eng.synchronize()
        buffered.update(pipelined_ms_per_push=round(1e3 * tsum / n_timed, 3), pipelined_value=round(n_timed * nb / synth.SAMPLE_RATE / tsum, 1))
        eng.set_option("pipeline", 0)
        details["buffered_audio_note"] = ("same engine, same stream semantics (80 ms lookahead, chunk-by-chunk caches), the 256 chunks of a push go "
                                          "through every layer as one launch sequence; not the headline value")

    # ---- diarization side-car beside the ASR engine (configs[4]) ---------------------------------------------------------
    def diarization_entry(r, n_ov):
        # The ASR engine and the side-car share the runtime's four hardware queues.  Round 6 (segment-tile TitaNet-L: an embedding call 3.4 -> 1.25 ms): ONE
        # side-car queue, lent by the ASR engine (nasr_engine_lend_stream), one host thread calling VAD then embeddings, and the ASR engine keeps THREE lanes
        # (4.50 ms per step; two side-car queues + two ASR lanes, the round-2 arrangement: 4.91; profiles/r6_titanet_segment_tiles.md, last table).  NASR_DIAR_SPLIT=1 / NASR_DIAR_ASR_LANES=n
        # select the other arrangements.
        split = os.environ.get("NASR_DIAR_SPLIT", "0") != "0" and not args.sync_steps
        side_depth = 0 if args.sync_steps else min(args.pipeline_depth, int(os.environ.get("NASR_DIAR_ASR_LANES", "2" if split else "3")))
        r.drain()
        dW = synth.make_diar_weights()
        dvad = capi.Diar(dW, dtype=capi.DTYPE_BF16 | (0 if os.environ.get("NASR_DIAR_VAD_F32") else capi.DIAR_VAD_F16), max_segments=max(8, 2 * r.B), device=local_rank)
        demb = capi.Diar(dW, dtype=capi.DTYPE_BF16, max_segments=max(8, 2 * r.B), device=local_rank) if split else dvad
        if side_depth:
            dvad.set_stream(r.eng.lend_stream())       # a hardware queue the ASR engine no longer uses
            if split:
                demb.set_stream(r.eng.lend_stream())
        r.eng.set_option("pipeline", side_depth)
        hist = 10080 - 160                                   # samples of history a new 10 ms hop needs
        # the side-car reads the SAME s16 PCM the ASR streams were fed, already resident in HBM
        vad_ptrs = [r.pcm_dev[b] for b in range(r.B)]
        vad_n = [hist + r.n_step] * r.B
        n_seg = max(1, int(round(r.B * (r.n_step / synth.SAMPLE_RATE) / 0.75)))                          # sub-segment shift 0.75 s
        seg_ptrs = [r.pcm_dev[i % r.B] + 2 * 12000 * (i // r.B) for i in range(n_seg)]
        dvad.vad_device_s16(vad_ptrs, vad_n); demb.embed_device_s16(seg_ptrs)
        reps = 10
        r.eng.synchronize()
        tq = time.perf_counter()
        for _ in range(reps):
            pv = dvad.vad_device_s16(vad_ptrs, vad_n)
        t_vad = (time.perf_counter() - tq) / reps
        tq = time.perf_counter()
        for _ in range(reps):
            demb.embed_device_s16(seg_ptrs)
        t_spk = (time.perf_counter() - tq) / reps
        # the same work overlapped: the side-car's calls come from their own host threads while the ASR step of the same audio
        # runs on the engine's streams (ctypes releases the GIL during all of them)
        import threading
        n_side = 2 if split else 1
        gate_go, gate_done = threading.Barrier(1 + n_side), threading.Barrier(1 + n_side)

        def side_car(which):
            for _ in range(n_ov):
                gate_go.wait()
                if which in (0, 2):
                    dvad.vad_device_s16(vad_ptrs, vad_n)
                if which in (1, 2):
                    demb.embed_device_s16(seg_ptrs)
                gate_done.wait()

        ovs = []
        for _ in range(REPEATS):
            ths = [threading.Thread(target=side_car, args=(w,)) for w in ((0, 1) if split else (2,))]
            for th in ths:
                th.start()
            r.eng.synchronize()
            tq = time.perf_counter()
            for _ in range(n_ov):
                gate_go.wait()
                r.step()
                gate_done.wait()
            r.eng.synchronize()
            ovs.append((time.perf_counter() - tq) / n_ov)
            for th in ths:
                th.join()
        r.drain()
        r.eng.set_option("pipeline", depth)
        t_ov = statistics.median(ovs)
        d = dict(value=round(r.audio_per_step / t_ov, 1), ms_per_step=round(1e3 * t_ov, 3), vad_ms=round(1e3 * t_vad, 3), embed_ms=round(1e3 * t_spk, 3))
        # roofline of the side-car's dominant launch sequence, measured live: HIP events on the side-car's own stream around the kernels of an embedding
        # call run alone (nasr_diar_last_gpu_ms).  Algorithmic flops: TitaNet-L = 2 x 160 frames x 16 646 144 MAC of pointwise / attention
        # GEMMs per 1.5 s sub-segment (src/diarize_spk.cpp:28-34: 80->1024, 9 + 3 x 1024->1024, 1024->3072, 3072->128->3072), MarbleNet = 11.4 MFLOP per 0.63 s
        # window (src/diarize_vad.cpp:25-32: 89 k MAC per frame x 64 frames); the depthwise taps (< 1 %) and the small linears are not counted.
        spk_flops, vad_flops = n_seg * 2.0 * 160 * 16646144, float(sum(x.size for x in pv)) * 11.4e6
        demb.embed_device_s16(seg_ptrs)
        emb_gpu_ms = demb.last_gpu_ms("embed")
        dvad.vad_device_s16(vad_ptrs, vad_n)
        vad_gpu_ms = dvad.last_gpu_ms("vad")
        asr = step_roofline(args.layers, r.B, r.R, t_ov, 1.0625 if args.weights == "q8_0" else 2.0)
        if emb_gpu_ms > 0:
            ach = spk_flops / (emb_gpu_ms * 1e-3) / 1e12
            # fabric traffic of one embedding call from the PMC passes (tests/prof_diar_pmc.sh: FETCH_SIZE x 2 + WRITE_SIZE, summed over the call's 40 launches); profiled at 96 sub-segments
            traffic = None
            try:
                pj = json.loads((ROOT / "profiles" / "r6_pmc_traffic_diar.json").read_text())["embed_call_96_segments"]
                if n_seg == 96 and not pj["kernels_without_counters"]:
                    traffic = int(pj["hbm_bytes_corrected"])
            except (OSError, KeyError, ValueError):
                pass
            d["roofline"] = dict(bound="mfma", achieved=round(ach, 1), peak=MFMA_PEAK_TFLOPS, unit="TFLOP/s", frac=round(ach / MFMA_PEAK_TFLOPS, 4), traffic=traffic,
                                 kernel="TitaNet-L launch sequence (one nasr_diar_embed call, alone)",
                                 avg_launch_us=round(1e3 * emb_gpu_ms, 1), launches_per_step=1)
        d["step_mfma_frac"] = round((asr["flops_per_step"] + spk_flops + vad_flops) / t_ov / 1e12 / MFMA_PEAK_TFLOPS, 4)
        d["embed_gpu_ms"], d["vad_gpu_ms"] = round(emb_gpu_ms, 3), round(vad_gpu_ms, 3)
        details["diarize"] = dict(runs_ms_per_step=[round(1e3 * x, 3) for x in ovs], steps_per_region=n_ov, vad_windows_per_step=int(sum(x.size for x in pv)),
                                  embeddings_per_step=n_seg, asr_pipeline_depth=side_depth, split_streams=split,
                                  note="side-car (MarbleNet VAD on every 10 ms window + TitaNet-L embeddings of 1.5 s sub-segments at a 0.75 s shift, random-init "
                                       "weights) on the streams' own s16 PCM, device-resident, on HIP stream(s) lent by the ASR engine (split_streams: VAD and embeddings each "
                                       "on their own stream and host thread; otherwise one stream, one thread), beside the ASR step; vad_ms / embed_ms: each call run alone")
        dvad.close()
        if split:
            demb.close()
        return d

    diar = None
    if args.diarize and rank == 0:
        diar = diarization_entry(run, min(args.steps, 50))

    # ---- CPU baseline: the oracle (a port of the reference's algorithm), bounded sample; token agreement -------------
    cpu, agreement, cpu_ref, f32_entry, random_ckpt = None, None, None, None, None
    headline_is_default = (B, R, args.dtype, args.layers, args.chunks_per_step, args.weights) == (1, 0, "bf16", 24, 1, "f32")
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import binding as ob
        om = ob.OracleModel(Wcpu, args.layers)
        n_step = run.n_step
        p = run.pcm_host[0]
        cpu, ost, ref_tokens, n_cpu_steps = cpu_baseline_sample(ob, om, synth, p, R, n_step, args.cpu_seconds)
        # engine tokens of stream 0 (warm-up + timed + host-PCM + profile steps, one continuous stream) vs the F32 oracle on the
        # same audio, cut at the frames both have decoded
        ref_frames, ref_log = ost.token_frames(), ost.decision_log()
        # the first push completes no chunk, every later one exactly one; audio is contiguous until the stream's PCM wraps
        if args.chunks_per_step == 1:
            n_frames = (min(steps_pushed, run.n_avail, 2 + n_cpu_steps) - 1) * T
            agreement = agreement_entry(ob, ref_log, ref_tokens, ref_frames, tok_log_keep, frames_keep, n_frames)
            agreement["margins_ge_0p5"] = round(float((ref_log["margin"] >= 0.5).mean()), 4)
        # ---- the f32 engine: the configuration whose tokens AND emission frames equal the oracle's in every bit -----------
        if headline_is_default and not args.no_f32_engine:
            run.close()
            run = None
            frun = Run(capi, synth, W, args.layers, capi.DTYPE_F32, B, R, local_rank, sharding.stream_ids(rank, world, B), 1, pipeline=depth,
                       audio_s=audio_s, speech=speech)
            fsteps = min(args.steps, 100)
            for _ in range(max(args.warmup, 6)):
                frun.step()
            fr = timed_regions(frun, fsteps, barrier_for(frun), max_over_ranks, repeats=3, prime=prime)
            frun.drain()
            f32_entry = summarize(fr, fsteps, frun.audio_per_step, world)
            details["f32_engine_runs_ms_per_step"] = f32_entry.pop("runs_ms_per_step")
            frun.eng.set_option("pipeline", 0)
            for _ in range(3):
                frun.step()
            frun.eng.synchronize()
            tq = time.perf_counter()
            for _ in range(fsteps):
                frun.step()
            frun.eng.synchronize()
            f32_entry["synchronous_ms_per_step"] = round(1e3 * (time.perf_counter() - tq) / fsteps, 4)
            frun.drain()
            fa = agreement_entry(ob, ref_log, ref_tokens, ref_frames, frun.tok_log[0], frun.streams[0].token_frames(),
                                 (min(frun.k, frun.n_avail, 2 + n_cpu_steps) - 1) * T)
            f32_entry.update(tokens_equal_oracle=fa["tokens_equal"], frames_equal_oracle=fa["tokens_equal"] and fa["timing_shifts"] == 0,
                             oracle_tokens=fa["oracle_tokens"])
            frun.close()
            # ---- the same exact-parity configuration at configs[2]'s batch, on the near-tie (random) checkpoint: 64 streams x R = 13,
            # f32 GEMMs on the f32 MFMA (round 4).  Timing here; tokens of 8 streams against the oracle here, of all 64 in
            # tests/test_gpu_configs.py::test_f32_engine_64_streams_is_token_exact_on_the_near_tie_checkpoint
            del om
            Wr = synth.make_weights(n_layers=args.layers, margins="random")
            xR, xB, n_f = 13, 64, 12
            f64 = Run(capi, synth, Wr, args.layers, capi.DTYPE_F32, xB, xR, local_rank, list(range(xB)), 1, pipeline=depth, audio_s=20.0, speech=False, log_streams=8)
            for _ in range(4):
                f64.step()
            f64.drain()
            f6 = timed_regions(f64, n_f, barrier_for(f64), max_over_ranks, repeats=3, prime=min(prime, 4))
            f64.drain()
            e64 = summarize(f6, n_f, f64.audio_per_step, world)
            e64.pop("runs_ms_per_step")
            # the headline shape on the near-tie checkpoint too (round-3 advisor: `value` moved to the speech checkpoint in round 3; same
            # shapes and kernels, another token density): a stable key for cross-round comparisons
            rrun = Run(capi, synth, Wr, args.layers, dtype, B, R, local_rank, run_ids, 1, pipeline=depth, audio_s=20.0, speech=False)
            for _ in range(max(args.warmup, 6)):
                rrun.step()
            rrun.drain()
            rr = timed_regions(rrun, args.steps, barrier_for(rrun), max_over_ranks, repeats=3, prime=prime)
            rrun.drain()
            random_ckpt = summarize(rr, args.steps, rrun.audio_per_step, world)
            random_ckpt.pop("runs_ms_per_step")
            rrun.close()
            omr = ob.OracleModel(Wr, args.layers)
            n_cmp = 3                                   # pushes compared per stream (the first completes no chunk)
            eq, n_tok = True, 0
            for b in range(f64.n_log):
                ost = ob.OracleStream(omr, xR)
                rt = []
                for k in range(n_cmp):
                    rt += ost.process(f64.pcm_host[b][k * f64.n_step:(k + 1) * f64.n_step])
                rf = ost.token_frames()
                gt = [(t, f) for t, f in zip(f64.tok_log[b], f64.streams[b].token_frames()) if f < (n_cmp - 1) * (1 + xR)]
                eq = eq and gt == list(zip(rt, rf))
                n_tok += len(rt)
            e64.update(tokens_and_frames_equal_oracle=bool(eq), streams_checked=f64.n_log, oracle_tokens=n_tok, checkpoint="random (near-tie)")
            details["f32_engine_b64_R13"] = e64
            f32_entry["b64_R13_ms_per_step"] = e64["ms_per_step"]
            f32_entry["b64_R13_tokens_equal_oracle"] = bool(eq)
            f64.close()
            del omr, Wr
            om = None
        del om
        cpu_ref = reference_cli_baseline(p[:int(args.cpu_seconds * synth.SAMPLE_RATE)], R)

    # ---- the other configurations BASELINE.json names ------------------------------------------------------------------
    configs = {}
    if args.full and headline_is_default and not args.no_extra_configs:
        if run is not None:
            run.close()
            run = None
        xB, xR = 64, 13
        # one GPU: BASELINE configs[2], the engine fed Q8_0 tensors; N GPUs: configs[3] ("bf16, 512 streams sharded 8 x MI355X, 64 / GPU"): the
        # f32 tensors, rounded to bf16 at upload -- the entry is named after what it feeds
        xkey = "b64_R13_q8_0" if world == 1 else "b64_R13_bf16"
        q8deq = None
        if world == 1:
            q8W, q8deq = synth.quantize_weights(W, "q8_0")
        else:
            q8W = W
        xrun = Run(capi, synth, q8W, args.layers, capi.DTYPE_BF16, xB, xR, local_rank, sharding.stream_ids(rank, world, xB), 1,
                   pipeline=depth, audio_s=60.0, speech=speech, log_streams=3)
        del q8W
        xbar = barrier_for(xrun)
        for _ in range(8):
            xrun.step()
        xrun.drain()
        xrun.tokens = 0
        xr = timed_regions(xrun, args.extra_steps, xbar, max_over_ranks, prime=prime)
        xrun.drain()
        e = summarize(xr, args.extra_steps, xrun.audio_per_step, world)
        details[xkey] = dict(runs_ms_per_step=e.pop("runs_ms_per_step"), steps_per_region=args.extra_steps, regions=REPEATS, tokens_emitted=xrun.tokens,
                                       workload=f"nemotron-speech-streaming-0.6B ({args.layers} layers) bf16{' from Q8_0 tensors' if world == 1 else ''}, batch={xB} streams/GPU, 1.12 s "
                                                f"lookahead (R=13), {world}xMI355X [BASELINE.json configs[{2 if world == 1 else 3}]]")
        xh = timed_regions(xrun, args.extra_steps, xbar, max_over_ranks, host=True, repeats=3, prime=prime)
        xrun.drain()
        e["host_pcm_ms_per_step"] = summarize(xh, args.extra_steps, xrun.audio_per_step, world)["ms_per_step"]
        sr = step_roofline(args.layers, xB, xR, statistics.median(xr) / args.extra_steps, 34.0 / 32.0)
        e["step_mfma_frac"] = sr["mfma_frac"]
        details[xkey]["step_roofline"] = sr
        x_pushed = xrun.k
        x_logs = [list(t) for t in xrun.tok_log]
        x_frames = [xrun.streams[b].token_frames() for b in range(xrun.n_log)] if rank == 0 else []
        if prof_steps:                           # every rank (see above); rank 0 keeps the result
            xroof, xk, xs = profile_pass(xrun, 20, "batch=64 R=13 bf16 from q8_0", "b64_R13", depth, bound="mfma")
            e["synchronous_ms_per_step"] = round(1e3 * xs, 4)
            if xroof:
                e["roofline"] = {k: xroof[k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_us")}
                details[xkey]["roofline"] = xroof
            details[xkey]["kernels"] = [dict(name=k["name"], launches=k["launches"], ms=round(k["total_ms"], 3)) for k in xk]
            xrun.drain()
        if rank == 0 and world == 1 and not args.no_cpu_baseline:
            # token agreement of the first streams against the F32 oracle on the dequantised weights
            from oracle import binding as ob
            om = ob.OracleModel(q8deq, args.layers)
            n_cmp = min(x_pushed, xrun.n_avail, 27)                      # pushes compared: at most 30 s of audio per stream
            rows = []
            for b in range(xrun.n_log):
                ost = ob.OracleStream(om, xR)
                ost.enable_decision_log()
                rt = []
                for k in range(n_cmp):
                    rt += ost.process(xrun.pcm_host[b][k * xrun.n_step:(k + 1) * xrun.n_step])
                rows.append(agreement_entry(ob, ost.decision_log(), rt, ost.token_frames(), x_logs[b], x_frames[b], (n_cmp - 1) * (1 + xR)))
            del om
            e["token_agreement"] = dict(streams=len(rows), oracle_tokens=sum(r["oracle_tokens"] for r in rows), tokens_equal=all(r["tokens_equal"] for r in rows),
                                        aligned_ratio=round(sum(r["aligned_ratio"] * r["oracle_tokens"] for r in rows) / max(1, sum(r["oracle_tokens"] for r in rows)), 4),
                                        timing_shifts=sum(r["timing_shifts"] for r in rows), max_shift_margin=max(r["max_shift_margin"] for r in rows))
            details[xkey]["token_agreement_rows"] = rows
        del q8deq
        configs[xkey] = e
        if rank == 0 and world == 1:
            configs["b64_R13_diarize"] = diarization_entry(xrun, 40)
        xrun.close()
        if rank == 0 and world == 1 and not args.no_b512:
            # north_star's third batch size on ONE GPU: 512 streams x 1.12 s (M = 7 168 rows per GEMM: 7 tiles per CU), Q8_0 tensors; and 256 streams (3 584 rows:
            # the size VERDICT round 4 set a bar for -- four pieces, the 224 x 256 tiles from 32 of them).  The second entry never costs the line: an error in it is reported in its place.
            q8W, _ = synth.quantize_weights(W, "q8_0")
            for nb in (512, 256):
                bkey = f"b{nb}_R13_q8_0"
                try:
                    brun = Run(capi, synth, q8W, args.layers, capi.DTYPE_BF16, nb, xR, local_rank, list(range(nb)), 1, pipeline=depth, audio_s=12.0, speech=speech)
                    for _ in range(6):
                        brun.step()
                    brun.drain()
                    br = timed_regions(brun, 20, barrier_for(brun), max_over_ranks, repeats=3, prime=prime)
                    brun.drain()
                    b = summarize(br, 20, brun.audio_per_step, 1)
                    details[bkey] = dict(runs_ms_per_step=b.pop("runs_ms_per_step"), step_roofline=step_roofline(args.layers, nb, xR, statistics.median(br) / 20, 34.0 / 32.0))
                    b["step_mfma_frac"] = details[bkey]["step_roofline"]["mfma_frac"]
                    configs[bkey] = b
                    brun.close()
                except Exception as ex:          # noqa: BLE001 -- the 512-stream entry is part of the contract of this line, the 256-stream one is an extra
                    if nb == 512:
                        raise
                    configs[bkey] = dict(error=str(ex)[:300])
            del q8W

    if args.full and rank == 0 and world > 1 and not args.no_cpu_baseline:
        # N > 1: the same baseline, after the last timed region (the other ranks are already in the closing barrier), on this rank's share
        # of the host: threads = cores / world (set before the oracle library loads), so that a SCALE line is self-contained
        os.environ.setdefault("NASR_ORACLE_THREADS", str(max(1, min(16, host_info()["affinity"] // world))))
        from oracle import binding as ob
        om = ob.OracleModel(W, args.layers)
        cpu = cpu_baseline_sample(ob, om, synth, pcm0, R, n_step0, min(args.cpu_seconds, 30.0))[0]
        cpu["sample"] += f"; rank 0 of {world}, threads = cores / {world}"
        del om

    if rank == 0:
        workload = (f"nemotron-speech-streaming-0.6B ({args.layers} layers) {args.dtype}"
                    + (f" from {args.weights.upper()} tensors" if args.weights != "f32" else "") + f", batch={B} stream(s)/GPU, "
                    f"{80 * T} ms lookahead (R={R}), {world}xMI355X"
                    + (f", {args.chunks_per_step} chunks pushed per step" if args.chunks_per_step > 1 else "")
                    + (" [BASELINE.json configs[1]]" if headline_is_default else ""))
        roof_keys = ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_us", "launches_per_step", "frac_of_measured", "regime", "step_ms")
        sr = step_roofline(args.layers, B * args.chunks_per_step, R, step_s, {"f32": 2.0, "f16": 2.0, "q8_0": 34.0 / 32.0, "q4_0": 18.0 / 32.0}[args.weights])
        out = {
            "metric": "RTFx (audio-sec/sec), nemotron-0.6B streaming forward path",
            "value": head["value"],
            "unit": "audio-s/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": head["ms_per_step"],
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {"workload": workload, "streams_per_gpu": B, "right_context": R, "parallelism": f"stream-sharded x{world} ({sharding.PLACEMENT}: the server's --devices rule), no collectives",
                       **({"rehearsal": f"all {world} ranks on device {args.share_device}, gloo barrier (one-GPU box)"} if args.share_device >= 0 else {}),
                       "pcm": "device-resident", "checkpoint": "speech" if speech else "random", "pipeline": depth, "tokens_emitted": tokens_timed,
                       "bracket": (f"primed: {prime} untimed steps fill the pipeline, K timed calls, no drain inside the region (idle-to-idle: cold_ms_per_step; "
                                   f"one chunk at a time: synchronous_ms_per_step)") if prime else "idle-to-idle, synchronous steps"},
            "per_rank": per_rank,
            "configs": configs or None,
            "roofline": {k: roofline[k] for k in roof_keys if k in roofline} if roofline else None,
            "cpu_baseline": cpu,
            "f32_engine": f32_entry,
            "token_agreement": agreement,
            "cold_ms_per_step": cold["ms_per_step"] if cold else None,
            "random_checkpoint": random_ckpt,
            "synchronous_ms_per_step": round(1e3 * sync_step_s, 4) if sync_step_s else None,
            "host_pcm_ms_per_step": host_pcm["ms_per_step"] if host_pcm else None,
            "pipeline8_ms_per_step": grouped_ms,
            "step_roofline": {"hbm_frac": sr["hbm_frac"], "mfma_frac": sr["mfma_frac"], "gbs": sr["gbs"]},
            "timed_regime": timed_regime_block(f"b{B}_R{R}", depth, head["ms_per_step"], sr),
            "buffered_audio": buffered,
            "diarization": diar,
            "cpu_baseline_reference_cli": cpu_ref,
            "timing": f"median of {args.regions} region(s) of {args.steps} steps; region = barrier+sync, {prime} priming steps, K timed calls; max over ranks",
            "details": args.details if args.full else None,
        }
        out = {k: v for k, v in out.items() if v is not None or k == "vs_baseline" or (args.full and k in ("roofline", "cpu_baseline"))}
        if args.full:
            details.update(runs_ms_per_step=head["runs_ms_per_step"], cold_runs_ms_per_step=cold["runs_ms_per_step"],
                           host_pcm=host_pcm, roofline=roofline, step_roofline=sr, chunks=chunks_timed, setup_s={"weights": round(t_weights, 1)},
                           kernels=[dict(name=k["name"], launches=k["launches"], ms=round(k["total_ms"], 3)) for k in kernels], line=out)
            try:
                dpath = ROOT / args.details                  # an absolute --details stays as it is
                dpath.parent.mkdir(parents=True, exist_ok=True)
                dpath.write_text(json.dumps(details, indent=1))
            except OSError:
                out["details"] = None
        print(json.dumps(out), flush=True)
    if run is not None:
        run.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def _cleanup_shm():
    import shutil
    for d in SHM_DIRS:
        shutil.rmtree(d, ignore_errors=True)
        shutil.rmtree(d.with_name(d.name + ".tmp"), ignore_errors=True)


if __name__ == "__main__":
    import atexit
    atexit.register(_cleanup_shm)          # also on sys.exit / an exception; a SIGKILL leaves at most what remove_stale_shm() sweeps next time
    main()
