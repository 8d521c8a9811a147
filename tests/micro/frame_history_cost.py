"""Cost of engine option "frame_history" on one MI355X (24 layers, bf16, speech checkpoint, host PCM): ms per step in three regimes (20
untimed steps, three timed regions) for ONE build and ONE setting per process, the append launch's own device time from the engine's
profiler, and with `beam` nasr_engine_history_beam (4, 4) over 64 windows of 250 frames beside nasr_engine_transcribe_beam on the same
audio.  Usage: python tests/micro/frame_history_cost.py TREE N ROWS [beam] -- TREE = the root of a built checkout (this one, or the
parent commit's), N = frame_history (0: off), ROWS = history_append_rows (0: the rule).  profiles/frame_history.md: the arms parent /
off / N = 2048 / N = 2048 with four rows per workgroup, alternating, twice"""
import importlib.util, json, sys, time
import numpy as np  # noqa: F401
from pathlib import Path
root = Path(sys.argv[1]).resolve()
N, rows = int(sys.argv[2]), int(sys.argv[3])
sys.path.insert(0, str(root))
spec = importlib.util.spec_from_file_location("nemotron_asr_amd", root / "nemotron-asr.cpp_amd" / "__init__.py", submodule_search_locations=[str(root / "nemotron-asr.cpp_amd")])
mod = importlib.util.module_from_spec(spec); sys.modules["nemotron_asr_amd"] = mod; spec.loader.exec_module(mod)
from nemotron_asr_amd import capi, synth
W = synth.make_weights(24, margins="speech")
out = {}
def step_time(B, R, options, steps, warm=20, reps=3):
    eng = capi.Engine(W, n_layers=24, dtype=capi.DTYPE_BF16, max_streams=B)
    if N: eng.set_option("frame_history", N)
    if rows: eng.set_option("history_append_rows", rows)
    for k, v in options: eng.set_option(k, v)
    n = synth.shift_samples(R)
    sts = [eng.stream(R) for _ in range(B)]
    pcm = [synth.make_speech_pcm(b % 8, (steps * reps + warm + 2) * n / 16000)[0] for b in range(min(B, 8))]
    at, res = 0, []
    for rep in range(reps + 1):
        k = warm if rep == 0 else steps
        eng.synchronize(); t0 = time.perf_counter()
        for _ in range(k):
            eng.step(sts, [pcm[b % 8][at:at + n] for b in range(B)]); at += n
        eng.collect(sts); eng.synchronize()
        if rep: res.append((time.perf_counter() - t0) / k * 1e3)
    eng.close()
    return res
for name, (B, R, opts, steps) in {"1xR0 sync": (1, 0, (("pipeline", 0),), 300), "1xR0 pipeline4": (1, 0, (("pipeline", 4),), 300), "64xR13 pipeline4": (64, 13, (("pipeline", 4),), 40)}.items():
    out[name] = step_time(B, R, opts, steps)
if N:
    for B, R in ((1, 0), (64, 13)):
        eng = capi.Engine(W, n_layers=24, dtype=capi.DTYPE_BF16, max_streams=B)
        eng.set_option("frame_history", N)
        if rows: eng.set_option("history_append_rows", rows)
        eng.profile(True)
        n = synth.shift_samples(R)
        sts = [eng.stream(R) for _ in range(B)]
        pcm = [synth.make_speech_pcm(b % 8, 30 * n / 16000)[0] for b in range(min(B, 8))]
        for k in range(25): eng.step(sts, [pcm[b % 8][k * n:(k + 1) * n] for b in range(B)])
        a = {s["name"]: s for s in eng.profile_read()}["k_history_append"]
        out[f"append {B}xR{R} us"] = a["total_ms"] / a["launches"] * 1e3
        eng.close()
if N and len(sys.argv) > 4 and sys.argv[4] == "beam":
    # second pass: history_beam (4, 4) over 64 windows of 250 frames beside transcribe_beam on the same audio
    B, R = 64, 13
    eng = capi.Engine(W, n_layers=24, dtype=capi.DTYPE_BF16, max_streams=B)
    eng.set_option("frame_history", 256)
    n = synth.shift_samples(R)
    base = [synth.make_speech_pcm(b, 250 * 0.08 + 0.05)[0] for b in range(8)]
    pcms = [base[b % 8] for b in range(B)]
    sts = [eng.stream(R) for _ in range(B)]
    for o in range(0, pcms[0].size, n):
        eng.step(sts, [p[o:o + n] for p in pcms])
    eng.finalize(sts)
    wins = [(0, min(s.history_range()[1], 250)) for s in sts]
    print("frames kept", wins[0], flush=True)
    for rep in range(3):
        eng.synchronize(); t0 = time.perf_counter()
        h = eng.history_beam(sts, wins, beam=4, max_symbols=4)
        t1 = time.perf_counter()
        o = eng.transcribe_beam(pcms, beam=4, max_symbols=4)
        t2 = time.perf_counter()
        out.setdefault("history_beam ms", []).append((t1 - t0) * 1e3)
        out.setdefault("transcribe_beam ms", []).append((t2 - t1) * 1e3)
        print("beam", (t1 - t0) * 1e3, (t2 - t1) * 1e3, flush=True)
    eng.close()
print(json.dumps(out))
