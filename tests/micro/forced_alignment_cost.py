"""Cost of forced alignment (nasr_engine_align) beside transcription of the same batch: one JSON line.
  workload    : 64 utterances x 20 s of speech PCM, each aligned to its own greedy transcript; 24 layers, speech checkpoint, bf16
  wall        : transcribe and align alternate in one process: one untimed call each, then REPEATS timed calls each (host clock around
                calls that end in a device synchronise); median, min, max, spread = (max - min) / median
  kernels     : device time of one align call by kernel class (nasr_engine_profile); for k_align_lattice its launches, cells per launch
                and its FLOP/s (2 x 640 x 1025 per cell) as a fraction of the 155 TFLOP/s f32 MFMA rate"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import __graft_entry__ as ge

ge.load_package()
from nemotron_asr_amd import capi, synth

REPEATS = 5
F32_MFMA_TFLOPS = 155.0


def stats(ts):
    ts = np.asarray(ts) * 1e3
    med = float(np.median(ts))
    return dict(median_ms=round(med, 2), min_ms=round(float(ts.min()), 2), max_ms=round(float(ts.max()), 2), spread=round(float((ts.max() - ts.min()) / med), 4))


W = synth.make_weights(24, margins="speech")
pcms = [synth.make_speech_pcm(s, 20.0)[0] for s in range(64)]
eng = capi.Engine(W, n_layers=24, dtype=capi.DTYPE_BF16, max_streams=1)
toks, _ = eng.transcribe(pcms)                          # warm-up of the offline path; the transcripts
eng.align(pcms, toks)                                   # warm-up of the alignment buffers
t_tr, t_al = [], []
for _ in range(REPEATS):
    t0 = time.perf_counter()
    eng.transcribe(pcms)
    t_tr.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    res = eng.align(pcms, toks)
    t_al.append(time.perf_counter() - t0)
eng.profile(True)
eng.align(pcms, toks)
prof = eng.profile_read()
eng.profile(False)
eng.set_debug(True)
eng.align(pcms[:1], toks[:1])
T0 = eng.offline_tap(capi.TAP_ENCODER_OUT, 0).shape[0]
eng.close()
n_tok = [len(t) for t in toks]
kern = sorted(({"name": p["name"], "launches": p["launches"], "ms": round(p["total_ms"], 3),
                "tflops": round(p["flops"] / (p["total_ms"] * 1e-3) / 1e12, 2) if p["total_ms"] > 0 and p["flops"] else None} for p in prof),
              key=lambda r: -r["ms"])
lat = next(p for p in prof if p["name"] == "k_align_lattice")
cells = lat["flops"] / (2.0 * 640 * 1025)
out = dict(utterances=len(pcms), audio_s=sum(p.size for p in pcms) / 16000.0, encoder_frames_of_utterance_0=T0,
           tokens=dict(min=min(n_tok), max=max(n_tok), total=sum(n_tok)),
           transcribe=stats(t_tr), align=stats(t_al), align_over_transcribe=round(float(np.median(t_al) / np.median(t_tr)), 3),
           lattice=dict(cells=int(round(cells)), launches=lat["launches"], cells_per_launch=int(round(cells / max(lat["launches"], 1))), ms=round(lat["total_ms"], 3),
                        tflops=round(lat["flops"] / (lat["total_ms"] * 1e-3) / 1e12, 2),
                        fraction_of_f32_mfma_rate=round(lat["flops"] / (lat["total_ms"] * 1e-3) / 1e12 / F32_MFMA_TFLOPS, 3)),
           loglik=dict(min=round(min(r[0] for r in res), 2), max=round(max(r[0] for r in res), 2)),
           kernels=kern)
print(json.dumps(out))
