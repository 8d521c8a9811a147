"""Offline path throughput (nasr_engine_transcribe): one JSON line.
  rtfx        : 64 utterances x 20 s of speech PCM, 24 layers, bf16 engine fed Q8_0 tensors, one call (median of 3 after a warm-up)
  kernels     : per-kernel-class device time of one such call (nasr_engine_profile)
  attention   : k_off_attn_bf16 alone (1-layer engine, its profile entry) at B = 8 utterances of T frames, in useful TFLOP/s:
                4 T^2 128 (QK + PV) + 2 T^2 128 (position term) per head"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import __graft_entry__ as ge

ge.load_package()
from nemotron_asr_amd import capi, synth


def mel_frames_for(T):
    n = 8 * (T - 3)
    while (((n // 2 + 1) // 2 + 1) // 2 + 1) < T:
        n += 1
    return n


out = {}
W = synth.make_weights(24, margins="speech")
WQ = synth.quantize_weights(W, "q8_0")[0]
pcms = [synth.make_speech_pcm(s, 20.0)[0] for s in range(64)]
audio_s = sum(p.size for p in pcms) / 16000.0
eng = capi.Engine(WQ, n_layers=24, dtype=capi.DTYPE_BF16, max_streams=1)
eng.transcribe(pcms)                                   # warm-up: position table, buffers
times = []
for _ in range(3):
    t0 = time.perf_counter()
    eng.transcribe(pcms)
    times.append(time.perf_counter() - t0)
wall = float(np.median(times))
eng.profile(True)
eng.transcribe(pcms)
prof = eng.profile_read()
eng.profile(False)
eng.close()
tot = sum(p["total_ms"] for p in prof)
out["rtfx"] = dict(utterances=64, audio_s=audio_s, wall_ms=wall * 1e3, rtfx=audio_s / wall, device_ms_profiled=tot)
out["kernels"] = sorted(({"name": p["name"], "launches": p["launches"], "ms": round(p["total_ms"], 3),
                          "tflops": round(p["flops"] / (p["total_ms"] * 1e-3) / 1e12, 1) if p["total_ms"] > 0 and p["flops"] else None}
                         for p in prof), key=lambda r: -r["ms"])
W1 = synth.make_weights(1)
e1 = capi.Engine(W1, n_layers=1, dtype=capi.DTYPE_BF16, max_streams=1)
rng = np.random.default_rng(0)
att = []
for T in (256, 1024, 2048):
    mels = [rng.standard_normal((mel_frames_for(T), 128)).astype(np.float32) for _ in range(8)]
    e1.transcribe_mel(mels)
    e1.profile(True)
    for _ in range(3):
        e1.transcribe_mel(mels)
    pr = {p["name"]: p for p in e1.profile_read()}
    e1.profile(False)
    a = pr["k_off_attention"]
    ms = a["total_ms"] / a["launches"]
    layer_ms = sum(p["total_ms"] for n, p in pr.items() if n not in ("k_mel", "k_off_conv0_dw", "k_sub_dw", "k_encproj", "k_dec_iter")) / a["launches"]
    useful = 8 * 8 * 6.0 * T * T * 128
    att.append(dict(T=T, B=8, attn_ms=round(ms, 3), tflops=round(useful / (ms * 1e-3) / 1e12, 1), layer_ms_approx=round(layer_ms, 3),
                    attn_share_of_layer=round(ms / layer_ms, 3)))
e1.close()
out["attention"] = att
print(json.dumps(out))
