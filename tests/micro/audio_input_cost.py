"""Cost of the device-side audio input conversion (nasr_engine_step_audio): one JSON line per case, all of them to the file named on the
command line (default profiles/audio_input_cost.json).
  workload : 64 and 512 streams x 1.12 s pushes (right_context = 13) of host buffers: 16 kHz s16 through nasr_engine_step for comparison,
             48 kHz s16, 8 kHz mu-law and 44.1 kHz f32 stereo (mixed) through nasr_engine_step_audio, the first two also with engine option
             "audio_lds_table" = 1 (coefficients from LDS); two warm-up pushes, five timed ones
  engine   : 2 layers, bf16: the converter and the upload do not depend on the encoder, so the step's own device time here is NOT the
             full model's (DESIGN section 0 has that); what is reported per step is the device time of the classes audio_convert and
             h2d_pcm (nasr_engine_profile: HIP events on the engine's stream), their bytes and FLOPs, and the sum over all classes"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge

ge.load_package()
from nemotron_asr_amd import capi, synth

W = synth.make_weights(n_layers=2)
out = []
R = 13
for S in (64, 512):
    for (fin, enc, ch, chan, lds) in ((16000, "s16", 1, 0, 0), (48000, "s16", 1, 0, 0), (48000, "s16", 1, 0, 1), (8000, "mulaw", 1, 0, 0), (8000, "mulaw", 1, 0, 1),
                                      (44100, "f32", 2, -1, 0)):
        e = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=S)
        e.set_option("audio_lds_table", lds)
        sts = [e.stream(R) for _ in range(S)]
        default = (fin, enc, ch, chan) == (16000, "s16", 1, 0)
        if not default:
            for s in sts:
                s.set_audio_format(fin, enc, ch, chan)
        frames = 17920 * fin // 16000
        rng = np.random.default_rng(1)
        dt = capi.AUDIO_DTYPES[capi.AUDIO_ENCODINGS[enc]]
        x = (rng.integers(0, 256, frames * ch).astype(dt) if dt == np.uint8 else (rng.standard_normal(frames * ch) * (3000 if dt == np.int16 else 0.1)).astype(dt))
        arrs = [x] * S
        push = (lambda: e.step(sts, arrs)) if default else (lambda: e.step_audio(sts, arrs))
        push(); push()
        e.profile(True)
        t0 = time.perf_counter()
        n = 5
        for _ in range(n):
            push()
        e.synchronize()
        wall = (time.perf_counter() - t0) / n
        st = {r["name"]: r for r in e.profile_read()}
        e.profile(False)
        rec = dict(streams=S, rate=fin, enc=enc, channels=ch, lds_table=lds, frames_per_push=frames, eager_step_wall_ms=1e3 * wall,
                   two_layer_step_device_ms=sum(r["total_ms"] for r in st.values()) / n)
        for k in ("audio_convert", "h2d_pcm"):
            if k in st:
                rec[k] = dict(ms_per_step=st[k]["total_ms"] / st[k]["launches"], bytes_per_step=st[k]["bytes"] / st[k]["launches"],
                              gflop_per_step=st[k]["flops"] / st[k]["launches"] / 1e9)
        out.append(rec)
        print(json.dumps(rec), flush=True)
        for s in sts:
            s.destroy()
        e.close()
dst = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "audio_input_cost.json"
dst.parent.mkdir(parents=True, exist_ok=True)
dst.write_text(json.dumps(out, indent=1))
