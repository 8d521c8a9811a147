"""Cost of the beam search (nasr_engine_transcribe_beam) beside greedy transcription of the same batch: one JSON line.
  workload    : 64 utterances x 20 s of speech PCM; 24 layers, speech checkpoint, bf16
  wall        : the calls alternate in one process: one untimed call each, then REPEATS timed rounds over all of them (host clock around
                calls that end in a device synchronise); median, min, max, spread = (max - min) / median
  encoder     : nasr_engine_align of the same audio against empty transcripts: the offline encoder plus one lattice column, the closest
                call to "the encoder alone" the ABI has; search = beam - encoder
  rounds      : the host enqueues T_max * (S + 1) rounds of 5 launches; the cost of one more round per frame = the difference between
                max_symbols S + 1 and S at the same beam, per frame of the longest utterance"""
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
SETTINGS = ((4, 3), (4, 4), (4, 5), (8, 4), (1, 4))
LAUNCHES_PER_ROUND = 5


def stats(ts):
    ts = np.asarray(ts) * 1e3
    med = float(np.median(ts))
    return dict(median_ms=round(med, 2), min_ms=round(float(ts.min()), 2), max_ms=round(float(ts.max()), 2), spread=round(float((ts.max() - ts.min()) / med), 4))


W = synth.make_weights(24, margins="speech")
pcms = [synth.make_speech_pcm(s, 20.0)[0] for s in range(64)]
empty = [[] for _ in pcms]
eng = capi.Engine(W, n_layers=24, dtype=capi.DTYPE_BF16, max_streams=1)
calls = {"transcribe": lambda: eng.transcribe(pcms), "encoder": lambda: eng.align(pcms, empty)}
for Wd, S in SETTINGS:
    calls[f"beam {Wd} x {S}"] = lambda Wd=Wd, S=S: eng.transcribe_beam(pcms, Wd, 0, S)
res = {k: f() for k, f in calls.items()}                # warm-up of every path
times = {k: [] for k in calls}
for _ in range(REPEATS):
    for k, f in calls.items():
        t0 = time.perf_counter()
        f()
        times[k].append(time.perf_counter() - t0)
eng.set_debug(True)
longest = max(range(len(pcms)), key=lambda u: pcms[u].size)          # the host enqueues rounds by the longest utterance of a sub-batch
eng.transcribe([pcms[longest]])
T0 = eng.offline_tap(capi.TAP_ENCODER_OUT, 0).shape[0]
eng.close()
med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
greedy = res["transcribe"][0]
b44 = res["beam 4 x 4"]
out = dict(utterances=len(pcms), audio_s=sum(p.size for p in pcms) / 16000.0, encoder_frames_of_longest_utterance=T0,
           greedy_tokens=sum(len(t) for t in greedy), wall={k: stats(v) for k, v in times.items()},
           search_ms={k: round(med[k] - med["encoder"], 2) for k in med if k.startswith("beam")},
           over_transcribe={k: round(med[k] / med["transcribe"], 3) for k in med if k.startswith("beam")},
           launches_per_frame={f"S = {S}": LAUNCHES_PER_ROUND * (S + 1) for S in (3, 4, 5)},
           one_more_round_per_frame_us=dict(S3_to_S4=round((med["beam 4 x 4"] - med["beam 4 x 3"]) * 1e3 / T0, 2), S4_to_S5=round((med["beam 4 x 5"] - med["beam 4 x 4"]) * 1e3 / T0, 2)),
           beam_4x4=dict(best_equals_greedy=sum(1 for u in range(len(pcms)) if b44[u][0][1] == greedy[u]), hypotheses=sum(len(h) for h in b44),
                         best_tokens=sum(len(h[0][1]) for h in b44), most_on_one_frame=max((max(np.bincount(h[0][2])) if h[0][2] else 0) for h in b44)))
print(json.dumps(out, default=lambda o: o.item()))
