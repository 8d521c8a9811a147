"""Cost of phrase boosting in the beam search (NASR_FLAG_BEAM_BOOST): one JSON line.
  workload : 64 utterances x 20 s of speech PCM; 24 layers, speech checkpoint, bf16 -- the shape of tests/micro/beam_search_cost.py
  calls    : transcribe_beam at (4, 4) and (8, 4): unflagged; flag on with the empty set (the boosted joint form with its raw-logit store, the
             BOOST select with its extra loads; the prune stays); flag on with a populated set (unpruned); and, beside it, the unflagged call
             with a language model whose one positive back-off switches the prune off (a unigram model: the cheapest look-up)
  wall     : the calls alternate in one process: one untimed round, then REPEATS timed rounds over all of them (host clock around calls that
             end in a device synchronise); median, min, max, spread = (max - min) / median.  The timed calls return the plain tuples
  parent   : the script measures the library it loads.  On a tree without nasr_engine_beam_hypothesis_boost it times the unflagged calls
             only; that is how the parent commit is measured in the same session: run it from a checkout of the parent, then here with
             --parent-json FILE (the parent's output lines, one or more), alternating.  It then prints, per unflagged call, the parent's
             medians, this library's median, the difference, the session's run-to-run spread (the largest (max - min) / median either side
             showed, and the distance between the parent's own runs) and whether the difference lies within it
The phrase set: PHRASES cuts of 1 .. 3 tokens from the unflagged 4 x 4 N-best (so they match), bonuses drawn from {0.5, 1, 2, 4}; seeded."""
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
SETTINGS = ((4, 4), (8, 4))
PHRASES = 300


def stats(ts):
    ts = np.asarray(ts) * 1e3
    med = float(np.median(ts))
    return dict(median_ms=round(med, 2), min_ms=round(float(ts.min()), 2), max_ms=round(float(ts.max()), 2), spread=round(float((ts.max() - ts.min()) / med), 4))


def build_phrases(hyps, rng):
    seqs = [h[1] for u in hyps for h in u if h[1]]
    out = {}
    while len(out) < PHRASES and seqs:
        y = seqs[int(rng.integers(len(seqs)))]
        n = int(rng.integers(1, min(3, len(y)) + 1))
        at = int(rng.integers(0, len(y) - n + 1))
        out.setdefault(tuple(y[at:at + n]), float(rng.choice((0.5, 1.0, 2.0, 4.0))))
    return out


W = synth.make_weights(24, margins="speech")
pcms = [synth.make_speech_pcm(s, 20.0)[0] for s in range(64)]
eng = capi.Engine(W, n_layers=24, dtype=capi.DTYPE_BF16, max_streams=1)
has_boost = hasattr(capi.Engine, "beam_hypothesis_boost")
if has_boost:
    eng.set_option("phrase_boost", 4096)
calls = {f"beam {Wd} x {S}": ("free", lambda Wd=Wd, S=S: eng.transcribe_beam(pcms, Wd, 0, S)) for Wd, S in SETTINGS}
res = {k: f() for k, (_, f) in calls.items()}                             # warm-up of the unflagged paths
info = {}
if has_boost:
    phrases = build_phrases(res["beam 4 x 4"], np.random.default_rng(7))
    lm = {(t,): (-1.0 - 0.1 * (t % 7), 1e-3 if t == 0 else 0.0) for t in range(1024)}       # one back-off above 0: unpruned
    for Wd, S in SETTINGS:
        calls[f"beam {Wd} x {S} + flag, empty set"] = ("empty", lambda Wd=Wd, S=S: eng.transcribe_beam(pcms, Wd, 0, S, flags=capi.FLAG_BEAM_BOOST))
        calls[f"beam {Wd} x {S} + flag, {PHRASES} phrases"] = ("set", lambda Wd=Wd, S=S: eng.transcribe_beam(pcms, Wd, 0, S, flags=capi.FLAG_BEAM_BOOST))
        calls[f"beam {Wd} x {S} + lm unpruned"] = ("lm", lambda Wd=Wd, S=S: eng.transcribe_beam(pcms, Wd, 0, S))
times = {k: [] for k in calls}
state = [None]
for rep in range(REPEATS + 1):                                            # round 0 is the untimed warm-up
    for k, (mode, f) in calls.items():
        if has_boost and mode != state[0]:
            eng.set_boost_phrases(list(phrases), list(phrases.values())) if mode == "set" else eng.set_boost_phrases(())
            eng.set_lm(lm, order=1, unk_logprob=-10.0, weight=0.5) if mode == "lm" else eng.set_lm(None)
            state[0] = mode
        t0 = time.perf_counter()
        out = f()
        if rep:
            times[k].append(time.perf_counter() - t0)
        res[k] = out
if has_boost:
    info = dict(phrases=len(phrases), boost_states=None)
    eng.set_boost_phrases(list(phrases), list(phrases.values()))
    info["boost_states"] = eng.counter("boost_states")
eng.close()
med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
out = dict(library="with beam boost" if has_boost else "without beam boost", utterances=len(pcms), wall={k: stats(v) for k, v in times.items()}, boost=info)
if has_boost:
    for Wd, S in SETTINGS:
        b = f"beam {Wd} x {S}"
        out[b] = dict(flag_empty_minus_unflagged_ms=round(med[b + " + flag, empty set"] - med[b], 2),
                      populated_minus_empty_ms=round(med[b + f" + flag, {PHRASES} phrases"] - med[b + " + flag, empty set"], 2),
                      populated_over_unflagged=round(med[b + f" + flag, {PHRASES} phrases"] / med[b], 3),
                      lm_unpruned_over_unflagged=round(med[b + " + lm unpruned"] / med[b], 3),
                      empty_equals_unflagged=sum(1 for u in range(len(pcms)) if [(h[0], h[1], h[2]) for h in res[b + " + flag, empty set"][u]] == [(h[0], h[1], h[2]) for h in res[b][u]]),
                      best_changed_by_the_set=sum(1 for u in range(len(pcms)) if res[b + f" + flag, {PHRASES} phrases"][u][0][1] != res[b][u][0][1]))
if "--parent-json" in sys.argv:
    parents = [json.loads(ln) for ln in open(sys.argv[sys.argv.index("--parent-json") + 1]) if ln.startswith("{") and '"without beam boost"' in ln]
    cmp = {}
    for k in [f"beam {Wd} x {S}" for Wd, S in SETTINGS]:
        pm = [p["wall"][k]["median_ms"] for p in parents]
        spread = max([p["wall"][k]["spread"] for p in parents] + [out["wall"][k]["spread"]] + [(max(pm) - min(pm)) / min(pm)])
        diff = out["wall"][k]["median_ms"] / float(np.mean(pm)) - 1.0
        cmp[k] = dict(parent_median_ms=pm, this_median_ms=out["wall"][k]["median_ms"], difference=round(diff, 4), session_spread=round(spread, 4),
                      within_spread=bool(diff <= spread))
    out["unflagged_against_parent"] = cmp
print(json.dumps(out, default=lambda o: o.item()))
