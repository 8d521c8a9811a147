"""Cost of shallow fusion in the beam search (nasr_engine_set_lm): one JSON line.
  workload : 64 utterances x 20 s of speech PCM; 24 layers, speech checkpoint, bf16 -- the shape of tests/micro/beam_search_cost.py
  calls    : transcribe_beam at (4, 4) and (8, 4) without a model; with a 3-gram model of about 10^5 n-grams, pruned (no positive value,
             token_bonus 0) and unpruned (the same n-grams with one back-off above 0, so the prune's condition fails)
  wall     : the calls alternate in one process: one untimed call each, then REPEATS timed rounds over all of them (host clock around calls
             that end in a device synchronise); median, min, max, spread = (max - min) / median
           The timed calls with a model return the plain tuples (no lm=True): their wall time holds the search, not the LM read-out
  parent   : the script measures the library it loads.  On a tree without nasr_engine_set_lm it times the LM-free calls only; that is how
             the parent commit is measured in the same session: run it from a checkout of the parent, then here with
             --parent-json FILE (the parent's output lines, one or more), alternating.  It then prints, per LM-free call, the parent's
             medians, this library's median, the difference, the session's run-to-run spread (the largest (max - min) / median either side
             showed, and the distance between the parent's own runs) and whether the difference lies within it
The model: a unigram for every token, every bigram and trigram of the LM-free 4 x 4 N-best (the n-grams the search really meets) and
random ones that start at the tokens seen there, up to the size asked for; seeded."""
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
N_NGRAMS = 100_000
WEIGHT = 0.5


def stats(ts):
    ts = np.asarray(ts) * 1e3
    med = float(np.median(ts))
    return dict(median_ms=round(med, 2), min_ms=round(float(ts.min()), 2), max_ms=round(float(ts.max()), 2), spread=round(float((ts.max() - ts.min()) / med), 4))


def build_lm(hyps, rng):
    g = {(t,): (-float(rng.random()) * 6.0 - 0.5, -float(rng.random())) for t in range(1024)}
    g[(1025,)] = (-20.0, -0.5)
    g[(1026,)] = (-3.0, 0.0)
    seen = sorted({t for u in hyps for h in u for t in h[1]})
    for u in hyps:
        for h in u:
            y = [1025] + list(h[1]) + [1026]
            for i in range(len(y) - 1):
                g.setdefault(tuple(y[i:i + 2]), (-float(rng.random()) * 3.0 - 0.1, -float(rng.random()) if y[i + 1] != 1026 else 0.0))
            for i in range(len(y) - 2):
                g.setdefault(tuple(y[i:i + 3]), (-float(rng.random()) * 2.0 - 0.05, 0.0))
    real = len(g)
    tries = 0
    while len(g) < N_NGRAMS * 0.45 and seen and tries < 20 * N_NGRAMS:    # random bigrams from a token the search meets to any token
        tries += 1
        g.setdefault((seen[int(rng.integers(len(seen)))], int(rng.integers(1024))), (-float(rng.random()) * 3.0 - 0.1, -float(rng.random())))
    bigrams = [k for k in g if len(k) == 2 and k[1] != 1026]
    tries = 0
    while len(g) < N_NGRAMS and bigrams and tries < 20 * N_NGRAMS:        # ... and trigrams that extend a bigram of the set
        tries += 1
        k = bigrams[int(rng.integers(len(bigrams)))]
        g.setdefault(k + (int(rng.integers(1024)),), (-float(rng.random()) * 2.0 - 0.05, 0.0))
    return g, real


W = synth.make_weights(24, margins="speech")
pcms = [synth.make_speech_pcm(s, 20.0)[0] for s in range(64)]
eng = capi.Engine(W, n_layers=24, dtype=capi.DTYPE_BF16, max_streams=1)
has_lm = hasattr(capi.Engine, "set_lm")
calls = {f"beam {Wd} x {S}": (None, lambda Wd=Wd, S=S: eng.transcribe_beam(pcms, Wd, 0, S)) for Wd, S in SETTINGS}
res = {k: f() for k, (_, f) in calls.items()}                             # warm-up of the LM-free paths
info = {}
if has_lm:
    lm, real = build_lm(res["beam 4 x 4"], np.random.default_rng(7))
    pos = dict(lm)
    k0 = next(k for k in pos if len(k) == 1 and k[0] < 1024)
    pos[k0] = (pos[k0][0], 1e-3)                                          # one back-off above 0: the prune's condition fails
    t0 = time.perf_counter()
    eng.set_lm(lm, order=3, unk_logprob=-10.0, weight=WEIGHT)
    info = dict(ngrams=len(lm), from_the_n_best=real, set_lm_ms=round((time.perf_counter() - t0) * 1e3, 1), states=eng.counter("lm_states"),
                max_probe=eng.counter("lm_max_probe"))
    eng.set_lm(None)
    for Wd, S in SETTINGS:
        calls[f"beam {Wd} x {S} + lm pruned"] = (lm, lambda Wd=Wd, S=S: eng.transcribe_beam(pcms, Wd, 0, S))
        calls[f"beam {Wd} x {S} + lm unpruned"] = (pos, lambda Wd=Wd, S=S: eng.transcribe_beam(pcms, Wd, 0, S))
times = {k: [] for k in calls}
attach = []
attached = [None]
for rep in range(REPEATS + 1):                                            # round 0 is the untimed warm-up
    for k, (model, f) in calls.items():
        if has_lm and model is not attached[0]:                           # the dictionary is ordered LM-free, pruned, unpruned per setting
            t0 = time.perf_counter()
            eng.set_lm(model, order=3, unk_logprob=-10.0, weight=WEIGHT) if model is not None else eng.set_lm(None)
            attached[0] = model
            if model is not None and rep:
                attach.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        out = f()
        if rep:
            times[k].append(time.perf_counter() - t0)
        res[k] = out
eng.close()
med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
out = dict(library="with set_lm" if has_lm else "without set_lm", utterances=len(pcms), wall={k: stats(v) for k, v in times.items()}, lm=info)
if has_lm:
    out["set_lm_ms"] = stats(attach)
    for Wd, S in SETTINGS:
        b = f"beam {Wd} x {S}"
        out[b] = dict(lm_pruned_minus_lm_free_ms=round(med[b + " + lm pruned"] - med[b], 2), lost_prune_ms=round(med[b + " + lm unpruned"] - med[b + " + lm pruned"], 2),
                      best_changed=sum(1 for u in range(len(pcms)) if res[b + " + lm pruned"][u][0][1] != res[b][u][0][1]),
                      pruned_equals_unpruned=sum(1 for u in range(len(pcms)) if [h[1] for h in res[b + " + lm pruned"][u]] == [h[1] for h in res[b + " + lm unpruned"][u]]))
if "--parent-json" in sys.argv:
    parents = [json.loads(ln) for ln in open(sys.argv[sys.argv.index("--parent-json") + 1]) if ln.startswith("{") and '"without set_lm"' in ln]
    cmp = {}
    for k in [f"beam {Wd} x {S}" for Wd, S in SETTINGS]:
        pm = [p["wall"][k]["median_ms"] for p in parents]
        spread = max([p["wall"][k]["spread"] for p in parents] + [out["wall"][k]["spread"]] + [(max(pm) - min(pm)) / min(pm)])
        diff = out["wall"][k]["median_ms"] / float(np.mean(pm)) - 1.0
        cmp[k] = dict(parent_median_ms=pm, this_median_ms=out["wall"][k]["median_ms"], difference=round(diff, 4), session_spread=round(spread, 4),
                      within_spread=bool(diff <= spread))
    out["lm_free_against_parent"] = cmp
print(json.dumps(out, default=lambda o: o.item()))
