"""CPU pre-check of tests/test_gpu_beam_boost.py's phrase set: the float64 boosted reference search (tests/beam_boost_ref.py) over the f32
oracle's offline encoder rows (tests/offline_ref.py), for the test's runs.  Prints every pair's margins and whether the reference alone meets
the test's conditions (every pair with W <= 2 qualifies, at most a quarter left out, proposed_by_boost >= 1, the N-best moved in >= 3 pairs).
No GPU.
  usage: beam_boost_margins.py [--rows FILE.npz] [--quiet] [seed ..]      (default: the test's BOOST_SEED; several seeds scan)
--rows: also check the conditions on encoder rows an engine left (arrays "<name>_<T>" of shape [T][1024], e.g. the f32 and bf16 engines'
offline_tap(TAP_ENCODER_OUT) of the test's utterances): the GPU test runs the reference over ITS engine's rows, which differ from the oracle's
in the last bits (f32) or the third digit (bf16), so a seed has to hold on each.  The phrase set itself always comes from the oracle's rows."""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import __graft_entry__ as ge

ge.load_package()
from nemotron_asr_amd import synth
from oracle import binding as ob
from tests import beam_boost_ref as bbr
from tests import beam_lm_ref as blr
from tests import beam_ref as br
from tests import lm_ref
from tests import test_gpu_beam_boost as tg

import numpy as np

args = sys.argv[1:]
quiet = "--quiet" in args
args = [a for a in args if a != "--quiet"]
rows_file = None
if "--rows" in args:
    rows_file = args[args.index("--rows") + 1]
    del args[args.index("--rows"):args.index("--rows") + 2]
t0 = time.perf_counter()
W = tg.sharpened(synth.make_weights(n_layers=2), tg.GAIN)
om = tg.CachedOracle(ob.OracleModel(W, 2))
cpu = tg.cpu_reference(W, om, tg.build_mels())
encs = cpu["encs"]
ref_lm = lm_ref.RefLM(tg.make_lm(cpu["ids"]), 3, tg.LM_UNK)
print(f"{len(cpu['ids'])} expanded tokens, {len(cpu['nbest'])} reference transcripts, {len(cpu['near'])} ids at ranks 9 .. 12 "
      f"({sum(g < 3.5 for g in cpu['near'].values())} within 3.5 of the 8th output) ({time.perf_counter() - t0:.1f} s)")
row_sets = {"oracle": encs}
if rows_file:
    z = np.load(rows_file)
    for key in z.files:
        name, T = key.rsplit("_", 1)
        row_sets.setdefault(name, {})[int(T)] = z[key]
for seed in [int(a) for a in args] or [tg.BOOST_SEED]:
    phrases = tg.build_phrases(seed, cpu)
    ph = bbr.Phrases(phrases)
    print(f"seed {seed}: {len(phrases)} phrases {phrases}")
    all_met = True
    for name, rows in row_sets.items():
        joints = {T: bbr.OracleJoint(om, rows[T]) for T in rows}
        pairs = left = moved = proposed = 0
        ok = True
        for run in tg.RUNS:
            (Wd, S), with_lm = run
            for T in sorted(rows):
                free = (blr.search(joints[T], T, Wd, Wd, S, lm=ref_lm, weight=tg.LM_WEIGHT) if with_lm else br.search(joints[T], T, Wd, Wd, S))[0]
                hyps, st = bbr.search(joints[T], T, Wd, Wd, S, phrases=ph, lm=ref_lm if with_lm else None, weight=tg.LM_WEIGHT if with_lm else 0.0)
                U = max(len(h["tokens"]) for h in hyps)
                bound = (T + U + 1) * tg.LP_BOUND
                q = st["margin"] > 2 * bound and st["expand_margin"] > 2 * tg.LP_BOUND
                pairs += 1
                left += not q
                ok = ok and (q or Wd > 2)
                proposed += st["proposed_by_boost"]
                moved += [h["tokens"] for h in hyps] != [h["tokens"] for h in free]
                if not quiet:
                    print(f"seed {seed} {name} W{Wd}-S{S}-T{T}{'-lm' if with_lm else ''}: margin on keys / threshold {st['margin'] / (2 * bound):.2f}, merge gap / threshold "
                          f"{st['merge_margin'] / (2 * bound):.2f}, expansion cut / (2 LP_BOUND) {st['expand_margin'] / (2 * tg.LP_BOUND):.1f}, proposed by boost "
                          f"{st['proposed_by_boost']}, {'qualifies' if q else 'LEFT OUT'}, boosts {[h['boost'] for h in hyps]}")
        met = ok and left * 4 <= pairs and proposed >= 1 and moved >= 3
        all_met = all_met and met
        print(f"seed {seed} {name}: {pairs} pairs, {left} left out, N-best moved in {moved}, proposed by boost {proposed}, conditions {'MET' if met else 'NOT met'} "
              f"({time.perf_counter() - t0:.1f} s)")
    print(f"seed {seed}: conditions on every row set {'MET' if all_met else 'NOT met'}")
