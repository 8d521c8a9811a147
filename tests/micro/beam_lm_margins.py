"""CPU pre-check of tests/test_gpu_beam_lm.py's language model: the float64 fused reference search (tests/beam_lm_ref.py) over the f32
oracle's offline encoder rows (tests/offline_ref.py), for the test's runs.  Prints every pair's margins and whether the reference alone
meets the test's conditions (every pair with W <= 2 qualifies, at most a quarter left out).  No GPU.
  usage: beam_lm_margins.py [seed ..]      (default: the test's LM_SEED; several seeds scan)"""
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import __graft_entry__ as ge

ge.load_package()
from nemotron_asr_amd import synth
from oracle import binding as ob
from tests import beam_lm_ref as blr
from tests import beam_ref as br
from tests import lm_ref
from tests import test_gpu_beam_lm as tg

t0 = time.perf_counter()
W = tg.sharpened(synth.make_weights(n_layers=2), tg.GAIN)
om = tg.CachedOracle(ob.OracleModel(W, 2))
mels = tg.build_mels()
ids, encs = tg.expanded_tokens(W, om, mels)
print(f"{len(ids)} expanded tokens ({time.perf_counter() - t0:.1f} s)")
joints = {T: br.OracleJoint(om, encs[T]) for T in encs}
free = {(st, T): br.search(joints[T], T, st[0], st[0], st[1])[0] for st in tg.SETTINGS for T in encs}
for seed in [int(a) for a in sys.argv[1:]] or [tg.LM_SEED]:
    tg.LM_SEED = seed
    plain, pos = tg.make_lm(ids), tg.make_lm(ids, positive=True)
    refs = dict(plain=lm_ref.RefLM(plain, 3, tg.LM_UNK), pos=lm_ref.RefLM(pos, 3, tg.LM_UNK))
    pairs = left = moved = 0
    ok = True
    for (Wd, S), which, weight, bonus in tg.RUNS:
        for T in sorted(encs):
            hyps, st = blr.search(joints[T], T, Wd, Wd, S, lm=refs[which], weight=weight, bonus=bonus)
            U = max(len(h["tokens"]) for h in hyps)
            bound = (T + U + 1) * tg.LP_BOUND
            q = st["margin"] > 2 * bound and st["expand_margin"] > 2 * tg.LP_BOUND
            pairs += 1
            left += not q
            ok = ok and (q or Wd > 2)
            moved += [h["tokens"] for h in hyps] != [h["tokens"] for h in free[((Wd, S), T)]]
            print(f"seed {seed} W{Wd}-S{S}-T{T}-{which}: margin on totals / threshold {st['margin'] / (2 * bound):.2f}, merge gap / threshold "
                  f"{st['merge_margin'] / (2 * bound):.2f}, expansion cut / (2 LP_BOUND) {st['expand_margin'] / (2 * tg.LP_BOUND):.1f}, "
                  f"{'qualifies' if q else 'LEFT OUT'}, lengths {[len(h['tokens']) for h in hyps]}")
    print(f"seed {seed}: {len(plain)} n-grams, {pairs} pairs, {left} left out, N-best moved in {moved}, conditions {'MET' if ok and left * 4 <= pairs else 'NOT met'} "
          f"({time.perf_counter() - t0:.1f} s)")
