"""Phrase boosting inside the offline beam search (NASR_FLAG_BEAM_BOOST, nasr_engine_beam_hypothesis_boost), with and without the language
model, on the MI355X.

The set-up is that of tests/test_gpu_beam_lm.py, re-stated here: a 2-layer engine per dtype, the sharpened synthetic weights (GAIN = 30),
LP_BOUND = 2e-4, seed 12, utterances of T = 0, 1, 5, 13 encoder frames, settings (W, S) = (1, 10), (2, 3), (4, 3), (8, 2), plus (4, 3) with
that test's language model attached (LM_SEED 13, weight 0.5); engine option "phrase_boost" = 64 states.

The phrase set is built on the CPU (build_phrases) from the float64 reference search over the f32 oracle's offline encoder rows
(tests/offline_ref.py), so it is the same wherever the test runs: phrases of 1 .. 3 tokens cut from the unboosted reference N-best (matches
complete), the same with the last token replaced (matches fail midway and keep what they were paid), and phrases that start with an id just
outside the 8 largest raw outputs of a row the search evaluates (the boost proposes it).  Bonuses are drawn from {0.5, 1, 2, 4}: dyadic, so
boost sums are exact.  BOOST_SEED was chosen on the CPU (tests/micro/beam_boost_margins.py) so that the reference search alone meets the
conditions of test 3 and has proposed_by_boost >= 1 -- over the oracle's rows and over the encoder rows the f32 and the bf16 engine leave
(test 3 runs the reference over its engine's rows); profiles/beam_boost.md has the margins found on each.

Every figure is printed before it is asserted (run with -s)."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi, gguf_io, synth
from oracle import binding as ob
from tests import align_ref as ar
from tests import beam_boost_ref as bbr
from tests import beam_lm_ref as blr
from tests import beam_ref as br
from tests import lm_ref
from tests import offline_ref as orf

pytestmark = pytest.mark.gpu

BLANK, V = 1024, 1025
LP_BOUND = 2e-4
GAIN = 30.0
CASE_T = (0, 1, 5, 13)
SETTINGS = ((1, 10), (2, 3), (4, 3), (8, 2))
SEED = 12
LM_SEED, LM_WEIGHT, LM_UNK = 13, 0.5, -8.0
BOOST_SEED = 5
BONUSES = (0.5, 1.0, 2.0, 4.0)
CAPACITY = 64
RUNS = [(st, False) for st in SETTINGS] + [((4, 3), True)]             # (setting, with the LM)
BIN = Path(__file__).resolve().parent.parent / "nemotron-asr.cpp_amd" / "bin"


def mel_for(T, rng):
    """a log-mel of the fewest frames that give T encoder frames (the recipe of tests/test_gpu_offline.py)"""
    n = max(1, 8 * (T - 3))
    while orf.enc_frames(n) < T:
        n += 1
    assert orf.enc_frames(n) == T
    return rng.standard_normal((n, 128)).astype(np.float32)


def sharpened(W, gain):
    """the joint's output layer centred over the vocabulary and scaled (tests/test_gpu_align.py)"""
    w = dict(W)
    wo = np.asarray(W["joint.joint_net.2.weight"], np.float64)
    bo = np.asarray(W["joint.joint_net.2.bias"], np.float64)
    w["joint.joint_net.2.weight"] = ((wo - wo.mean(axis=0, keepdims=True)) * gain).astype(np.float32)
    w["joint.joint_net.2.bias"] = ((bo - bo.mean()) * gain).astype(np.float32)
    return w


def build_mels():
    rng = np.random.default_rng(SEED)
    mels = {T: mel_for(T, rng) for T in CASE_T if T > 0}
    mels[0] = np.zeros((0, 128), np.float32)
    return mels


class CachedOracle:
    """the oracle's decoder + joint with its calls remembered: the hypotheses of an utterance share most of their cells"""

    def __init__(self, om):
        self.om, self.memo = om, {}

    def decoder_joint(self, prev, h, c, enc_t):
        key = (int(prev), np.asarray(h).tobytes(), np.asarray(c).tobytes(), np.asarray(enc_t).tobytes())
        if key not in self.memo:
            self.memo[key] = self.om.decoder_joint(prev, h, c, enc_t)
        return self.memo[key]


def cpu_reference(W, om, mels):
    """the unboosted reference search at (4, 3) and (8, 2) over the f32 oracle's offline encoder rows: -> dict(encs, nbest = token lists, ids =
    the non-blank ids among the 8 largest outputs of the evaluated rows, near = {id: gap} of the non-blank ids at ranks 9 .. 12 of an evaluated
    row that are among no evaluated row's 8 largest, with the smallest logit distance to that row's 8th output, row0 = the fresh-state row of
    frame 0 of T = 13)"""
    ids, near, nbest, encs = set(), {}, [], {}
    rows = []
    for T in CASE_T:
        if T == 0:
            continue
        encs[T] = orf.encode(om.om, W, mels[T], 2)[2]
        joint = br.OracleJoint(om, encs[T])
        for Wd, S in ((4, 3), (8, 2)):
            nbest += [h["tokens"] for h in br.search(joint, T, Wd, Wd, S)[0] if h["tokens"]]
        rows += list(joint.rows.values())
    for row in rows:
        ids.update(int(k) for k in br.top_order(row)[:8] if int(k) != BLANK)
    for row in rows:
        order = br.top_order(row)
        for k in order[8:12]:
            gap = float(row[order[7]]) - float(row[k])
            if int(k) != BLANK and int(k) not in ids:
                near[int(k)] = min(near.get(int(k), np.inf), gap)
    row0 = np.asarray(br.OracleJoint(om, encs[13])(0, ()))
    return dict(encs=encs, nbest=nbest, ids=sorted(ids), near=near, row0=row0)


def build_phrases(seed, cpu):
    """-> [(tokens, bonus)]: 5 cuts of the reference N-best, 4 cuts with the last token replaced, 3 phrases that start outside the raw top-8"""
    rng = np.random.default_rng(seed)
    out, seen = [], set()

    def add(toks, w):
        toks = tuple(int(t) for t in toks)
        if toks and toks not in seen:
            seen.add(toks)
            out.append((toks, float(w)))

    def cut():
        h = cpu["nbest"][int(rng.integers(len(cpu["nbest"])))]
        n = int(rng.integers(1, min(3, len(h)) + 1))
        at = int(rng.integers(0, len(h) - n + 1))
        return list(h[at:at + n])

    while len(out) < 5:
        add(cut(), rng.choice(BONUSES))
    while len(out) < 9:
        c = cut()
        if len(c) < 2:
            continue
        c[-1] = int(rng.choice(cpu["ids"]))
        add(c, rng.choice(BONUSES))
    close = sorted(k for k, gap in cpu["near"].items() if gap < 3.5)
    assert len(close) >= 3, cpu["near"]
    for k in rng.choice(close, 3, replace=False):
        tail = [int(t) for t in rng.choice(cpu["ids"], int(rng.integers(0, 2)))]
        add([int(k)] + tail, 4.0)
    return out


def make_lm(ids):
    """the seeded random trigram of tests/test_gpu_beam_lm.py over `ids`"""
    rng = np.random.default_rng(LM_SEED)
    return lm_ref.random_lm(rng, 3, len(ids), tokens=ids, bos=True, eos=True, positive_backoff=False, density=0.05, max_per_level=1500)


@pytest.fixture(scope="module")
def W():
    return sharpened(synth.make_weights(n_layers=2), GAIN)


@pytest.fixture(scope="module")
def cpu(W):
    om = CachedOracle(ob.OracleModel(W, 2))
    c = cpu_reference(W, om, build_mels())
    c["om"] = om
    c["phrases"] = build_phrases(BOOST_SEED, c)
    c["lm"] = make_lm(c["ids"])
    c["ref_lm"] = lm_ref.RefLM(c["lm"], 3, LM_UNK)
    return c


def set_phrases(eng, phrases):
    eng.set_boost_phrases([p for p, _ in phrases], [w for _, w in phrases])


def rescore(eng, mels, hyps_of):
    """the engine's own lattice of every hypothesis: one ragged align call; -> {key: (loglik, best, frames, lps, lb, ly)}"""
    keys = [(k, r) for k, hyps in hyps_of.items() for r in range(len(hyps))]
    res = eng.align_mel([mels[k] for k, r in keys], [hyps_of[k][r][1] for k, r in keys])
    out = {}
    for u, (k, r) in enumerate(keys):
        lb, ly = eng.align_lattice(u, len(hyps_of[k][r][1]))
        out[(k, r)] = res[u] + (lb, ly)
    return out


def _key(hyps):
    return [(h[0], h[1], h[2], h[3].tobytes()) for h in hyps]


def _key_lm(hyps):
    return [(h[0], h[1], h[2], h[3].tobytes(), h[4], h[5], h[6].tobytes()) for h in hyps]


def boost_fields(h, with_lm):
    """(boost, total, token_bonuses) of a tuple of a boosted call"""
    return h[7:10] if with_lm else h[4:7]


@pytest.fixture(scope="module", params=[capi.DTYPE_F32, capi.DTYPE_BF16], ids=["f32", "bf16"])
def world(request, W, cpu):
    """one engine per dtype: the unflagged calls (empty and populated set, with and without the LM), the flagged calls with the empty set and
    after re-clearing, the boosted call per run, the engine's own lattices of every boosted hypothesis and the reference boosted search from
    the engine's encoder rows -- computed once"""
    mels = build_mels()
    group = [mels[T] for T in CASE_T]
    eng = capi.Engine(W, n_layers=2, dtype=request.param, max_streams=1)
    call = lambda st, **kw: eng.transcribe_beam_mel(group, beam=st[0], nbest=0, max_symbols=st[1], **kw)
    try:
        eng.set_option("phrase_boost", CAPACITY)
        eng.set_debug(True)
        free, empty, populated, recleared, got, own = {}, {}, {}, {}, {}, {}
        for st in SETTINGS:
            free[st] = call(st)
            if st == SETTINGS[0]:
                enc = {T: eng.offline_tap(capi.TAP_ENCODER_OUT, i) for i, T in enumerate(CASE_T)}
            empty[st] = call(st, boost=True)
        states_empty = eng.counter("boost_states")
        set_phrases(eng, cpu["phrases"])
        states = eng.counter("boost_states")
        for st in SETTINGS:
            populated[st] = call(st)
        for run in RUNS:
            st, with_lm = run
            if with_lm:
                eng.set_lm(cpu["lm"], order=3, unk_logprob=LM_UNK, weight=LM_WEIGHT, token_bonus=0.0)
                free["lm"] = call(st, lm=True)
            res = call(st, lm=with_lm, boost=True)
            got[run] = {T: res[i] for i, T in enumerate(CASE_T)}
        eng.set_boost_phrases(())                                  # re-cleared, the LM still attached
        recleared["lm"] = call((4, 3), lm=True, boost=True)
        eng.set_lm(None)
        for st in SETTINGS:
            recleared[st] = call(st, boost=True)
        for run in RUNS:
            own[run] = rescore(eng, mels, {T: got[run][T] for T in CASE_T if T > 0})
    finally:
        eng.close()
    om, phrases = cpu["om"], bbr.Phrases(cpu["phrases"])
    ref, ref_lat, ref_free = {}, {}, {}
    for T in CASE_T:
        if T == 0:
            continue
        joint = bbr.OracleJoint(om, enc[T])
        for run in RUNS:
            st, with_lm = run
            ref[(run, T)] = bbr.search(joint, T, st[0], st[0], st[1], phrases=phrases, lm=cpu["ref_lm"] if with_lm else None, weight=LM_WEIGHT if with_lm else 0.0)
            for r, h in enumerate(got[run][T]):
                ref_lat[(run, T, r)] = ar.lattice(om, enc[T], h[1])
    return dict(free=free, empty=empty, populated=populated, recleared=recleared, got=got, own=own, ref=ref, ref_lat=ref_lat, states=(states_empty, states))


def test_the_empty_set_changes_nothing(world):
    """1: with the flag on and the empty set, and after re-clearing a non-empty one, every hypothesis equals the unflagged call bit for bit, in
    order, with the LM attached too; boost is 0 and total the unflagged key.  An unflagged call with a populated set equals the unflagged call"""
    assert world["states"][0] == 2 and world["states"][1] > 2
    n = 0
    for st in SETTINGS:
        for i, T in enumerate(CASE_T):
            assert _key(world["empty"][st][i]) == _key(world["free"][st][i]) == _key(world["recleared"][st][i]), (st, T)
            assert _key(world["populated"][st][i]) == _key(world["free"][st][i]), (st, T)
            for h in world["empty"][st][i] + world["recleared"][st][i]:
                assert h[4] == 0.0 and h[5] == h[0] and not h[6].any() and h[6].shape == (len(h[1]),), (st, T)
                n += 1
    for i, T in enumerate(CASE_T):
        assert _key_lm(world["recleared"]["lm"][i]) == _key_lm(world["free"]["lm"][i]), T
        for h in world["recleared"]["lm"][i]:
            assert h[7] == 0.0 and h[8] == h[5], T
    assert n >= 60


def test_invariants_with_boost_on(world, cpu):
    """2: distinct, sorted by total; total == score (+ LM terms) + boost by the reference's expression; boost and the per-token bonuses equal
    brute force on the returned tokens exactly; the path-score, `best` and cell bounds against the engine's own lattice and the float64
    lattice; at most S symbols per frame; the N-best differs from the unboosted one in at least 3 (setting, utterance) pairs"""
    phrases = bbr.Phrases(cpu["phrases"])
    n = moved = 0
    for run in RUNS:
        (Wd, S), with_lm = run
        for ti, T in enumerate(CASE_T):
            hyps = world["got"][run][T]
            name = f"W{Wd}-S{S}-T{T}{'-lm' if with_lm else ''}"
            assert 1 <= len(hyps) <= Wd and len({tuple(h[1]) for h in hyps}) == len(hyps), name
            totals = [boost_fields(h, with_lm)[1] for h in hyps]
            assert all(a >= b for a, b in zip(totals, totals[1:])), name
            base = world["free"]["lm"][ti] if with_lm else world["free"][(Wd, S)][ti]
            moved += [h[1] for h in hyps] != [h[1] for h in base]
            worst_cell = worst_path = 0.0
            for r, h in enumerate(hyps):
                score, toks, frames, lps = h[:4]
                boost, total, bonuses = boost_fields(h, with_lm)
                U = len(toks)
                bound = (T + U + 1) * LP_BOUND
                want = phrases.bonuses(tuple(toks))
                assert bonuses.shape == (U,) and bonuses.tolist() == want and boost == sum(want), (name, r, boost, want)
                if with_lm:
                    lm, total_lm = h[4], h[5]
                    assert abs(lm - cpu["ref_lm"].score(toks)[0]) <= 1e-9 and total_lm == total, (name, r)
                    assert total == bbr.key_of(score, lm, U, LM_WEIGHT, 0.0, boost, True), (name, r)
                else:
                    assert total == score + boost, (name, r)
                assert len(frames) == U and lps.shape == (U,) and math.isfinite(score) and score <= 0.0, (name, r)
                if T == 0:
                    assert (score, toks, frames, boost) == (0.0, [], [], 0.0) and len(hyps) == 1
                    continue
                assert all(0 <= t < BLANK for t in toks) and all(0 <= f < T for f in frames) and all(a <= b for a, b in zip(frames, frames[1:])), (name, r)
                assert U == 0 or max(np.bincount(frames)) <= S, (name, r)
                loglik, best, _, _, lb, ly = world["own"][run][(T, r)]
                rb, ry = world["ref_lat"][(run, T, r)]
                for what, b_, y_, best_ in (("engine", lb.astype(np.float64), ly.astype(np.float64), best), ("float64", rb, ry, ar.recursions(rb, ry)["best"])):
                    path = ar.path_score(b_, y_, frames)
                    cell = max((abs(float(lps[i]) - float(y_[f, i])) for i, f in enumerate(frames)), default=0.0)
                    worst_cell, worst_path = max(worst_cell, cell), max(worst_path, abs(score - path) / bound)
                    assert abs(score - path) <= bound, (name, r, what, score, path)
                    assert score <= best_ + bound, (name, r, what, score, best_)
                    assert cell <= LP_BOUND, (name, r, what, cell)
                n += 1
            print(f"beam+boost {name}: {len(hyps)} hypotheses, lengths {[len(h[1]) for h in hyps]}, boosts {[boost_fields(h, with_lm)[0] for h in hyps]}, "
                  f"worst |lp - cell| {worst_cell:.3e}, worst |score - path| / bound {worst_path:.3f}")
    print(f"beam+boost: {n} hypotheses checked; the N-best differs from the unboosted one in {moved} of {len(RUNS) * len(CASE_T)} (setting, utterance) pairs")
    assert n >= 35 and moved >= 3


def test_equality_with_the_reference_where_its_margins_allow(world):
    """3: equality with tests/beam_boost_ref.py where the reference's smallest margin on keys exceeds 2 (T + U + 1) LP_BOUND and no expansion
    cut (on logit + bonus) is closer than 2 LP_BOUND; every pair with W <= 2 qualifies, at most a quarter of all pairs is left out"""
    pairs = left_out = frames_skipped = proposed = 0
    for run in RUNS:
        (Wd, S), with_lm = run
        for T in CASE_T:
            if T == 0:
                continue
            hyps, (ref, stats) = world["got"][run][T], world["ref"][(run, T)]
            U = max(len(h["tokens"]) for h in ref)
            bound = (T + U + 1) * LP_BOUND
            proposed += stats["proposed_by_boost"]
            print(f"beam+boost W{Wd}-S{S}-T{T}{'-lm' if with_lm else ''}: margin on keys / threshold {stats['margin'] / (2 * bound):.2f}, merge gap / threshold "
                  f"{stats['merge_margin'] / (2 * bound):.2f}, expansion cut / (2 LP_BOUND) {stats['expand_margin'] / (2 * LP_BOUND):.1f}, proposed by boost "
                  f"{stats['proposed_by_boost']}, reference lengths {[len(h['tokens']) for h in ref]}")
            assert stats["pruned"] is False
            pairs += 1
            if not (stats["margin"] > 2 * bound and stats["expand_margin"] > 2 * LP_BOUND):
                assert Wd > 2, f"W = {Wd}, T = {T} does not qualify (margin {stats['margin']:.3e}, cut {stats['expand_margin']:.3e}): change the boost seed, not the threshold"
                left_out += 1
                continue
            assert [h[1] for h in hyps] == [h["tokens"] for h in ref], (run, T)
            for h, g in zip(hyps, ref):
                boost, total, bonuses = boost_fields(h, with_lm)
                assert abs(h[0] - g["score"]) <= bound and boost == g["boost"] and bonuses.tolist() == g["bonuses"], (run, T)
                assert abs(total - g["total"]) <= bound, (run, T)
                if with_lm:
                    assert abs(h[4] - g["lm_final"]) <= 1e-9, (run, T)
            if stats["merge_margin"] > 2 * bound:
                assert [h[2] for h in hyps] == [h["frames"] for h in ref], (run, T)
            else:
                frames_skipped += 1
    print(f"beam+boost: {pairs} pairs, {left_out} left out, frames not compared in {frames_skipped}, children proposed by the boost in the reference {proposed}")
    assert pairs == 15 and left_out * 4 <= pairs and proposed >= 1


def test_the_boost_proposes(W, cpu):
    """4: T = 13, (4, 3), f32: a token v outside the 8 largest raw outputs of frame 0's fresh-state row (from the CPU oracle), as a one-token
    phrase with bonus 1000: rank 0 is [v] * (T * S), its ln P are its own lattice cells, boost == 1000 * T * S exactly, and the unboosted
    N-best never contains v"""
    mels = build_mels()
    T, Wd, S = 13, 4, 3
    order = br.top_order(cpu["row0"])
    v = int(next(k for k in order[8:] if int(k) != BLANK))
    assert v not in [int(k) for k in order[:8]]
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=1)
    try:
        eng.set_option("phrase_boost", 8)
        eng.set_debug(True)                                        # the lattice read-out below
        eng.set_boost_phrases([[v]], 1000.0)
        old = eng.transcribe_beam_mel([mels[T]], Wd, 0, S)[0]
        new = eng.transcribe_beam_mel([mels[T]], Wd, 0, S, boost=True)[0]
        top = new[0]
        res = eng.align_mel([mels[T]], [top[1]])[0]
        lb, ly = eng.align_lattice(0, len(top[1]))
    finally:
        eng.close()
    print(f"the boost proposes: token {v} (raw rank {list(order).index(v) + 1} at frame 0); rank 0 has {len(top[1])} tokens, score {top[0]:.3f}, boost {top[4]:.1f}")
    assert all(v not in h[1] for h in old)
    assert top[1] == [v] * (T * S) and top[2] == [t for t in range(T) for _ in range(S)]
    assert top[4] == 1000.0 * T * S and top[5] == top[0] + top[4] and top[6].tolist() == [1000.0] * (T * S)
    cell = max(abs(float(top[3][i]) - float(ly[f, i])) for i, f in enumerate(top[2]))
    print(f"the boost proposes: worst |lp - cell| {cell:.3e}")
    assert cell <= LP_BOUND and abs(top[0] - ar.path_score(lb.astype(np.float64), ly.astype(np.float64), top[2])) <= (T + len(top[1]) + 1) * LP_BOUND


@pytest.mark.parametrize("dtype", [capi.DTYPE_F32, capi.DTYPE_BF16], ids=["f32", "bf16"])
def test_bit_identity_with_boost_on(W, cpu, dtype):
    """5: a ragged batch (T = 0 included, more rows than one sub-batch of 70) equals each utterance alone, boost values included; with and
    without the LM"""
    mels = build_mels()
    order = [13, 5, 0, 1, 13, 13, 5, 13, 13, 13, 1]
    group = [mels[T] for T in order]

    def full(hyps):                                            # every field of every tuple, arrays by their bytes
        return [tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in h) for h in hyps]

    eng = capi.Engine(W, n_layers=2, dtype=dtype, max_streams=1)
    try:
        eng.set_option("phrase_boost", CAPACITY)
        set_phrases(eng, cpu["phrases"])
        for (Wd, S), with_lm in (((4, 3), False), ((8, 2), True)):
            if with_lm:
                eng.set_lm(cpu["lm"], order=3, unk_logprob=LM_UNK, weight=LM_WEIGHT, token_bonus=0.0)
            kw = dict(lm=with_lm, boost=True)
            alone = {T: full(eng.transcribe_beam_mel([mels[T]], Wd, 0, S, **kw)[0]) for T in CASE_T}
            batch = eng.transcribe_beam_mel(group, Wd, 0, S, **kw)
            eng.set_option("offline_rows", 70)
            cut = eng.transcribe_beam_mel(group, Wd, 0, S, **kw)
            eng.set_option("offline_rows", 16384)
            for i, T in enumerate(order):
                assert full(batch[i]) == alone[T] and full(cut[i]) == alone[T], (Wd, S, i, T)
            assert len(alone[0]) == 1 and alone[0][0][-3] == 0.0                  # T == 0: boost 0
            assert any(h[-3] > 0.0 for h in alone[13])
    finally:
        eng.close()


def test_errors(W, cpu):
    """6: the flag without the option; the flag with NASR_FLAG_NO_BOOST; the boost getter after an unboosted call -- each fails with a
    message and leaves the engine usable; a later set_boost_phrases does not change a read-out"""
    mels = build_mels()
    good = [mels[5], mels[13]]
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    try:
        base = _key(eng.transcribe_beam_mel(good, 2, 0, 3)[1])
        with pytest.raises(capi.NasrError, match="phrase_boost"):
            eng.transcribe_beam_mel(good, 2, 0, 3, boost=True)
        with pytest.raises(capi.NasrError, match="phrase_boost"):
            eng.transcribe_beam([np.zeros(16000, np.int16)], 2, 0, 3, boost=True)
        assert _key(eng.transcribe_beam_mel(good, 2, 0, 3)[1]) == base
    finally:
        eng.close()
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    try:
        eng.set_option("phrase_boost", CAPACITY)
        set_phrases(eng, cpu["phrases"])
        with pytest.raises(capi.NasrError, match="exclude"):
            eng.transcribe_beam_mel(good, 2, 0, 3, flags=capi.FLAG_NO_BOOST, boost=True)
        assert _key(eng.transcribe_beam_mel(good, 2, 0, 3)[1]) == base
        with pytest.raises(capi.NasrError, match="without phrase boosting"):
            eng.beam_hypothesis_boost(0, 0)
        hyps = eng.transcribe_beam_mel(good, 4, 0, 3, boost=True)[1]
        assert any(h[4] > 0 for h in hyps)
        eng.set_boost_phrases([[5]], 2.0)                                              # another set: the read-out of the last call stays
        again = [eng.beam_hypothesis_boost(1, r) for r in range(len(hyps))]
        assert [(b, t, x.tolist()) for b, t, x in again] == [(h[4], h[5], h[6].tolist()) for h in hyps]
        for u, rank in ((2, 0), (-1, 0), (0, 9), (0, -1)):
            with pytest.raises(capi.NasrError):
                eng.beam_hypothesis_boost(u, rank)
        assert capi.lib().nasr_engine_beam_hypothesis_boost(eng.h, 1, 0, None, None, None, 0) == len(hyps[0][1])       # cap 0 returns the count
        eng.transcribe_mel(good)
        with pytest.raises(capi.NasrError, match="no beam hypotheses"):
            eng.beam_hypothesis_boost(0, 0)
        eng.transcribe_beam_mel(good, 2, 0, 3, boost=True)
    finally:
        eng.close()


def test_cli_with_a_boost_file(tmp_path, W):
    """7: nemotron-transcribe-amd --beam 4 --boost-file on the synthetic PCM prints the ABI's values: the lines gain `boost` (and the key)"""
    vocab = gguf_io.synthetic_vocab()
    model = tmp_path / "model.gguf"
    gguf_io.write_gguf(model, W, gguf_io.default_hparams(n_layers=2), vocab)
    pcm = synth.make_pcm(2, 3.0)
    audio = tmp_path / "a.pcm"
    pcm.tofile(audio)
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=1)
    try:
        eng.set_option("phrase_boost", 4096)
        free = eng.transcribe_beam([pcm], 4, 3, 3)[0]
        toks = [t for h in free for t in h[1]]
        assert len(toks) >= 2
        phrase = free[-1][1][:2] if len(free[-1][1]) >= 2 else toks[:2]
        eng.set_boost_phrases([phrase], 2.0)
        hyps = eng.transcribe_beam([pcm], 4, 3, 3, boost=True)[0]
    finally:
        eng.close()
    boost_file = tmp_path / "boost.txt"
    boost_file.write_text("ids:" + ",".join(str(t) for t in phrase) + "\n", encoding="utf-8")
    exe = str(BIN / "nemotron-transcribe-amd")
    base = [exe, str(model), str(audio), "--f32", "--beam", "4", "--nbest", "3", "--max-symbols", "3", "--print-tokens"]
    r = subprocess.run(base + ["--boost-file", str(boost_file), "--boost-bonus", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    lines = r.stdout.strip().splitlines()
    rows = [ln.split(None, 4) for ln in lines if ln.split()[0] not in ("tokens", "frames")]
    out_toks = [[int(x) for x in ln.split()[1:]] for ln in lines if ln.split()[0] == "tokens"]
    assert len(rows) == len(hyps) and out_toks == [h[1] for h in hyps]
    for row, h in zip(rows, hyps):
        assert float(row[1]) == pytest.approx(h[0], abs=1e-5) and float(row[2]) == pytest.approx(h[4], abs=1e-5) and float(row[3]) == pytest.approx(h[5], abs=1e-5)
    assert any(h[4] > 0 for h in hyps)
    r = subprocess.run(base, capture_output=True, text=True, timeout=120)                    # without --boost-file: what it was
    assert r.returncode == 0, r.stderr[-800:]
    lines = r.stdout.strip().splitlines()
    assert [[int(x) for x in ln.split()[1:]] for ln in lines if ln.split()[0] == "tokens"] == [h[1] for h in free]
    r = subprocess.run([exe, str(model), str(audio), "--f32", "--boost-bonus", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stderr.strip()
