"""Shallow fusion of a back-off n-gram language model in the beam search (nasr_engine_set_lm / _set_lm_weights / _beam_hypothesis_lm), on
the MI355X.

The set-up is that of tests/test_gpu_beam.py, re-stated here: a 2-layer engine per dtype, the sharpened synthetic weights (GAIN = 30),
LP_BOUND = 2e-4, seed 12, utterances of T = 0, 1, 5, 13 encoder frames, settings (W, S) = (1, 10), (2, 3), (4, 3), (8, 2).

The model is a seeded random trigram with BOS and EOS entries over tokens the LM-free search expands on these utterances (the non-blank
ids among the 8 largest outputs of the rows the float64 reference search evaluates over the f32 oracle's offline encoder rows,
tests/offline_ref.py -- CPU work, so the model is the same wherever the test runs); every other id gets the unk value.  LM_SEED and
LM_WEIGHT were chosen on the CPU (tests/micro/beam_lm_margins.py) so that the reference search alone meets the conditions of test 3;
profiles/beam_lm.md has the margins found there and on the GPU.  One more setting, (4, 3) with a positive back-off and token_bonus > 0,
covers the unpruned path.

Every figure is printed before it is asserted (run with -s)."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi, gguf_io, synth
from oracle import binding as ob
from tests import align_ref as ar
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
EXTRA = dict(setting=(4, 3), weight=0.5, bonus=0.25)        # with a positive back-off: the search runs unpruned
BIN = Path(__file__).resolve().parent.parent / "nemotron-asr.cpp_amd" / "bin"
GOLDEN = Path(__file__).resolve().parent / "golden"
BOS, EOS = lm_ref.BOS, lm_ref.EOS


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


def expanded_tokens(W, om, mels):
    """the non-blank ids among the 8 largest outputs of every row the LM-free reference search evaluates at (4, 3) and (8, 2), over the f32
    oracle's offline encoder rows; -> (sorted ids, {T: encoder rows})"""
    ids, encs = set(), {}
    for T in CASE_T:
        if T == 0:
            continue
        encs[T] = orf.encode(om.om, W, mels[T], 2)[2]
        joint = br.OracleJoint(om, encs[T])
        for Wd, S in ((4, 3), (8, 2)):
            br.search(joint, T, Wd, Wd, S)
        for row in joint.rows.values():
            ids.update(int(k) for k in br.top_order(row)[:8] if int(k) != BLANK)
    return sorted(ids), encs


def make_lm(ids, positive=False):
    """the seeded random trigram over `ids`; positive: some back-offs above 0"""
    rng = np.random.default_rng(LM_SEED)
    return lm_ref.random_lm(rng, 3, len(ids), tokens=ids, bos=True, eos=True, positive_backoff=positive, density=0.05, max_per_level=1500)


@pytest.fixture(scope="module")
def W():
    return sharpened(synth.make_weights(n_layers=2), GAIN)


@pytest.fixture(scope="module")
def lms(W):
    om = CachedOracle(ob.OracleModel(W, 2))
    ids, _ = expanded_tokens(W, om, build_mels())
    plain, pos = make_lm(ids), make_lm(ids, positive=True)
    assert any(bo > 0 for _, bo in pos.values()) and all(bo <= 0 for _, bo in plain.values())
    return dict(om=om, ids=ids, plain=plain, pos=pos, ref=lm_ref.RefLM(plain, 3, LM_UNK), ref_pos=lm_ref.RefLM(pos, 3, LM_UNK))


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


RUNS = [(st, "plain", LM_WEIGHT, 0.0) for st in SETTINGS] + [(EXTRA["setting"], "pos", EXTRA["weight"], EXTRA["bonus"])]


@pytest.fixture(scope="module", params=[capi.DTYPE_F32, capi.DTYPE_BF16], ids=["f32", "bf16"])
def world(request, W, lms):
    """one engine per dtype: the LM-free call, the call at weight 0, the call after detaching and the fused call per setting, the engine's own
    lattices of every fused hypothesis, and the reference fused search from the engine's encoder rows -- computed once"""
    mels = build_mels()
    group = [mels[T] for T in CASE_T]
    eng = capi.Engine(W, n_layers=2, dtype=request.param, max_streams=1)
    try:
        eng.set_debug(True)
        free, zero, got, own, counters = {}, {}, {}, {}, {}
        for st in SETTINGS:
            free[st] = eng.transcribe_beam_mel(group, beam=st[0], nbest=0, max_symbols=st[1])
            if st == SETTINGS[0]:
                enc = {T: eng.offline_tap(capi.TAP_ENCODER_OUT, i) for i, T in enumerate(CASE_T)}
        counters["detached"] = [eng.counter(n) for n in ("lm_ngrams", "lm_states", "lm_max_probe")]
        eng.set_lm(lms["plain"], order=3, unk_logprob=LM_UNK, weight=0.0, token_bonus=0.0)
        counters["attached"] = [eng.counter(n) for n in ("lm_ngrams", "lm_states", "lm_max_probe")]
        for st in SETTINGS:
            zero[st] = eng.transcribe_beam_mel(group, beam=st[0], nbest=0, max_symbols=st[1], lm=True)
        for run in RUNS:
            st, which, weight, bonus = run
            eng.set_lm(lms[which], order=3, unk_logprob=LM_UNK, weight=weight, token_bonus=bonus)
            res = eng.transcribe_beam_mel(group, beam=st[0], nbest=0, max_symbols=st[1], lm=True)
            got[run] = {T: res[i] for i, T in enumerate(CASE_T)}
        for run in RUNS:
            own[run] = rescore(eng, mels, {T: got[run][T] for T in CASE_T if T > 0})
        eng.set_lm(None)
        counters["after"] = [eng.counter(n) for n in ("lm_ngrams", "lm_states", "lm_max_probe")]
        after = {st: eng.transcribe_beam_mel(group, beam=st[0], nbest=0, max_symbols=st[1]) for st in SETTINGS}
    finally:
        eng.close()
    om = lms["om"]
    ref, ref_lat = {}, {}
    for T in CASE_T:
        if T == 0:
            continue
        joint = br.OracleJoint(om, enc[T])
        for run in RUNS:
            st, which, weight, bonus = run
            ref[(run, T)] = blr.search(joint, T, st[0], st[0], st[1], lm=lms["ref" if which == "plain" else "ref_pos"], weight=weight, bonus=bonus)
            for r, h in enumerate(got[run][T]):
                ref_lat[(run, T, r)] = ar.lattice(om, enc[T], h[1])
    return dict(free=free, zero=zero, after=after, got=got, own=own, ref=ref, ref_lat=ref_lat, counters=counters)


def test_weight_zero_and_detaching_change_nothing(world, lms):
    """1: attached at weight 0 / bonus 0 every hypothesis equals the LM-free call bit for bit, in order; after set_lm(None) too"""
    assert world["counters"]["detached"] == [0, 0, 0] == world["counters"]["after"]
    n_ng, n_st, probe = world["counters"]["attached"]
    assert n_ng == len(lms["plain"]) and n_st == 1 + sum(1 for k in lms["plain"] if len(k) < 3) and probe >= 1
    n = 0
    for st in SETTINGS:
        for i, T in enumerate(CASE_T):
            assert _key(world["zero"][st][i]) == _key(world["free"][st][i]) == _key(world["after"][st][i]), (st, T)
            for h in world["zero"][st][i]:
                assert h[5] == h[0], (st, T)                  # total == score bit for bit
                n += 1
    assert n >= 30


def test_invariants_with_the_lm_on(world, lms):
    """2: the path-score, `best` and cell bounds against the engine's own lattice and the float64 lattice still hold; lm_logprob is lm_ref of
    the returned tokens (EOS included); the per-token values sum to it; total is score + weight * lm + bonus * len; distinct, sorted by total"""
    n = moved = 0
    for run in RUNS:
        (Wd, S), which, weight, bonus = run
        ref_lm = lms["ref" if which == "plain" else "ref_pos"]
        for ti, T in enumerate(CASE_T):
            hyps = world["got"][run][T]
            name = f"W{Wd}-S{S}-T{T}-{which}"
            assert 1 <= len(hyps) <= Wd and len({tuple(h[1]) for h in hyps}) == len(hyps), name
            assert all(a[5] >= b[5] for a, b in zip(hyps, hyps[1:])), name
            moved += [h[1] for h in hyps] != [h[1] for h in world["free"][(Wd, S)][ti]]
            worst_cell = worst_path = worst_lm = 0.0
            for r, (score, toks, frames, lps, lm, total, tok_lm) in enumerate(hyps):
                U = len(toks)
                bound = (T + U + 1) * LP_BOUND
                want, terms = ref_lm.score(toks)
                worst_lm = max(worst_lm, abs(lm - want))
                assert abs(lm - want) <= 1e-9, (name, r, lm, want)
                assert tok_lm.shape == (U,) and np.array_equal(tok_lm, np.asarray(terms, np.float32)), (name, r)
                eos_term = want - sum(terms)
                assert abs(float(tok_lm.astype(np.float64).sum()) + eos_term - lm) <= 1e-6 * (U + 1), (name, r)      # f32 rounding of terms below 16 in size
                assert total == blr.total_of(score, lm, U, weight, bonus), (name, r)
                assert len(frames) == U and lps.shape == (U,) and math.isfinite(score) and score <= 0.0, (name, r)
                if T == 0:
                    assert (score, toks, frames) == (0.0, [], []) and len(hyps) == 1
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
            print(f"beam+lm {name}: {len(hyps)} hypotheses, lengths {[len(h[1]) for h in hyps]}, worst |lp - cell| {worst_cell:.3e}, "
                  f"worst |score - path| / bound {worst_path:.3f}, worst |lm - ref| {worst_lm:.2e}")
    print(f"beam+lm: {n} hypotheses checked; the N-best differs from the LM-free one in {moved} of {len(RUNS) * len(CASE_T)} (setting, utterance) pairs")
    assert n >= 35 and moved >= 3                              # the model bites


def test_equality_with_the_reference_where_its_margins_allow(world):
    """3: equality with tests/beam_lm_ref.py where the reference's smallest margin on totals exceeds 2 (T + U + 1) LP_BOUND and no expansion
    cut is closer than 2 LP_BOUND; every pair with W <= 2 qualifies, at most a quarter of all pairs is left out"""
    pairs = left_out = frames_skipped = by_cut_alone = 0
    for run in RUNS:
        (Wd, S), which, weight, bonus = run
        for T in CASE_T:
            if T == 0:
                continue
            hyps, (ref, stats) = world["got"][run][T], world["ref"][(run, T)]
            U = max(len(h["tokens"]) for h in ref)
            bound = (T + U + 1) * LP_BOUND
            print(f"beam+lm W{Wd}-S{S}-T{T}-{which}: margin on totals / threshold {stats['margin'] / (2 * bound):.2f}, merge gap / threshold "
                  f"{stats['merge_margin'] / (2 * bound):.2f}, expansion cut / (2 LP_BOUND) {stats['expand_margin'] / (2 * LP_BOUND):.1f}, pruned "
                  f"{stats['pruned']}, reference lengths {[len(h['tokens']) for h in ref]}")
            assert stats["pruned"] is False                    # the reference runs unpruned; the engine prunes where it may
            pairs += 1
            if not (stats["margin"] > 2 * bound and stats["expand_margin"] > 2 * LP_BOUND):
                assert Wd > 2, f"W = {Wd}, T = {T} does not qualify (margin {stats['margin']:.3e}, cut {stats['expand_margin']:.3e}): change the LM seed, not the threshold"
                left_out += 1
                by_cut_alone += 1 if stats["margin"] > 2 * bound else 0
                continue
            assert [h[1] for h in hyps] == [h["tokens"] for h in ref], (run, T)
            for h, g in zip(hyps, ref):
                assert abs(h[0] - g["score"]) <= bound and abs(h[4] - g["lm_final"]) <= 1e-9, (run, T)
                assert abs(h[5] - g["total"]) <= bound, (run, T)
            if stats["merge_margin"] > 2 * bound:
                assert [h[2] for h in hyps] == [h["frames"] for h in ref], (run, T)
            else:
                frames_skipped += 1
    print(f"beam+lm: {pairs} pairs, {left_out} left out ({by_cut_alone} of them by the expansion cut alone), frames not compared in {frames_skipped}")
    assert pairs == 15 and left_out * 4 <= pairs


def test_the_lm_decides(W):
    """4: a token of the LM-free rank 0 at (4, 3) on T = 13 gets a unigram of -20 (everything else costs 0) at weight 1: the new rank 0 does
    not contain it and its model score is not above the old rank 0's.  The token is one that occurs in rank 0 and not in some lower rank.
    On these weights no such token exists -- on both engines all four hypotheses contain every token of rank 0 ([655, 44, 912, 1003, 255,
    655, 595, 44]; the lower ranks swap two tokens or insert one) -- so the rule falls back to the first token that occurs exactly once
    in rank 0 (912).  The fused search, not a re-ranking of the LM-free N-best, then has to find the transcript without it."""
    mels = build_mels()
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=1)
    try:
        old = eng.transcribe_beam_mel([mels[13]], 4, 0, 3)[0]
        print(f"the LM decides: LM-free N-best {[h[1] for h in old]}")
        cands = [t for t in old[0][1] if any(t not in h[1] for h in old[1:])]
        if not cands:
            cands = [t for t in old[0][1] if old[0][1].count(t) == 1]
        assert cands, [h[1] for h in old]
        tok = cands[0]
        eng.set_lm({(tok,): -20.0}, order=1, unk_logprob=0.0, weight=1.0)
        new = eng.transcribe_beam_mel([mels[13]], 4, 0, 3, lm=True)[0]
    finally:
        eng.close()
    print(f"the LM decides: token {tok}; old rank 0 {old[0][1]} score {old[0][0]:.4f}; new rank 0 {new[0][1]} score {new[0][0]:.4f} lm {new[0][4]:.1f}")
    assert tok in old[0][1] and tok not in new[0][1]
    assert new[0][0] <= old[0][0] and new[0][4] == 0.0 and new[0][5] == new[0][0]
    assert new[0][1] != old[0][1]


@pytest.mark.parametrize("dtype", [capi.DTYPE_F32, capi.DTYPE_BF16], ids=["f32", "bf16"])
def test_bit_identity_with_the_lm_on(W, lms, dtype):
    """5a: a ragged batch (T = 0 included, more rows than one sub-batch of 70) equals each utterance alone, LM values included"""
    mels = build_mels()
    order = [13, 5, 0, 1, 13, 13, 5, 13, 13, 13, 1]
    group = [mels[T] for T in order]
    full = lambda hyps: [(h[0], h[1], h[2], h[3].tobytes(), h[4], h[5], h[6].tobytes()) for h in hyps]
    eng = capi.Engine(W, n_layers=2, dtype=dtype, max_streams=1)
    try:
        for (Wd, S), which, weight, bonus in (((4, 3), "plain", LM_WEIGHT, 0.0), ((8, 2), "pos", 0.5, 0.25)):
            eng.set_lm(lms[which], order=3, unk_logprob=LM_UNK, weight=weight, token_bonus=bonus)
            alone = {T: full(eng.transcribe_beam_mel([mels[T]], Wd, 0, S, lm=True)[0]) for T in CASE_T}
            batch = eng.transcribe_beam_mel(group, Wd, 0, S, lm=True)
            eng.set_option("offline_rows", 70)
            cut = eng.transcribe_beam_mel(group, Wd, 0, S, lm=True)
            eng.set_option("offline_rows", 16384)
            for i, T in enumerate(order):
                assert full(batch[i]) == alone[T] and full(cut[i]) == alone[T], (Wd, S, i, T)
            part = eng.transcribe_beam_mel([mels[13]], Wd, 2, S, lm=True)[0]
            assert full(part) == alone[13][:2]
            eng.set_lm_weights(weight, bonus)                                   # the same weights again: the same bits
            assert full(eng.transcribe_beam_mel([mels[13]], Wd, 0, S, lm=True)[0]) == alone[13]
    finally:
        eng.close()


def test_transcription_and_live_streams_never_see_the_lm(W, lms):
    """5b: transcribe_mel and a live stream give the same bits before set_lm, while attached and after detaching"""
    mels = build_mels()
    group = [mels[T] for T in CASE_T]
    rng = np.random.default_rng(9)
    pcm = (rng.standard_normal(16000 * 2) * 3000).astype(np.int16)

    def run(with_lm):
        eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=2)
        try:
            s = eng.stream(right_context=1)
            out = eng.step([s], [pcm[:16000]])[0]
            first = eng.transcribe_mel(group)
            if with_lm:
                eng.set_lm(lms["plain"], order=3, unk_logprob=LM_UNK, weight=2.0, token_bonus=1.0)
                eng.transcribe_beam_mel(group, 4, 0, 3)
            second = eng.transcribe_mel(group)
            out += eng.step([s], [pcm[16000:24000]])[0]
            if with_lm:
                eng.set_lm(None)
            third = eng.transcribe_mel(group)
            out += eng.step([s], [pcm[24000:]])[0]
            out += eng.finalize([s])[0]
            return out, first, second, third, s.tap(capi.TAP_DEC_STATE).tobytes()
        finally:
            eng.close()

    a, b = run(False), run(True)
    assert a[1] == a[2] == a[3] == b[1] == b[2] == b[3]
    assert a[0] == b[0] and a[4] == b[4] and len(a[0]) >= 3


def test_errors_and_limits(W, lms):
    """6: each validity failure, a weight out of range, the LM getter after an LM-free call; the engine stays usable and the previous model in force"""
    mels = build_mels()
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    full = lambda hyps: [(h[0], h[1], h[4], h[5]) for h in hyps]
    try:
        good = [mels[5], mels[13]]
        eng.transcribe_beam_mel(good, 2, 0, 3)
        with pytest.raises(capi.NasrError, match="without a language model"):
            eng.beam_hypothesis_lm(0, 0)
        with pytest.raises(capi.NasrError, match="no language model"):
            eng.set_lm_weights(1.0, 0.0)
        eng.set_lm(lms["plain"], order=3, unk_logprob=LM_UNK, weight=LM_WEIGHT)
        base = full(eng.transcribe_beam_mel(good, 2, 0, 3, lm=True)[1])
        ok = [((5,), -1.0, -0.5), ((6,), -1.5, 0.0), ((5, 6), -0.5, 0.0)]
        bad = [(ok + [((5, 6), -0.25, 0.0)], 2, "duplicate"), (ok + [((5, 6, 5), -0.25, 0.0)], 2, "length"), (ok + [((5, 1024), -0.25, 0.0)], 2, "out of place"),
               (ok + [((5, BOS), -0.25, 0.0)], 2, "out of place"), (ok + [((EOS, 5), -0.25, 0.0)], 2, "out of place"), (ok + [((7,), float("nan"), 0.0)], 2, "finite"),
               (ok + [((7,), 0.5, 0.0)], 2, "<= 0"), (ok + [((7,), -0.5, float("inf"))], 2, "finite"), (ok + [((9, 6), -0.25, 0.0)], 2, "context"), (ok, 6, "order")]
        for items, order, msg in bad:
            with pytest.raises(capi.NasrError, match=msg):
                eng.set_lm(items, order=order, unk_logprob=-5.0, weight=1.0)
            assert eng.counter("lm_ngrams") == len(lms["plain"])                           # the previous model stays in force
        for kw in (dict(weight=-0.5), dict(weight=100.5), dict(weight=float("nan")), dict(token_bonus=-1.0), dict(token_bonus=101.0)):
            with pytest.raises(capi.NasrError, match="weight"):
                eng.set_lm(ok, order=2, unk_logprob=-5.0, **kw)
            with pytest.raises(capi.NasrError, match="weight"):
                eng.set_lm_weights(kw.get("weight", 1.0), kw.get("token_bonus", 0.0))
        with pytest.raises(capi.NasrError, match="unk"):
            eng.set_lm(ok, order=2, unk_logprob=0.5)
        assert full(eng.transcribe_beam_mel(good, 2, 0, 3, lm=True)[1]) == base            # usable, same model, same weights
        for u, rank in ((2, 0), (-1, 0), (0, 9), (0, -1)):
            with pytest.raises(capi.NasrError):
                eng.beam_hypothesis_lm(u, rank)
        n = capi.lib().nasr_engine_beam_hypothesis_lm(eng.h, 1, 0, None, None, None, 0)
        assert n == len(eng.beam_hypothesis(1, 0)[1])                                      # cap 0 returns the count
        eng.transcribe_mel(good)
        with pytest.raises(capi.NasrError, match="no beam hypotheses"):
            eng.beam_hypothesis_lm(0, 0)
        eng.set_lm(ok, order=2, unk_logprob=-5.0, weight=1.0)                               # a smaller model replaces the larger one
        assert [eng.counter(n) for n in ("lm_ngrams", "lm_states")] == [3, 3]
        eng.transcribe_beam_mel(good, 4, 0, 3, lm=True)
        eng.set_lm_weights(0.25, 0.0)                                                       # new weights leave the read-out of the last call alone ...
        assert len(eng.beam_hypothesis_lm(0, 0)[2]) == len(eng.beam_hypothesis(0, 0)[1])
        eng.set_lm(ok, order=2, unk_logprob=-4.0, weight=1.0)                               # ... another model ends it: no values of two models mixed
        with pytest.raises(capi.NasrError, match="replaced"):
            eng.beam_hypothesis_lm(0, 0)
        assert eng.beam_hypothesis(0, 0)[1] is not None
        eng.transcribe_beam_mel(good, 4, 0, 3, lm=True)
    finally:
        eng.close()


def test_cli_with_an_arpa_file(tmp_path, W):
    """7: nemotron-transcribe-amd --beam --lm on the golden ARPA file: the lines gain the LM log-probability and the total after the score
    and agree with the ABI given the same model; without --lm the output is what it was"""
    vocab = gguf_io.synthetic_vocab()
    model = tmp_path / "model.gguf"
    gguf_io.write_gguf(model, W, gguf_io.default_hparams(n_layers=2), vocab)
    pcm = synth.make_pcm(2, 3.0)
    audio = tmp_path / "a.pcm"
    pcm.tofile(audio)
    ln10 = math.log(10.0)
    c = lambda x: float(np.float32(float(np.float32(x)) * ln10))
    g = {(BOS,): (c(-99), c(-0.30103)), (EOS,): (c(-1.0), 0.0), (0,): (c(-0.5), c(-0.25)), (1,): (c(-0.75), c(-0.125)), (3,): (c(-1.25), c(0.0625)),
         (700,): (c(-1.5), c(-0.5)), (BOS, 0): (c(-0.25), c(-0.125)), (0, 1): (c(-0.5), c(-0.25)), (1, EOS): (c(-0.625), 0.0), (3, 700): (c(-0.875), 0.0),
         (1, 3): (c(-0.375), c(0.03125)), (BOS, 0, 1): (c(-0.125), 0.0), (0, 1, EOS): (c(-0.0625), 0.0), (0, 1, 3): (c(-0.1875), 0.0)}
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=1)
    try:
        free = eng.transcribe_beam([pcm], 4, 3, 3)[0]
        eng.set_lm(g, order=3, unk_logprob=c(-2.5), weight=0.75, token_bonus=0.5)
        hyps = eng.transcribe_beam([pcm], 4, 3, 3, lm=True)[0]
    finally:
        eng.close()
    exe = str(BIN / "nemotron-transcribe-amd")
    base = [exe, str(model), str(audio), "--f32", "--beam", "4", "--nbest", "3", "--max-symbols", "3", "--print-tokens"]
    r = subprocess.run(base + ["--lm", str(GOLDEN / "lm_tiny.arpa"), "--lm-weight", "0.75", "--token-bonus", "0.5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    lines = r.stdout.strip().splitlines()
    rows = [ln.split(None, 4) for ln in lines if ln.split()[0] not in ("tokens", "frames")]
    toks = [[int(x) for x in ln.split()[1:]] for ln in lines if ln.split()[0] == "tokens"]
    assert len(rows) == len(hyps) == 3 and [int(row[0]) for row in rows] == [0, 1, 2]
    assert toks == [h[1] for h in hyps]
    for row, h in zip(rows, hyps):
        assert float(row[1]) == pytest.approx(h[0], abs=1e-5) and float(row[2]) == pytest.approx(h[4], abs=1e-5) and float(row[3]) == pytest.approx(h[5], abs=1e-5)
    totals = [float(row[3]) for row in rows]
    assert all(a >= b for a, b in zip(totals, totals[1:]))
    r = subprocess.run(base, capture_output=True, text=True, timeout=120)                    # without --lm: rank score text, as before
    assert r.returncode == 0, r.stderr[-800:]
    lines = r.stdout.strip().splitlines()
    rows = [ln.split(None, 2) for ln in lines if ln.split()[0] not in ("tokens", "frames")]
    assert [[int(x) for x in ln.split()[1:]] for ln in lines if ln.split()[0] == "tokens"] == [h[1] for h in free]
    for row, h in zip(rows, free):
        assert float(row[1]) == pytest.approx(h[0], abs=1e-5)
    for bad in (["--lm", str(GOLDEN / "lm_tiny.arpa")], ["--beam", "2", "--lm-weight", "1"], ["--beam", "2", "--lm", str(tmp_path / "missing.arpa")]):
        r = subprocess.run([exe, str(model), str(audio), "--f32"] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and r.stderr.strip()
