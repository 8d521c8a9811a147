"""Frame-synchronous beam search with N-best hypotheses (nasr_engine_transcribe_beam_mel / _beam / _beam_hypothesis), on the MI355X.

The set-up is that of tests/test_gpu_align.py: a 2-layer engine per dtype, the same sharpened synthetic weights (GAIN = 30) and
LP_BOUND = 2e-4, the project's bound for this joint arithmetic at this gain.  Utterances of T = 0, 1, 5, 13 encoder frames; settings
(W, S) = (1, 10), (2, 3), (4, 3), (8, 2).

Invariants (any correct search satisfies them, no reference search needed): every hypothesis is re-scored on the engine's own lattice
(align_mel + align_lattice of the returned transcript) and on the float64 lattice of tests/align_ref.py from the engine's encoder rows: its
score is the score of the path at its reported frames within (T + U + 1) * LP_BOUND and is at most `best` plus that bound, every token's
ln P is within LP_BOUND of its lattice cell, frames are non-decreasing in [0, T) with at most S on one frame, hypotheses are distinct and
sorted.  Equality with tests/beam_ref.py (float64, on the oracle's decoder + joint over the engine's encoder rows) is asked only where the
reference's smallest decision margin exceeds 2 * (T + U + 1) * LP_BOUND; every pair with W <= 2 must qualify and at most a quarter of all
pairs may be left out.  Frames are compared where the smallest merge gap exceeds the threshold too (a merge decides frames, not tokens).
A deliberate extension of that rule, which can only remove comparisons: a pair whose reference met an expansion list cut closer than
2 * LP_BOUND is left out as well.  The margin above never sees that decision (for W = 1, D has no dropped candidate at all), yet an engine
within its bound may take the other output there.  The two outputs on either side of the cut are values of one cell under one parent score,
so their difference carries twice the cell bound and nothing of the path's length.  The W <= 2 and one-quarter conditions hold over both
criteria together, and the test prints how many pairs this criterion alone left out.

Every figure is printed before it is asserted (run with -s); profiles/beam_search.md records them."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi, gguf_io, synth
from oracle import binding as ob
from tests import align_ref as ar
from tests import beam_ref as br
from tests import offline_ref as orf

pytestmark = pytest.mark.gpu

BLANK, V = 1024, 1025
LP_BOUND = 2e-4
GAIN = 30.0
CASE_T = (0, 1, 5, 13)
SETTINGS = ((1, 10), (2, 3), (4, 3), (8, 2))
SEED = 12
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


@pytest.fixture(scope="module")
def W():
    return sharpened(synth.make_weights(n_layers=2), GAIN)


def rescore(eng, mels, hyps_of):
    """the engine's own lattice of every hypothesis: one ragged align call; -> {key: (loglik, best, frames, lps, lb, ly)}"""
    keys = [(k, r) for k, hyps in hyps_of.items() for r in range(len(hyps))]
    res = eng.align_mel([mels[k] for k, r in keys], [hyps_of[k][r][1] for k, r in keys])
    out = {}
    for u, (k, r) in enumerate(keys):
        lb, ly = eng.align_lattice(u, len(hyps_of[k][r][1]))
        out[(k, r)] = res[u] + (lb, ly)
    return out


@pytest.fixture(scope="module", params=[capi.DTYPE_F32, capi.DTYPE_BF16], ids=["f32", "bf16"])
def world(request, W):
    """one engine per dtype: a ragged beam call per setting, the engine's own lattices of every hypothesis, the float64 lattices and the
    reference search from the engine's encoder rows -- computed once, shared by the tests below"""
    mels = build_mels()
    group = [mels[T] for T in CASE_T]
    eng = capi.Engine(W, n_layers=2, dtype=request.param, max_streams=1)
    try:
        eng.set_debug(True)
        got, own = {}, {}
        for Wd, S in SETTINGS:
            res = eng.transcribe_beam_mel(group, beam=Wd, nbest=0, max_symbols=S)
            if (Wd, S) == SETTINGS[0]:
                enc = {T: eng.offline_tap(capi.TAP_ENCODER_OUT, i) for i, T in enumerate(CASE_T)}      # the tap works after a beam call
            got[(Wd, S)] = {T: res[i] for i, T in enumerate(CASE_T)}
        for st in SETTINGS:
            own[st] = rescore(eng, mels, {T: got[st][T] for T in CASE_T if T > 0})
    finally:
        eng.close()
    om = CachedOracle(ob.OracleModel(W, 2))
    ref_lat, ref = {}, {}
    for T in CASE_T:
        if T == 0:
            continue
        joint = br.OracleJoint(om, enc[T])
        for st in SETTINGS:
            ref[(st, T)] = br.search(joint, T, st[0], st[0], st[1])
            for r, h in enumerate(got[st][T]):
                ref_lat[(st, T, r)] = ar.lattice(om, enc[T], h[1])
    return dict(got=got, own=own, enc=enc, ref_lat=ref_lat, ref=ref)


def check_invariants(name, T, Wd, S, hyps, own_of, ref_lat_of):
    """item 1 of the module docstring for the hypotheses of one utterance; own_of(r) = the engine's align results + lattice of hypothesis r,
    ref_lat_of(r) = the float64 lattice or None"""
    assert 1 <= len(hyps) <= Wd, name
    assert len({tuple(h[1]) for h in hyps}) == len(hyps), name
    assert all(a[0] >= b[0] for a, b in zip(hyps, hyps[1:])), name
    worst_cell = worst_path = 0.0
    for r, (score, toks, frames, lps) in enumerate(hyps):
        U = len(toks)
        bound = (T + U + 1) * LP_BOUND
        assert len(frames) == U and lps.shape == (U,) and math.isfinite(score) and score <= 0.0, (name, r)
        assert all(0 <= t < BLANK for t in toks), (name, r)
        assert all(0 <= f < T for f in frames) and all(a <= b for a, b in zip(frames, frames[1:])), (name, r)
        assert U == 0 or max(np.bincount(frames)) <= S, (name, r)
        loglik, best, _, _, lb, ly = own_of(r)
        lattices = [("engine", lb.astype(np.float64), ly.astype(np.float64), best)]
        if ref_lat_of(r) is not None:
            rb, ry = ref_lat_of(r)
            lattices.append(("float64", rb, ry, ar.recursions(rb, ry)["best"]))
        for what, b_, y_, best_ in lattices:
            path = ar.path_score(b_, y_, frames)
            cell = max((abs(float(lps[i]) - float(y_[f, i])) for i, f in enumerate(frames)), default=0.0)
            worst_cell, worst_path = max(worst_cell, cell), max(worst_path, abs(score - path) / bound)
            assert abs(score - path) <= bound, (name, r, what, score, path)
            assert score <= best_ + bound, (name, r, what, score, best_)
            assert cell <= LP_BOUND, (name, r, what, cell)
    print(f"beam {name}: {len(hyps)} hypotheses, lengths {[len(h[1]) for h in hyps]}, worst |lp - cell| {worst_cell:.3e}, worst |score - path| / bound {worst_path:.3f}")


def test_invariants_of_every_hypothesis(world):
    n = 0
    for (Wd, S) in SETTINGS:
        for T in CASE_T:
            hyps = world["got"][(Wd, S)][T]
            if T == 0:
                assert len(hyps) == 1 and hyps[0][:3] == (0.0, [], []) and hyps[0][3].size == 0
                continue
            check_invariants(f"W{Wd}-S{S}-T{T}", T, Wd, S, hyps, lambda r: world["own"][(Wd, S)][(T, r)], lambda r: world["ref_lat"][((Wd, S), T, r)])
            n += len(hyps)
    assert n >= 30
    assert any(len(h[1]) > T for st in SETTINGS for T in CASE_T if T > 0 for h in world["got"][st][T]), "U > T: several symbols fall on a frame"


def test_equality_with_the_reference_where_its_margins_allow(world):
    pairs = left_out = frames_skipped = by_cut_alone = 0
    for (Wd, S) in SETTINGS:
        for T in CASE_T:
            if T == 0:
                continue
            hyps, (ref, stats) = world["got"][(Wd, S)][T], world["ref"][((Wd, S), T)]
            U = max(len(h["tokens"]) for h in ref)
            bound = (T + U + 1) * LP_BOUND
            ratio, mratio = stats["margin"] / (2 * bound), stats["merge_margin"] / (2 * bound)
            print(f"beam W{Wd}-S{S}-T{T}: margin / threshold {ratio:.2f}, merge gap / threshold {mratio:.2f}, expansion cut / (2 LP_BOUND) "
                  f"{stats['expand_margin'] / (2 * LP_BOUND):.1f}, reference lengths {[len(h['tokens']) for h in ref]}")
            pairs += 1
            if not (stats["margin"] > 2 * bound and stats["expand_margin"] > 2 * LP_BOUND):
                assert Wd > 2, f"W = {Wd}, T = {T} does not qualify (margin {stats['margin']:.3e}, cut {stats['expand_margin']:.3e}): change the seed, not the threshold"
                left_out += 1
                by_cut_alone += 1 if stats["margin"] > 2 * bound else 0
                continue
            assert [h[1] for h in hyps] == [h["tokens"] for h in ref], (Wd, S, T)
            for h, g in zip(hyps, ref):
                assert abs(h[0] - g["score"]) <= bound, (Wd, S, T)
            if stats["merge_margin"] > 2 * bound:
                assert [h[2] for h in hyps] == [h["frames"] for h in ref], (Wd, S, T)
            else:
                frames_skipped += 1
    print(f"beam: {pairs} pairs, {left_out} left out ({by_cut_alone} of them by the expansion cut alone), frames not compared in {frames_skipped}")
    assert pairs == 12 and left_out * 4 <= pairs


def _key(hyps):
    return [(h[0], h[1], h[2], h[3].tobytes()) for h in hyps]


@pytest.mark.parametrize("dtype", [capi.DTYPE_F32, capi.DTYPE_BF16], ids=["f32", "bf16"])
def test_bit_identity(W, dtype):
    """a ragged batch (T = 0 included) equals each utterance alone, with offline_rows at its default and at 70 (several sub-batches);
    nbest = k gives the first k of nbest = W; two identical calls agree"""
    mels = build_mels()
    order = [13, 5, 0, 1, 13, 13, 5, 13, 13, 13, 1]                          # 94 rows: more than one sub-batch of 70
    group = [mels[T] for T in order]
    eng = capi.Engine(W, n_layers=2, dtype=dtype, max_streams=1)
    try:
        for Wd, S in ((4, 3), (8, 2), (1, 10)):
            alone = {T: _key(eng.transcribe_beam_mel([mels[T]], Wd, 0, S)[0]) for T in CASE_T}
            batch = eng.transcribe_beam_mel(group, Wd, 0, S)
            again = eng.transcribe_beam_mel(group, Wd, 0, S)
            eng.set_option("offline_rows", 70)
            cut = eng.transcribe_beam_mel(group, Wd, 0, S)
            eng.set_option("offline_rows", 16384)                             # the default
            for i, T in enumerate(order):
                assert _key(batch[i]) == alone[T], (Wd, S, i, T)
                assert _key(again[i]) == alone[T] and _key(cut[i]) == alone[T], (Wd, S, i, T)
            for k in range(1, Wd + 1):
                part = eng.transcribe_beam_mel([mels[13], mels[5]], Wd, k, S)
                assert _key(part[0]) == alone[13][:k] and _key(part[1]) == alone[5][:k], (Wd, S, k)
    finally:
        eng.close()


def test_an_utterance_longer_than_the_greedy_window(W):
    """about 300 frames (the greedy decode works in windows of 256) at (4, 3): the invariants against the engine's own lattice (the float64
    lattice of 300 frames x hundreds of label positions would take minutes, so it is left to the short cases)"""
    rng = np.random.default_rng(SEED + 1)
    mel = mel_for(300, rng)
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    try:
        eng.set_debug(True)
        hyps = eng.transcribe_beam_mel([mel], 4, 0, 3)[0]
        own = rescore(eng, {300: mel}, {300: hyps})
    finally:
        eng.close()
    assert any(len(h[1]) >= 10 and max(h[2]) >= 256 for h in hyps)
    check_invariants("W4-S3-T300", 300, 4, 3, hyps, lambda r: own[(300, r)], lambda r: None)


@pytest.mark.parametrize("opts", [(), (("token_logprobs", 1), ("token_alternatives", 4))], ids=["plain", "logprobs+alternatives"])
def test_transcription_and_live_streams_are_untouched(W, opts):
    mels = build_mels()
    group = [mels[T] for T in CASE_T]
    rng = np.random.default_rng(9)
    pcm = (rng.standard_normal(16000 * 2) * 3000).astype(np.int16)

    def run(beam):
        eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=2)
        try:
            for k, v in opts:
                eng.set_option(k, v)
            s = eng.stream(right_context=1)
            out = eng.step([s], [pcm[:16000]])[0]
            first = eng.transcribe_mel(group)
            extra = [eng.offline_token_logprobs(u).tobytes() for u in range(len(group))] if opts else []
            if beam:
                eng.transcribe_beam_mel(group, 4, 0, 3)
                eng.transcribe_beam_mel([mels[13]], 8, 2, 2)
            out += eng.step([s], [pcm[16000:]])[0]
            second = eng.transcribe_mel(group)
            extra += [eng.offline_token_logprobs(u).tobytes() for u in range(len(group))] if opts else []
            out += eng.finalize([s])[0]
            return out, first, second, s.tap(capi.TAP_DEC_STATE).tobytes(), s.tap(capi.TAP_K_CACHE, 1).tobytes(), extra
        finally:
            eng.close()

    a, b = run(False), run(True)
    assert b[1] == b[2] == a[1] == a[2]
    assert a[0] == b[0] and a[3] == b[3] and a[4] == b[4] and a[5] == b[5]
    assert len(a[0]) >= 3


def test_errors_and_limits(W):
    mels = build_mels()
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    L = capi.lib()
    try:
        good = [mels[5], mels[13]]
        base = _key(eng.transcribe_beam_mel(good, 2, 0, 3)[1])
        for kw, msg in ((dict(beam=0), "beam"), (dict(beam=9), "beam"), (dict(beam=2, nbest=3), "nbest"), (dict(beam=2, max_symbols=11), "max_symbols"),
                        (dict(beam=2, flags=capi.FLAG_NO_SYNC), "NO_SYNC")):
            with pytest.raises(capi.NasrError, match=msg):
                eng.transcribe_beam_mel(good, **kw)
            with pytest.raises(capi.NasrError, match="no beam hypotheses"):                 # every beam call forgets the call before, a refused one too
                eng.beam_hypothesis(0, 0)
            assert _key(eng.transcribe_beam_mel(good, 2, 0, 3)[1]) == base                  # the engine stays usable
        assert orf.enc_frames(8 * 2048) == 2049
        with pytest.raises(capi.NasrError, match="2048"):
            eng.transcribe_beam_mel([mels[5], np.zeros((8 * 2048, 128), np.float32)], 2)
        with pytest.raises(capi.NasrError, match="no beam hypotheses"):                     # a failed call leaves none
            eng.beam_hypothesis(0, 0)
        res = eng.transcribe_beam_mel(good, 2, 0, 3)
        assert _key(res[1]) == base
        # the getter
        n = L.nasr_engine_beam_hypothesis(eng.h, 1, 0, None, None, None, 0, None)
        assert n == len(res[1][0][1])                                                       # cap 0 returns the count
        for u, rank in ((2, 0), (-1, 0), (0, len(res[0])), (0, -1)):
            with pytest.raises(capi.NasrError):
                eng.beam_hypothesis(u, rank)
        eng.transcribe_mel(good)                                                            # every offline call forgets them
        with pytest.raises(capi.NasrError, match="no beam hypotheses"):
            eng.beam_hypothesis(0, 0)
        # the PCM entry is the mel entry behind the device preprocessor
        pcm = synth.make_pcm(5, 1.5)
        eng.set_debug(True)
        a = eng.transcribe_beam([pcm], 4, 2, 3)[0]
        mel = eng.offline_tap(capi.TAP_MEL, 0)
        assert _key(eng.transcribe_beam_mel([mel], 4, 2, 3)[0]) == _key(a) and len(a) == 2
        dev = [(eng.upload(pcm), pcm.size)]
        assert _key(eng.transcribe_beam(dev, 4, 2, 3, flags=capi.FLAG_PCM_DEVICE)[0]) == _key(a)
    finally:
        eng.close()


def test_cli_prints_the_n_best(tmp_path, W):
    """nemotron-transcribe-amd on a synthetic GGUF and a short PCM: N lines with scores descending, line 1 the ABI's rank 0"""
    vocab = gguf_io.synthetic_vocab()
    model = tmp_path / "model.gguf"
    gguf_io.write_gguf(model, W, gguf_io.default_hparams(n_layers=2), vocab)
    pcm = synth.make_pcm(2, 3.0)
    audio = tmp_path / "a.pcm"
    pcm.tofile(audio)
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=1)
    try:
        hyps = eng.transcribe_beam([pcm], 4, 3, 3)[0]
        greedy = eng.transcribe([pcm])[0][0]
    finally:
        eng.close()
    exe = str(BIN / "nemotron-transcribe-amd")
    r = subprocess.run([exe, str(model), str(audio), "--f32", "--beam", "4", "--nbest", "3", "--max-symbols", "3", "--print-tokens"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    lines = r.stdout.strip().splitlines()
    rows = [ln.split(None, 2) for ln in lines if ln.split()[0] not in ("tokens", "frames")]
    toks = [[int(x) for x in ln.split()[1:]] for ln in lines if ln.split()[0] == "tokens"]
    frames = [[int(x) for x in ln.split()[1:]] for ln in lines if ln.split()[0] == "frames"]
    assert len(rows) == len(hyps) == 3 and [int(row[0]) for row in rows] == [0, 1, 2]
    scores = [float(row[1]) for row in rows]
    assert all(a >= b for a, b in zip(scores, scores[1:]))
    assert scores[0] == pytest.approx(hyps[0][0], abs=1e-5) and toks[0] == hyps[0][1] and frames[0] == hyps[0][2]
    assert [t for t in toks] == [h[1] for h in hyps]
    r = subprocess.run([exe, str(model), str(audio), "--f32", "--print-tokens"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    lines = r.stdout.strip().splitlines()
    assert [int(x) for x in [ln for ln in lines if ln.startswith("tokens")][0].split()[1:]] == greedy
