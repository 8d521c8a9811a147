"""N-gram LM shallow fusion in the device RNN-T greedy decode (engine option "lm_fusion"), live and offline, through the C ABI.

Reference: the greedy loop of tests/test_gpu_boost.py -- the oracle's decoder + joint (oracle.binding.OracleModel.decoder_joint) on the
engine's OWN encoder rows (NASR_TAP_ENCODER_OUT per one-chunk call, nasr_engine_offline_tap offline) of the f32 engine -- with the arg-max
taken over key = logits + (bonus_vector + lmbias), all f32, where bonus_vector is that file's slice-comparison definition of the phrase bonus
and lmbias(v) = (float)((double)weight * ln P(v | history) + (double)token_bonus) over tests/lm_ref.py (the recursive ARPA definition; the
history starts at BOS and gains every emitted token), 0 for blank, and 0 everywhere for a stream switched off or without a model.

No decision is left out of any comparison: every reference decode records its smallest top-1 minus top-2 margin of key and every
comparison asserts that it is at least MARGIN_MIN = 1e-3, the project's floor (30 x the 3.1e-5 engine / oracle logit agreement of
profiles/token_logprobs.md).  The seeds are those tests/test_gpu_boost.py picked for these shapes with the reference alone.

The models are built by the test from an UNFUSED reference decode (bigram_model): bigrams (a, x) with a an emitted token and x the runner-up
of the decision right after a, worth that decision's gap + 1, so x wins only through the state; and a unigram-only model over runner-ups of
frames that stayed blank (unigram_model).  unk = -20, weight 0.5 and token_bonus 10 make the bias of a token without n-grams exactly
0.5 * -20 + 10 = +0.0, so that only the chosen n-grams move a decision.

Measured on the MI355X (profiles/greedy_lm.md): smallest margin over all 54 reference decodes MEASURED_MIN_MARGIN = 6.4e-3 (16 x R = 13, the
unfused pass; fused 8.6e-3; offline 2.3e-2; the command line 2.7e-2; every 1 x R = 0 case 9.2e-3 and above); with "token_logprobs" the largest
|lp_engine - lp_reference| MEASURED_MAX_LP = 5.3e-5 (16 x R = 13, tiled kernel; 9.7e-6 at 1 x R = 0; bound 2e-4, the one of
tests/test_gpu_logprobs.py)."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi, gguf_io, synth
from oracle import binding as ob
from tests import lm_ref
from tests.test_gpu_boost import BIN, FRAMES_AFTER_CALL, LP_BOUND, MARGIN_MIN, SEEDS, W, bonus_vector, choose_phrases, drive, make_pcms, n_differences, om  # noqa: F401 (W, om: fixtures)

pytestmark = pytest.mark.gpu

BLANK, V, BOS = 1024, 1025, lm_ref.BOS
GOLDEN = Path(__file__).resolve().parent / "golden"
UNK, W_LM, B_LM = -20.0, 0.5, 10.0          # W_LM * UNK + B_LM == 0
MEASURED_MIN_MARGIN = 6.4e-3                # MI355X, see the docstring
MEASURED_MAX_LP = 5.3e-5
MARGINS = {}
_LM_CACHE = {}


def lm_vector(ref, hist, weight, bonus):
    """lmbias for every v at once: the definition, product and sum rounded on their own (Python floats), then f32"""
    ctx = tuple(hist)[-(ref.order - 1):] if ref.order > 1 else ()
    key = (id(ref), ctx, float(weight), float(bonus))
    if key not in _LM_CACHE:
        w, b = float(np.float32(weight)), float(np.float32(bonus))
        v = np.zeros(V, np.float32)
        for t in range(1024):
            v[t] = np.float32(w * ref.term(ctx, t) + b)
        _LM_CACHE[key] = v
    return _LM_CACHE[key]


class LmReplay:
    """the greedy loop of the reference (src/nemo-stream.cpp:840-930) with arg-max over logit + (phrase bonus + lmbias)"""

    def __init__(self, om, lm=None, weight=0.0, bonus=0.0, phrases=(), pbonus=(), lm_on=True, boost_on=True):
        self.om, self.h, self.c, self.prev = om, np.zeros(1280, np.float32), np.zeros(1280, np.float32), BLANK
        self.tokens, self.frames, self.lps, self.max_lps, self.n_frames, self.iterations = [], [], [], [], 0, 0
        self.min_margin, self.decisions, self.encs = math.inf, [], []
        self.phrases, self.pbonus, self.boost_on, self.bhist = [list(p) for p in phrases], [float(x) for x in pbonus], boost_on, []
        self.lm_on, self.weight, self.bonus = lm_on, weight, bonus
        self.set_lm(lm)

    def set_lm(self, lm, weight=None, bonus=None):
        """lm: (ngrams, order, unk) or None.  Like nasr_engine_set_lm the LM history restarts"""
        self.ref = lm_ref.RefLM(*lm) if lm else None
        if weight is not None:
            self.weight, self.bonus = weight, bonus
        self.restart_lm()

    def set_weights(self, weight, bonus):
        self.weight, self.bonus = weight, bonus                # the history stays
        self._bias()

    def restart_lm(self, on=None):
        if on is not None:
            self.lm_on = on
        self.lhist = (BOS,)
        self._bias()

    def _bias(self):
        bvec = bonus_vector(self.phrases, self.pbonus, self.bhist) if self.boost_on and self.phrases else np.zeros(V, np.float32)
        lvec = lm_vector(self.ref, self.lhist, self.weight, self.bonus) if self.lm_on and self.ref is not None else np.zeros(V, np.float32)
        self.bias = (bvec + lvec).astype(np.float32)            # the f32 sum the row holds

    def decode(self, enc):
        self.encs.append(np.array(enc, np.float32, copy=True))
        for row in np.asarray(enc, np.float32).reshape(-1, 1024):
            for _ in range(10):
                self.iterations += 1
                logits, hn, cn = self.om.decoder_joint(self.prev, self.h, self.c, row)
                key = logits + self.bias
                best = int(np.argmax(key))
                rest = key.copy()
                rest[best] = -np.inf
                margin = float(key[best]) - float(rest.max())
                self.min_margin = min(self.min_margin, margin)
                rest[BLANK] = -np.inf
                ru = int(np.argmax(rest))
                self.decisions.append(dict(frame=self.n_frames, best=best, margin=margin, ru=ru, ru_gap=float(key[best]) - float(rest[ru]), n_tok=len(self.tokens)))
                if best == BLANK:
                    break
                x = logits.astype(np.float64)
                lse = np.logaddexp.reduce(x)
                self.tokens.append(best)
                self.frames.append(self.n_frames)
                self.lps.append(float(x[best] - lse))
                self.max_lps.append(float(x.max() - lse))
                self.prev, self.h, self.c = best, hn, cn
                self.bhist.append(best)
                self.lhist = self.lhist + (best,)
                self._bias()
            self.n_frames += 1


def lp_for(bias):
    """the log-probability whose lmbias is `bias` under (W_LM, B_LM)"""
    assert bias <= B_LM - 1.0
    return (bias - B_LM) / W_LM


def bigram_model(reps, n=3, extra=1.0, start=False, min_frame=0):
    """from UNFUSED reference decodes: bigrams (a, x), a an emitted token, x the best other non-blank token of the decision right after a's
    emission, lmbias(x | a) = x's gap there + `extra` rounded to one decimal; a's unigram equals unk, so nothing but x moves.  start: also
    (BOS, x0) for the runner-up of the very first decision -- a model whose start state is not the empty context"""
    g = {}
    for rep in reps:
        D = rep.decisions
        emit = [i for i, d in enumerate(D) if d["best"] != BLANK and i + 1 < len(D) and d["frame"] >= min_frame]
        for i in emit[::max(len(emit) // n, 1)][:n]:
            a, nxt = D[i]["best"], D[i + 1]
            b = round(nxt["ru_gap"] + extra, 1)
            if nxt["ru"] != a and b <= B_LM - 1.0 and (a, nxt["ru"]) not in g:
                g[(a,)] = (UNK, 0.0)
                g[(a, nxt["ru"])] = (lp_for(b), 0.0)
        if start and D:
            b = round(D[0]["ru_gap"] + extra, 1)
            if b <= B_LM - 1.0:
                g[(BOS,)] = (-50.0, 0.0)
                g[(BOS, D[0]["ru"])] = (lp_for(b), 0.0)
    return g, 2, UNK


def unigram_model(reps, n=3, extra=1.0):
    """a unigram-only model: the runner-ups of the frames that stayed blank with the smallest gaps, each worth its gap + `extra`"""
    g = {}
    for rep in reps:
        for d in sorted((d for d in rep.decisions if d["best"] == BLANK), key=lambda d: d["ru_gap"])[:n]:
            b = round(d["ru_gap"] + extra, 1)
            if b <= B_LM - 1.0 and (d["ru"],) not in g:
                g[(d["ru"],)] = (lp_for(b), 0.0)
    return g, 1, UNK


def compare(toks, st, rep, what, frames=None):
    print(f"greedy_lm {what}: {len(rep.tokens)} tokens, {len(rep.decisions)} decisions, smallest margin {rep.min_margin:.3e}")
    MARGINS[what] = rep.min_margin
    assert rep.min_margin >= MARGIN_MIN, (what, rep.min_margin)                  # no near tie: every decision is compared
    assert toks == rep.tokens, what
    assert (st.token_frames() if frames is None else frames) == rep.frames, what
    if st is not None:
        assert st.stats().decode_iterations == rep.iterations, what


def attach(eng, lm, weight=W_LM, bonus=B_LM):
    eng.set_lm(lm[0], order=lm[1], unk_logprob=lm[2])
    eng.set_greedy_lm_weights(weight, bonus)


def fused_case(W, om, B, R, n_push, seed, choose_from, disabled=(), options=(), model=bigram_model, **model_kw):
    """pass A: option on, no model (must equal the unfused reference); the model is built from it; pass B on the same engine after
    nasr_engine_set_lm + the weights and a reset of every stream: every stream against its OWN single-stream reference, fused or (disabled) not"""
    pcms = make_pcms(B, R, n_push, seed)
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=B)
    eng.set_option("lm_fusion", 1)
    for k, v in options:
        eng.set_option(k, v)
    sts = [eng.stream(R) for _ in range(B)]
    plain = {b: [LmReplay(om)] for b in range(B)}
    toks_a = drive(eng, sts, pcms, R, plain)
    for b in range(B):
        compare(toks_a[b], sts[b], plain[b][0], f"{B} x R={R} seed {seed} no model, stream {b}")
    keep_a = dict(frames=[s.token_frames() for s in sts], fb=[s.frame_blank_logprobs() for s in sts] if dict(options).get("frame_blank_logprobs") else None)
    lm = model([plain[b][0] for b in choose_from], **model_kw)
    assert lm[0]
    attach(eng, lm)
    assert eng.counter("lm_ngrams") == len(lm[0])
    for b, s in enumerate(sts):
        s.reset()
        if b in disabled:
            s.set_lm(False)
    reps = {b: [LmReplay(om, lm, W_LM, B_LM, lm_on=b not in disabled)] for b in range(B)}
    toks_b = drive(eng, sts, pcms, R, reps)
    for b in range(B):
        compare(toks_b[b], sts[b], reps[b][0], f"{B} x R={R} seed {seed} fused, stream {b}{' (off)' if b in disabled else ''}")
        if b in disabled:
            assert toks_b[b] == toks_a[b] and sts[b].token_frames() == keep_a["frames"][b]
    return dict(eng=eng, sts=sts, pcms=pcms, lm=lm, plain={b: plain[b][0] for b in plain}, reps={b: reps[b][0] for b in reps}, toks_a=toks_a, toks_b=toks_b,
                frames_a=keep_a["frames"], fb_a=keep_a["fb"], frames_b=[s.token_frames() for s in sts])


def history_hits(case, streams):
    """positions where a bigram's x stands right after its a with the unfused tokens before it unchanged and something else (or nothing) there
    unfused: only the state made the difference"""
    hits = []
    for b in streams:
        ta, tb = case["toks_a"][b], case["toks_b"][b]
        for k in range(1, len(tb)):
            if (tb[k - 1], tb[k]) in case["lm"][0] and tb[:k] == ta[:k] and (ta + [BLANK])[k:k + 1] != [tb[k]]:
                hits.append((b, k))
    return hits


def assert_bites(case, streams, history=True):
    diffs = sum(n_differences(case["toks_a"][b], case["toks_b"][b]) for b in streams)
    hits = history_hits(case, streams)
    multi = max(int(np.bincount(case["frames_b"][b]).max()) if case["frames_b"][b] else 0 for b in streams)
    print(f"greedy_lm bite: {diffs} positions differ over streams {list(streams)}, {len(hits)} history-only decisions, up to {multi} symbols on one frame; model {case['lm'][0]}")
    assert diffs >= 1
    if history:
        assert hits and multi >= 2            # x follows a on a's own frame: that frame emits several symbols


# ---- the LM decides: the three kernel forms ----------------------------------------------------------------------------------------------
def test_lm_decides_small_joint_kernel(W, om):
    """1 stream x R = 0: one row per step, k_dec_joint.  The first bigram's x is emitted right after its a, on a's frame, where the unfused decode
    chose otherwise: only the history made the difference, and that frame emits several symbols"""
    case = fused_case(W, om, 1, 0, 30, SEEDS[(1, 0)], choose_from=(0,))
    assert_bites(case, (0,))
    case["eng"].close()


def test_unigram_only_model_and_a_start_state(W, om):
    """an order-1 model (no arcs at all: every lookup ends at the unigram), then on the same engine a model with BOS n-grams, whose start state is
    not the empty context: (BOS, x0) boosts x0 until the first emission only"""
    case = fused_case(W, om, 1, 0, 30, SEEDS[(1, 0)], choose_from=(0,), model=unigram_model)
    assert_bites(case, (0,), history=False)
    eng, st, plain = case["eng"], case["sts"][0], case["plain"][0]
    lm = bigram_model([plain], start=True)
    assert (BOS,) in lm[0] and any(k[0] == BOS and len(k) == 2 for k in lm[0])
    attach(eng, lm)
    st.reset()
    rep = LmReplay(om, lm, W_LM, B_LM)
    toks = drive(eng, [st], case["pcms"], 0, {0: [rep]})[0]
    compare(toks, st, rep, "model with start != 0")
    x0 = next(k[1] for k in lm[0] if k[0] == BOS and len(k) == 2)
    assert toks[0] == x0 and toks != case["toks_a"][0]         # the start state decided the first token
    case["eng"].close()


@pytest.fixture(scope="module")
def case16(W, om):
    opts = (("token_logprobs", 1), ("token_alternatives", 4), ("frame_blank_logprobs", 1))
    case = fused_case(W, om, 16, 13, 3, SEEDS[(16, 13)], choose_from=(0, 7), disabled=(3, 12), options=opts)
    yield case
    case["eng"].close()


def test_lm_decides_tiled_joint_kernel_16_streams(case16):
    """16 streams x R = 13 = 224 decode rows: k_dec_joint_tiled (with the LP + ALT + FB forms).  The streams emit in different iterations -- in most
    iterations only some of them do, and only those are refreshed -- and every one equals its own single-stream reference; streams 3 and 12 are
    switched off and equal the unfused run"""
    assert_bites(case16, [b for b in range(16) if b not in (3, 12)])
    per_stream = {b: len(case16["toks_b"][b]) for b in range(16)}
    assert len(set(per_stream.values())) > 1                   # the streams do not emit in step


def test_offline_three_utterances_and_the_flag(W, om):
    """nasr_engine_transcribe_mel: three utterances of different lengths, one without an encoder frame; NASR_FLAG_NO_LM = unfused; the beam and
    align entries reject the flag"""
    pp_args = (W["preprocessor.featurizer.fb"], W["preprocessor.featurizer.window"])
    mels = [ob.OraclePreproc(*pp_args).process(synth.make_pcm(330 + i, s)) for i, s in enumerate((5.0, 2.0))] + [np.zeros((0, 128), np.float32)]
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=1)
    eng.set_option("lm_fusion", 1)
    eng.set_debug(True)
    toks_a, frames_a = eng.transcribe_mel(mels)
    assert toks_a[2] == [] and len(toks_a[0]) >= 3
    encs = [eng.offline_tap(capi.TAP_ENCODER_OUT, u) for u in range(2)]
    plain = []
    for u in range(2):
        r = LmReplay(om)
        r.decode(encs[u])
        compare(toks_a[u], None, r, f"offline no model, utterance {u}", frames=frames_a[u])
        plain.append(r)
    lm = bigram_model(plain, n=4)
    attach(eng, lm)
    toks_b, frames_b = eng.transcribe_mel(mels)
    assert toks_b[2] == [] and frames_b[2] == []
    for u in range(2):
        r = LmReplay(om, lm, W_LM, B_LM)                       # every utterance starts at the model's start
        r.decode(eng.offline_tap(capi.TAP_ENCODER_OUT, u))
        compare(toks_b[u], None, r, f"offline fused, utterance {u}", frames=frames_b[u])
    assert toks_b[0] != toks_a[0] and toks_b[1] != toks_a[1]
    assert eng.transcribe_mel(mels, flags=capi.FLAG_NO_LM) == (toks_a, frames_a)
    assert eng.transcribe_mel(mels) == (toks_b, frames_b)
    with pytest.raises(capi.NasrError, match="NASR_FLAG_NO_LM"):
        eng.transcribe_beam_mel(mels, 2, flags=capi.FLAG_NO_LM)
    with pytest.raises(capi.NasrError, match="NASR_FLAG_NO_LM"):
        eng.align_mel(mels, [toks_a[0], toks_a[1], []], flags=capi.FLAG_NO_LM)
    st = eng.stream(0)
    with pytest.raises(capi.NasrError, match="NASR_FLAG_NO_LM"):
        eng.step([st], [np.zeros(1280, np.int16)], flags=capi.FLAG_NO_LM)
    assert eng.transcribe_mel(mels) == (toks_b, frames_b)      # the refusals changed nothing
    eng.close()


# ---- the state's life cycle --------------------------------------------------------------------------------------------------------------
def test_state_life_cycle(W, om):
    """R = 0, one frame per step.  Mid-stream: nasr_stream_set_lm off and on, nasr_engine_set_greedy_lm_weights (state kept) and nasr_engine_set_lm
    (state restarted) on an engine that has replayed step graphs -- no graph is rebuilt --, both reset modes, and destroy + create on the same slot"""
    R, n_push, seed = 0, 40, SEEDS[(1, 0)]
    pcms = make_pcms(1, R, n_push, seed)
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=1)
    eng.set_option("lm_fusion", 1)
    st = eng.stream(R)
    plain = LmReplay(om)
    toks0 = drive(eng, [st], pcms, R, {0: [plain]})[0]
    compare(toks0, st, plain, "life cycle: no model")
    lm, lm2 = bigram_model([plain], n=6, min_frame=4), unigram_model([plain], n=4)
    attach(eng, lm)
    st.reset()
    rep = LmReplay(om, lm, W_LM, B_LM)
    toks1 = drive(eng, [st], pcms, R, {0: [rep]})[0]
    compare(toks1, st, rep, "life cycle: fused")
    assert toks1 != toks0 and eng.counter("graph_replays") > 0
    shapes = eng.counter("graph_shapes")
    # the first decision only the history made: x at position k right after its a.  `call` is the step that decodes its frame, so a change made
    # right before that step is in force there, and with the fusion off x is not emitted at k
    fr1 = st.token_frames()
    k = next(i for i in range(1, len(toks1)) if (toks1[i - 1], toks1[i]) in lm[0] and toks1[:i] == toks0[:i] and (toks0 + [BLANK])[i] != toks1[i])
    call = next(ci for ci, nf in enumerate(FRAMES_AFTER_CALL) if nf > fr1[k])
    assert 1 <= call < n_push - 12
    # (a) switched off mid-stream, on again later: the state restarts both times
    st.reset()
    rep = LmReplay(om, lm, W_LM, B_LM)
    toks2 = drive(eng, [st], pcms, R, {0: [rep]}, events={call: lambda: (st.set_lm(False), rep.restart_lm(False)), call + 5: lambda: (st.set_lm(True), rep.restart_lm(True))})[0]
    compare(toks2, st, rep, "life cycle: set_lm off / on mid-stream")
    assert toks2[:k] == toks1[:k] and toks2[k:k + 1] != toks1[k:k + 1]
    # (b) new weights mid-stream (the state stays), then another model (the state restarts); the captured graphs are kept
    st.reset()
    rep = LmReplay(om, lm, W_LM, B_LM)
    toks3 = drive(eng, [st], pcms, R, {0: [rep]}, events={call: lambda: (eng.set_greedy_lm_weights(0.0, 0.0), rep.set_weights(0.0, 0.0)),
                                                          call + 3: lambda: (eng.set_greedy_lm_weights(W_LM, B_LM), rep.set_weights(W_LM, B_LM)),
                                                          call + 8: lambda: (eng.set_lm(lm2[0], order=lm2[1], unk_logprob=lm2[2]), rep.set_lm(lm2))})[0]
    compare(toks3, st, rep, "life cycle: weights, then model replaced mid-stream")
    assert toks3[:k] == toks1[:k] and toks3[k:k + 1] != toks1[k:k + 1] and eng.counter("graph_shapes") == shapes
    attach(eng, lm)
    # (c) nasr_stream_reset mid-stream, both modes: a fresh decode at the model's start
    for mode in (capi.RESET_FRESH, capi.RESET_REFERENCE):
        st.reset()
        box, first = [LmReplay(om, lm, W_LM, B_LM)], []
        reps = {0: [box[0]]}

        def do_reset():
            first.append((list(box[0].tokens), box[0].min_margin))
            st.reset(reference=mode == capi.RESET_REFERENCE)
            box[0] = LmReplay(om, lm, W_LM, B_LM)
            reps[0][0] = box[0]
        toks4 = drive(eng, [st], pcms, R, reps, events={call + 1: do_reset})[0]
        assert first[0][1] >= MARGIN_MIN and toks4[:len(first[0][0])] == first[0][0]
        compare(toks4[len(first[0][0]):], st, box[0], f"life cycle: nasr_stream_reset mode {mode} mid-stream")
    # (d) destroy, then create on the same slot: the new stream starts at the model's start with a fresh row
    st.destroy()
    st = eng.stream(R)
    rep = LmReplay(om, lm, W_LM, B_LM)
    toks5 = drive(eng, [st], pcms, R, {0: [rep]})[0]
    compare(toks5, st, rep, "life cycle: destroy + create on the slot")
    assert toks5 == toks1 and eng.counter("graph_shapes") == shapes
    # (e) detached: the unfused decode again
    eng.set_lm(None)
    st.reset()
    rep = LmReplay(om)
    compare(drive(eng, [st], pcms, R, {0: [rep]})[0], st, rep, "life cycle: detached")
    assert rep.tokens == toks0
    eng.close()


# ---- weight 0 / detached == option off, bit for bit ----------------------------------------------------------------------------------------
def run_engine(W, B, R, n_push, options, dtype, seed=500, setup=None, per_call=1):
    n = synth.shift_samples(R) * per_call
    pcms = [synth.make_pcm(seed + b, (n_push // per_call) * n / 16000 + 0.35) for b in range(B)]
    eng = capi.Engine(W, n_layers=2, dtype=dtype, max_streams=B)
    for k, v in options:
        eng.set_option(k, v)
    if setup:
        setup(eng)
    sts = [eng.stream(R) for _ in range(B)]
    toks = [[] for _ in range(B)]
    for o in range(0, pcms[0].size, n):
        for b, t in enumerate(eng.step(sts, [p[o:o + n] for p in pcms])):
            toks[b] += t
    for b, t in enumerate(eng.finalize(sts)):
        toks[b] += t
    opt = dict(options)
    res = dict(tokens=toks, frames=[s.token_frames() for s in sts], iterations=[s.stats().decode_iterations for s in sts],
               state=[s.tap(capi.TAP_DEC_STATE).tobytes() for s in sts],
               lps=[s.token_logprobs().tobytes() for s in sts] if opt.get("token_logprobs") else None,
               alts=[tuple(a.tobytes() for a in s.token_alternatives()) for s in sts] if opt.get("token_alternatives") else None,
               fb=[s.frame_blank_logprobs().tobytes() for s in sts] if opt.get("frame_blank_logprobs") else None,
               graph_replays=eng.counter("graph_replays"), pipelined=eng.counter("pipelined_steps"))
    eng.close()
    return res


SOME_LM = ({(5,): (-1.0, -0.5), (9,): (-2.0, 0.25), (5, 9): (-0.5, 0.0), (BOS,): (-30.0, -0.25), (BOS, 5): (-0.75, 0.0)}, 2, -7.0)


@pytest.mark.parametrize("B,R,n_push", [(1, 0, 24), (16, 13, 3)])
def test_weights_zero_and_detached_equal_the_option_off(W, B, R, n_push):
    """tokens, frames, iteration counts, decoder state, log-probs, alternatives and blank log-probs, bit for bit"""
    base = (("token_logprobs", 1), ("token_alternatives", 4), ("frame_blank_logprobs", 1))
    off = run_engine(W, B, R, n_push, base, capi.DTYPE_F32)
    assert sum(len(t) for t in off["tokens"]) >= 5 and off["graph_replays"] > 0
    detached = run_engine(W, B, R, n_push, base + (("lm_fusion", 1),), capi.DTYPE_F32, setup=lambda e: e.set_greedy_lm_weights(3.0, 2.0))
    zero = run_engine(W, B, R, n_push, base + (("lm_fusion", 1),), capi.DTYPE_F32, setup=lambda e: e.set_lm(SOME_LM[0], order=2, unk_logprob=SOME_LM[2], weight=0.7, token_bonus=0.3))
    for got in (detached, zero):
        assert got["graph_replays"] > 0
        for k in ("tokens", "frames", "iterations", "state", "lps", "alts", "fb"):
            assert got[k] == off[k], k


# ---- execution modes, bf16 -----------------------------------------------------------------------------------------------------------------
def test_execution_modes_agree_on_the_bf16_engine(W):
    """eager, graph replay, multi-chunk pushes and pipeline = 4 give the same tokens and frames; the model -- a bias of 6 for every fifth token and
    of 8 for the successor id after any of the unfused run's tokens -- changes the transcript"""
    B, R, n_push = 4, 13, 4
    off = run_engine(W, B, R, n_push, (), capi.DTYPE_BF16)
    g = {(t,): (lp_for(6.0), 0.0) for t in range(0, 1024, 5)}
    for t in sorted({t for ts in off["tokens"] for t in ts})[:40]:
        g.setdefault((t,), (UNK, 0.0))
        g[(t, (t + 1) % 1024)] = (lp_for(8.0), 0.0)
    on = (("lm_fusion", 1),)
    setup = lambda e: attach(e, (g, 2, UNK))
    base = run_engine(W, B, R, n_push, on, capi.DTYPE_BF16, setup=setup)
    assert base["graph_replays"] > 0 and base["tokens"] != off["tokens"]
    eager = run_engine(W, B, R, n_push, on + (("graph", 0),), capi.DTYPE_BF16, setup=setup)
    assert eager["graph_replays"] == 0
    multi = run_engine(W, B, R, n_push, on, capi.DTYPE_BF16, setup=setup, per_call=2)
    pipe = run_engine(W, B, R, n_push, on + (("pipeline", 4),), capi.DTYPE_BF16, setup=setup)
    assert pipe["pipelined"] > 0
    fold = run_engine(W, B, R, n_push, on + (("lm_refresh_fold", 0),), capi.DTYPE_BF16, setup=setup)      # the refresh as a launch of its own
    relook = run_engine(W, B, R, n_push, on + (("lm_commit_lookup", 1),), capi.DTYPE_BF16, setup=setup)      # the commit's second-lookup form
    assert relook["iterations"] == base["iterations"] and relook["state"] == base["state"]
    for what, got in (("eager", eager), ("multi-chunk", multi), ("pipeline 4", pipe), ("own refresh launch", fold), ("commit lookup", relook)):
        assert got["tokens"] == base["tokens"] and got["frames"] == base["frames"], what
    for got in (eager, pipe, fold):
        assert got["iterations"] == base["iterations"] and got["state"] == base["state"]


# ---- the probabilities stay the model's -------------------------------------------------------------------------------------------------------
def check_probabilities(case, streams, what):
    worst, below, total, own, same_frames = 0.0, 0, 0, 0, 0
    for b in streams:
        st, rep = case["sts"][b], case["reps"][b]
        lp = np.asarray(st.token_logprobs(), np.float32)
        assert lp.shape == (len(rep.tokens),) and np.isfinite(lp).all() and (lp <= 0).all()
        if lp.size:
            worst = max(worst, float(np.abs(lp.astype(np.float64) - np.asarray(rep.lps)).max()))
            below += int((lp < np.asarray(rep.max_lps) - 10 * LP_BOUND).sum())
            total += lp.size
            ids, alps = st.token_alternatives()
            for i, t in enumerate(rep.tokens):                 # the token's own entry, where it is among the K, equals its log-prob bit for bit
                at = np.nonzero(ids[i] == t)[0]
                if at.size:
                    assert alps[i][at[0]].tobytes() == lp[i].tobytes()
                    own += 1
        # frames the fused and the unfused decode went through with the same history: those before the frame of the first differing token
        ta, tb, fa, fb = case["toks_a"][b], case["toks_b"][b], case["frames_a"][b], case["frames_b"][b]
        k = next((i for i in range(min(len(ta), len(tb))) if (ta[i], fa[i]) != (tb[i], fb[i])), min(len(ta), len(tb)))
        got = st.frame_blank_logprobs()
        n_same = min(([fa[k]] if k < len(ta) else []) + ([fb[k]] if k < len(tb) else []) + [len(got)])
        assert got[:n_same].tobytes() == case["fb_a"][b][:n_same].tobytes()
        same_frames += n_same
    print(f"greedy_lm + token_logprobs {what}: {total} tokens, max |lp_engine - lp_reference| = {worst:.3e}, {below} values below their row's raw maximum, {own} own entries")
    MARGINS[f"lp {what}"] = worst
    assert total >= 5 and below >= 1 and own >= 1 and same_frames >= 1
    assert worst <= LP_BOUND, worst


def test_probabilities_stay_the_models_small_kernel(W, om):
    opts = (("token_logprobs", 1), ("token_alternatives", 4), ("frame_blank_logprobs", 1))
    case = fused_case(W, om, 1, 0, 30, SEEDS[(1, 0)], choose_from=(0,), options=opts, min_frame=4)      # the first frames keep the unfused history
    check_probabilities(case, (0,), "1 x R=0 (k_dec_joint)")
    case["eng"].close()


def test_probabilities_stay_the_models_tiled_kernel(case16):
    check_probabilities(case16, range(16), "16 x R=13 (k_dec_joint_tiled)")


# ---- with phrase boosting ------------------------------------------------------------------------------------------------------------------
def test_with_phrase_boost_the_sum_rule(W, om):
    """both options on: key = logit + (phrase bonus + lmbias).  The phrases are one-token runner-ups of blank frames, plus the first bigram's x with
    a bonus of 0.3 so that both terms are non-zero on one entry; each feature alone gives another transcript on the same rows"""
    R, seed = 0, SEEDS[(1, 0)]
    pcms = make_pcms(1, R, 30, seed)
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=1)
    eng.set_option("lm_fusion", 1)
    eng.set_option("phrase_boost", 64)
    st = eng.stream(R)
    plain = LmReplay(om)
    toks0 = drive(eng, [st], pcms, R, {0: [plain]})[0]
    compare(toks0, st, plain, "boost + lm: neither set")
    lm = bigram_model([plain])
    x = next(k[1] for k in lm[0] if len(k) == 2)
    chosen = [(p, w) for p, w in zip(*choose_phrases(plain, n_multi=1, n_single=2)) if len(p) == 1 and p != [x]]
    phrases, pbonus = [p for p, _ in chosen] + [[x]], [w for _, w in chosen] + [0.3]
    assert len(phrases) >= 2
    attach(eng, lm)
    eng.set_boost_phrases(phrases, pbonus)
    st.reset()
    both, lm_only, boost_only = LmReplay(om, lm, W_LM, B_LM, phrases, pbonus), LmReplay(om, lm, W_LM, B_LM), LmReplay(om, None, 0, 0, phrases, pbonus)
    toks = drive(eng, [st], pcms, R, {0: [both, lm_only, boost_only]})[0]
    compare(toks, st, both, "boost + lm: both")
    assert toks != lm_only.tokens and toks != boost_only.tokens and lm_only.tokens != toks0 and boost_only.tokens != toks0      # each decides its own case
    # a stream with boosting off keeps the LM, and the other way round
    st.reset()
    st.set_boost(False)
    rep = LmReplay(om, lm, W_LM, B_LM)
    compare(drive(eng, [st], pcms, R, {0: [rep]})[0], st, rep, "boost + lm: boost switched off")
    st.reset()
    st.set_boost(True)
    st.set_lm(False)
    rep = LmReplay(om, None, 0, 0, phrases, pbonus)
    compare(drive(eng, [st], pcms, R, {0: [rep]})[0], st, rep, "boost + lm: lm switched off")
    # the phrase set replaced with the LM in force: the rows follow
    eng.set_boost_phrases([], None)
    st.reset()
    st.set_lm(True)
    rep = LmReplay(om, lm, W_LM, B_LM)
    compare(drive(eng, [st], pcms, R, {0: [rep]})[0], st, rep, "boost + lm: phrases cleared")
    eng.close()


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def test_rejections(W):
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=1)
    st = eng.stream(0)
    with pytest.raises(capi.NasrError, match="lm_fusion"):
        eng.set_greedy_lm_weights(1.0, 0.0)                    # the option is off
    with pytest.raises(capi.NasrError, match="lm_fusion"):
        st.set_lm(False)
    with pytest.raises(capi.NasrError, match="lm_fusion must be 0 or 1"):
        eng.set_option("lm_fusion", 2)
    eng.set_option("lm_fusion", 1)
    for w, b in ((-0.1, 0.0), (100.5, 0.0), (1.0, -1.0), (1.0, 101.0), (float("nan"), 0.0), (1.0, float("inf"))):
        with pytest.raises(capi.NasrError, match=r"finite in \[0, 100\]"):
            eng.set_greedy_lm_weights(w, b)
    eng.set_greedy_lm_weights(100.0, 100.0)
    eng.set_greedy_lm_weights(0.0, 0.0)
    st.set_lm(False)
    st.set_lm(True)
    eng.step([st], [synth.make_pcm(3, 1.0)])
    with pytest.raises(capi.NasrError, match="before the first step"):
        eng.set_option("lm_fusion", 0)
    eng.close()
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=1)
    eng.transcribe([synth.make_pcm(1, 1.0)])
    with pytest.raises(capi.NasrError, match="before the first step or offline call"):
        eng.set_option("lm_fusion", 1)
    eng.close()


# ---- the beam search is untouched -----------------------------------------------------------------------------------------------------------
def test_beam_call_is_the_same_with_greedy_fusion_enabled(W):
    pp_args = (W["preprocessor.featurizer.fb"], W["preprocessor.featurizer.window"])
    mels = [ob.OraclePreproc(*pp_args).process(synth.make_pcm(40 + i, s)) for i, s in enumerate((2.5, 1.5))]

    def norm(h):
        return tuple(x.tobytes() if isinstance(x, np.ndarray) else tuple(x) if isinstance(x, list) else x for x in h)
    out = []
    for fusion in (0, 1):
        eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=1)
        if fusion:
            eng.set_option("lm_fusion", 1)
        eng.set_lm(SOME_LM[0], order=2, unk_logprob=SOME_LM[2], weight=0.6, token_bonus=0.2)
        if fusion:
            eng.set_greedy_lm_weights(2.0, 1.0)
            eng.transcribe_mel(mels)                           # a fused greedy call in between
        out.append([[norm(h) for h in hyps] for hyps in eng.transcribe_beam_mel(mels, 4, 3, 3, lm=True)])
        eng.close()
    assert out[0] == out[1] and all(len(h) >= 1 for h in out[0])


# ---- the command line -------------------------------------------------------------------------------------------------------------------------
def test_cli_lm_without_beam(tmp_path, W, om):
    """nemotron-transcribe-amd --lm (no --beam) on the golden ARPA file prints the transcript of the reference fused with the same model"""
    vocab = gguf_io.synthetic_vocab()
    model = tmp_path / "model.gguf"
    gguf_io.write_gguf(model, W, gguf_io.default_hparams(n_layers=2), vocab)
    pcm = synth.make_pcm(2, 3.0)
    audio = tmp_path / "a.pcm"
    pcm.tofile(audio)
    ln10 = math.log(10.0)
    c = lambda x: float(np.float32(float(np.float32(x)) * ln10))
    EOS = lm_ref.EOS                                            # tests/golden/lm_tiny.arpa, as tests/test_gpu_beam_lm.py restates it
    g = {(BOS,): (c(-99), c(-0.30103)), (EOS,): (c(-1.0), 0.0), (0,): (c(-0.5), c(-0.25)), (1,): (c(-0.75), c(-0.125)), (3,): (c(-1.25), c(0.0625)),
         (700,): (c(-1.5), c(-0.5)), (BOS, 0): (c(-0.25), c(-0.125)), (0, 1): (c(-0.5), c(-0.25)), (1, EOS): (c(-0.625), 0.0), (3, 700): (c(-0.875), 0.0),
         (1, 3): (c(-0.375), c(0.03125)), (BOS, 0, 1): (c(-0.125), 0.0), (0, 1, EOS): (c(-0.0625), 0.0), (0, 1, 3): (c(-0.1875), 0.0)}
    lm, weight, bonus = (g, 3, c(-2.5)), 2.0, 8.0
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=1)
    eng.set_debug(True)
    free = eng.transcribe([pcm])[0][0]
    rep = LmReplay(om, lm, weight, bonus)
    rep.decode(eng.offline_tap(capi.TAP_ENCODER_OUT, 0))
    eng.close()
    print(f"greedy_lm cli: smallest margin {rep.min_margin:.3e}")
    MARGINS["cli"] = rep.min_margin
    assert rep.min_margin >= MARGIN_MIN and rep.tokens != free
    exe = str(BIN / "nemotron-transcribe-amd")
    r = subprocess.run([exe, str(model), str(audio), "--f32", "--print-tokens", "--lm", str(GOLDEN / "lm_tiny.arpa"), "--lm-weight", str(weight), "--token-bonus", str(bonus)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    lines = r.stdout.strip().splitlines()
    assert [int(x) for x in next(ln for ln in lines if ln.startswith("tokens")).split()[1:]] == rep.tokens
    assert [int(x) for x in next(ln for ln in lines if ln.startswith("frames")).split()[1:]] == rep.frames
    r = subprocess.run([exe, str(model), str(audio), "--f32", "--print-tokens"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and [int(x) for x in next(ln for ln in r.stdout.splitlines() if ln.startswith("tokens")).split()[1:]] == free


def test_zz_report_margins():
    """not a check of its own: prints the figures of this module's run for profiles/greedy_lm.md"""
    margins = {k: v for k, v in MARGINS.items() if not k.startswith("lp ")}
    if margins:
        k = min(margins, key=margins.get)
        print(f"greedy_lm smallest reference margin over {len(margins)} reference decodes: {margins[k]:.3e} ({k})")
    for k, v in MARGINS.items():
        if k.startswith("lp "):
            print(f"greedy_lm {k}: max |lp_engine - lp_reference| = {v:.3e}")
