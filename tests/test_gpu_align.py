"""Forced alignment and transcript scoring on the RNN-T lattice (nasr_engine_align_mel / _align / _align_lattice), on the MI355X.

Reference (tests/align_ref.py): the engine's OWN encoder rows (offline_tap(TAP_ENCODER_OUT) after an align call with debug on) go to
the oracle's decoder + joint, teacher-forced over the transcript -- T * (U + 1) calls -- and the log-softmax and both recursions are
taken in float64.  That isolates the lattice, which is f32 in both engine dtypes, so one bound serves f32 and bf16 engines.

LP_BOUND = 2e-4 is the project's bound for this joint arithmetic at this gain (profiles/token_logprobs.md: measured 3.1e-5, x 4; the
sharpened checkpoint of tests/test_gpu_logprobs.py, restated here).  Every path sums T + U + 1 cell values and the recursions run in
double, so loglik and best are held to (T + U + 1) * LP_BOUND.  Frames are compared exactly: every case's smallest decision margin
along the reference's best path must exceed 2 * (T + U + 1) * LP_BOUND (asserted, none skipped).

Every figure is printed before it is asserted (run with -s); profiles/forced_alignment.md records them.  A measured cell deviation above
1e-4 would be a defect to explain, not a tolerance to raise (profiles/token_logprobs.md)."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi, gguf_io, synth
from oracle import binding as ob
from tests import align_ref as ar
from tests import offline_ref as orf

pytestmark = pytest.mark.gpu

BLANK, V = 1024, 1025
LP_BOUND = 2e-4
GAIN = 30.0
CASE_T = (1, 5, 13, 40)
SPECIAL = [0, 1023, 5, 5, 1023]             # ids 0 and 1023, a repeated id
BIN = Path(__file__).resolve().parent.parent / "nemotron-asr.cpp_amd" / "bin"


def mel_for(T, rng):
    """a log-mel of the fewest frames that give T encoder frames (the recipe of tests/test_gpu_offline.py)"""
    n = max(1, 8 * (T - 3))
    while orf.enc_frames(n) < T:
        n += 1
    assert orf.enc_frames(n) == T
    return rng.standard_normal((n, 128)).astype(np.float32)


def sharpened(W, gain):
    """the joint's output layer centred over the vocabulary and scaled (tests/test_gpu_logprobs.py: the near-tie checkpoint's logits are
    ~1e-3 apart, so every lp would sit near -ln 1025 and no Viterbi decision would have a margin)"""
    w = dict(W)
    wo = np.asarray(W["joint.joint_net.2.weight"], np.float64)
    bo = np.asarray(W["joint.joint_net.2.bias"], np.float64)
    w["joint.joint_net.2.weight"] = ((wo - wo.mean(axis=0, keepdims=True)) * gain).astype(np.float32)
    w["joint.joint_net.2.bias"] = ((bo - bo.mean()) * gain).astype(np.float32)
    return w


def build_mels():
    rng = np.random.default_rng(11)
    mels = {T: mel_for(T, rng) for T in CASE_T}
    mels["big"] = mel_for(40, rng)
    return mels


def build_cases(mels, greedy):
    """(name, mel, transcript): per T the utterance's own greedy tokens, a random transcript of min(T + 3, 9) ids, the empty one and one
    with ids 0, 1023 and a repeated id; then one lattice of several tiles in both directions (T = 40, U = 33)"""
    trng = np.random.default_rng(1711)
    cases = []
    for T in CASE_T:
        cases.append((f"T{T}-greedy", mels[T], [int(t) for t in greedy[T]]))
        cases.append((f"T{T}-random", mels[T], trng.integers(0, 1024, min(T + 3, 9)).tolist()))
        cases.append((f"T{T}-empty", mels[T], []))
        cases.append((f"T{T}-special", mels[T], list(SPECIAL)))
    cases.append(("T40-U33", mels["big"], trng.integers(0, 1024, 33).tolist()))
    return cases


@pytest.fixture(scope="module")
def W():
    return sharpened(synth.make_weights(n_layers=2), GAIN)


def run_align(eng, cases):
    res = eng.align_mel([c[1] for c in cases], [c[2] for c in cases])
    lat = [eng.align_lattice(u, len(c[2])) for u, c in enumerate(cases)]
    return res, lat


@pytest.fixture(scope="module", params=[capi.DTYPE_F32, capi.DTYPE_BF16], ids=["f32", "bf16"])
def world(request, W):
    """one engine per dtype: the greedy decode of the four utterances (with its token log-probabilities), one ragged align call over all
    cases, and the float64 reference of every case from the engine's own encoder rows -- computed once, shared by the tests below"""
    mels = build_mels()
    eng = capi.Engine(W, n_layers=2, dtype=request.param, max_streams=1)
    try:
        eng.set_option("token_logprobs", 1)
        eng.set_debug(True)
        toks, frames = eng.transcribe_mel([mels[T] for T in CASE_T])
        glp = [eng.offline_token_logprobs(u) for u in range(len(CASE_T))]
        greedy = {T: toks[i] for i, T in enumerate(CASE_T)}
        cases = build_cases(mels, greedy)
        res, lat = run_align(eng, cases)
        enc = [eng.offline_tap(capi.TAP_ENCODER_OUT, u) for u in range(len(cases))]
    finally:
        eng.close()
    om = ob.OracleModel(W, 2)
    ref_lat = [ar.lattice(om, enc[u], c[2]) for u, c in enumerate(cases)]
    ref = [ar.recursions(lb, ly) for lb, ly in ref_lat]
    return dict(cases=cases, res=res, lat=lat, ref_lat=ref_lat, ref=ref, greedy=greedy, greedy_frames={T: frames[i] for i, T in enumerate(CASE_T)},
                greedy_lp={T: glp[i] for i, T in enumerate(CASE_T)})


def test_shapes_of_the_cases(world):
    shapes = [(world["ref_lat"][u][0].shape[0], len(c[2])) for u, c in enumerate(world["cases"])]
    assert len(shapes) == 17 and len(set(shapes)) >= 12
    assert sum(1 for T, U in shapes if U > T) >= 4 and any(U > T > 1 for T, U in shapes), "U > T: several symbols fall on a frame"
    assert all(len(world["greedy"][T]) >= 3 for T in CASE_T)


def test_every_cell_against_the_float64_reference(world):
    worst = 0.0
    for u, (name, mel, y) in enumerate(world["cases"]):
        lb, ly = world["lat"][u]
        rb, ry = world["ref_lat"][u]
        U = len(y)
        assert lb.shape == rb.shape == ly.shape == (rb.shape[0], U + 1), name
        assert np.isneginf(ly[:, U]).all() and np.isfinite(ly[:, :U]).all() and np.isfinite(lb).all(), name
        assert (lb <= 0).all() and (ly[:, :U] <= 0).all(), name
        d = max(float(np.abs(lb - rb).max()), float(np.abs(ly[:, :U] - ry[:, :U]).max()) if U else 0.0)
        print(f"align {name}: T = {lb.shape[0]}, U = {U}, max |lp_engine - lp_reference| = {d:.3e}")
        worst = max(worst, d)
    print(f"align: max over every cell of every case = {worst:.3e}")
    assert worst <= LP_BOUND, worst


def test_loglik_and_best(world):
    for u, (name, mel, y) in enumerate(world["cases"]):
        loglik, best, frames, lps = world["res"][u]
        ref = world["ref"][u]
        T, U = world["ref_lat"][u][0].shape[0], len(y)
        bound = (T + U + 1) * LP_BOUND
        print(f"align {name}: loglik {loglik:.6f} (ref {ref['loglik']:.6f}), best {best:.6f} (ref {ref['best']:.6f}), bound {bound:.1e}")
        assert math.isfinite(loglik) and math.isfinite(best), name
        assert abs(loglik - ref["loglik"]) <= bound and abs(best - ref["best"]) <= bound, name
        assert loglik >= best, name
        if U == 0:
            col = 0.0                                                        # the sum of the blanks of column 0, frame after frame
            for x in world["lat"][u][0][:, 0]:
                col += float(x)
            assert loglik == best == col, name


def test_frames(world):
    for u, (name, mel, y) in enumerate(world["cases"]):
        loglik, best, frames, lps = world["res"][u]
        lb, ly = world["lat"][u]
        rb, ry = world["ref_lat"][u]
        ref = world["ref"][u]
        T, U = rb.shape[0], len(y)
        bound = (T + U + 1) * LP_BOUND
        assert len(frames) == U and lps.shape == (U,), name
        assert all(0 <= f < T for f in frames) and all(a <= b for a, b in zip(frames, frames[1:])), name
        for i, f in enumerate(frames):
            assert lps[i].tobytes() == ly[f, i].tobytes(), (name, i)          # bit for bit the engine's own lattice
        assert ar.path_score(rb, ry, frames) >= ref["best"] - 2 * bound, name
        print(f"align {name}: margin {ref['margin']:.3e}, threshold {2 * bound:.1e}")
        assert ref["margin"] > 2 * bound, (name, ref["margin"])              # every case qualifies
        assert frames == ref["frames"], name


def test_cross_check_with_token_logprobs(world):
    """the greedy path scored on the lattice of the greedy transcript: lp_token[f_i, i] is the decode's own token log-probability (both sit
    within LP_BOUND of the same oracle value), which pins the teacher-forced states to the decode's"""
    names = [c[0] for c in world["cases"]]
    n = 0
    for T in CASE_T:
        u = names.index(f"T{T}-greedy")
        lb, ly = world["lat"][u]
        f, lp = world["greedy_frames"][T], world["greedy_lp"][T]
        assert len(f) == len(lp) == ly.shape[1] - 1
        for i in range(len(f)):
            assert abs(float(ly[f[i], i]) - float(lp[i])) <= 2 * LP_BOUND, (T, i)
            n += 1
    assert n >= 20


def _same(a, b):
    return (a[0][0] == b[0][0] and a[0][1] == b[0][1] and a[0][2] == b[0][2] and a[0][3].tobytes() == b[0][3].tobytes()
            and a[1][0].tobytes() == b[1][0].tobytes() and a[1][1].tobytes() == b[1][1].tobytes())


@pytest.mark.parametrize("dtype", [capi.DTYPE_F32, capi.DTYPE_BF16], ids=["f32", "bf16"])
def test_batch_equals_alone_whatever_the_launch_cut(W, dtype):
    """a ragged batch of all cases equals each utterance alone, bit for bit (lattice, loglik, best, frames); the same with align_cells
    64 and 200 (several launches per lattice, launches over several lattices) and with offline_rows 70 (several sub-batches)"""
    mels = build_mels()
    eng = capi.Engine(W, n_layers=2, dtype=dtype, max_streams=1)
    try:
        eng.set_debug(True)
        toks, _ = eng.transcribe_mel([mels[T] for T in CASE_T])
        cases = build_cases(mels, {T: toks[i] for i, T in enumerate(CASE_T)})

        def batch():
            res, lat = run_align(eng, cases)
            return [(res[u], lat[u]) for u in range(len(cases))]

        alone = []
        for c in cases:
            res, lat = run_align(eng, [c])
            alone.append((res[0], lat[0]))
        runs = {"batch": batch()}
        with pytest.raises(capi.NasrError, match="align_cells"):
            eng.set_option("align_cells", 63)
        for cells in (64, 200):
            eng.set_option("align_cells", cells)
            runs[f"align_cells {cells}"] = batch()
        eng.set_option("align_cells", 1 << 20)
        eng.set_option("offline_rows", 70)
        runs["offline_rows 70"] = batch()
        for what, got in runs.items():
            for u, c in enumerate(cases):
                assert _same(got[u], alone[u]), (what, c[0])
    finally:
        eng.close()


def test_transcription_and_live_streams_are_untouched(W):
    mels = build_mels()
    group = [mels[T] for T in CASE_T]
    rng = np.random.default_rng(9)
    pcm = (rng.standard_normal(16000 * 2) * 3000).astype(np.int16)

    def run(align):
        eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=2)
        try:
            s = eng.stream(right_context=1)
            out = eng.step([s], [pcm[:16000]])[0]
            first = eng.transcribe_mel(group)
            if align:
                eng.align_mel(group, [first[0][i] for i in range(len(group))])
                eng.align_mel([mels["big"]], [SPECIAL])
            out += eng.step([s], [pcm[16000:]])[0]
            second = eng.transcribe_mel(group)
            out += eng.finalize([s])[0]
            return out, first, second, s.tap(capi.TAP_DEC_STATE).tobytes(), s.tap(capi.TAP_K_CACHE, 1).tobytes()
        finally:
            eng.close()

    a, b = run(False), run(True)
    assert b[1] == b[2] == a[1] == a[2]
    assert a[0] == b[0] and a[3] == b[3] and a[4] == b[4]
    assert len(a[0]) >= 3


def test_errors_and_limits(W):
    mels = build_mels()
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    try:
        eng.set_debug(True)
        good = ([mels[5], mels[13]], [[3, 4], [5]])

        def ok():
            res = eng.align_mel(*good)
            assert eng.align_lattice(1, 1)[0].shape == (13, 2)
            return res

        base = ok()
        for bad_tokens, msg in (([[3, BLANK], [5]], "utterance 0.*blank"), ([[3, 4], [1025]], "utterance 1.*1025"),
                                ([[3, 4], [7] * 1025], "utterance 1.*1025 tokens.*NASR_ALIGN_MAX_TOKENS"), ([[3, 4], [-1]], "utterance 1")):
            with pytest.raises(capi.NasrError, match=msg):
                eng.align_mel(good[0], bad_tokens)
            with pytest.raises(capi.NasrError, match="no lattice"):          # the previous results stay gone
                eng.align_lattice(0)
            assert [r[:3] for r in ok()] == [r[:3] for r in base]            # the engine stays usable
        assert orf.enc_frames(8 * 2048) == 2049
        with pytest.raises(capi.NasrError, match="2048"):
            eng.align_mel([mels[5], np.zeros((8 * 2048, 128), np.float32)], [[1], [2]])
        with pytest.raises(capi.NasrError, match="no lattice"):
            eng.align_lattice(0)
        with pytest.raises(capi.NasrError, match="NO_SYNC"):
            eng.align_mel(*good, flags=capi.FLAG_NO_SYNC)
        # the longest transcript the call takes
        long_y = (np.arange(1024) % 1024).tolist()
        r = eng.align_mel([mels[5]], [long_y])[0]
        assert math.isfinite(r[0]) and r[0] >= r[1] and len(r[2]) == 1024 and all(0 <= f < 5 for f in r[2])
        # no encoder frame
        empty = np.zeros((0, 128), np.float32)
        r = eng.align_mel([empty, empty, mels[1]], [[], [4, 5], [9]])
        assert r[0][:3] == (0.0, 0.0, []) and r[0][3].size == 0
        assert r[1][0] == r[1][1] == -math.inf and r[1][2] == [-1, -1] and np.isneginf(r[1][3]).all()
        assert math.isfinite(r[2][0]) and r[2][2] == [0]
        assert eng.align_lattice(0, 0)[0].size == 0 and eng.align_lattice(2)[0].shape == (1, 2)      # the binding knows U of the call
        assert np.isneginf(eng.align_lattice(2)[1][:, 1]).all()
        # a transcribe call forgets the lattice; without debug there is none
        eng.transcribe_mel([mels[5]])
        with pytest.raises(capi.NasrError, match="no lattice"):
            eng.align_lattice(0)
        eng.set_debug(False)
        eng.align_mel(*good)
        with pytest.raises(capi.NasrError, match="set_debug"):
            eng.align_lattice(0)
        # the PCM entry is the mel entry behind the device preprocessor
        pcm = synth.make_pcm(5, 1.5)
        eng.set_debug(True)
        a = eng.align([pcm], [[11, 12, 13]])[0]
        mel = eng.offline_tap(capi.TAP_MEL, 0)
        b = eng.align_mel([mel], [[11, 12, 13]])[0]
        assert a[:3] == b[:3] and a[3].tobytes() == b[3].tobytes()
        dev = [(eng.upload(pcm), pcm.size)]
        c = eng.align(dev, [[11, 12, 13]], flags=capi.FLAG_PCM_DEVICE)[0]
        assert c[:3] == a[:3]
    finally:
        eng.close()


def test_cli_word_rows_and_loglik(tmp_path, W):
    """nemotron-align-amd on a synthetic GGUF with an ids: transcript: its word rows and loglik are those of the capi call"""
    vocab = gguf_io.synthetic_vocab()
    model = tmp_path / "model.gguf"
    gguf_io.write_gguf(model, W, gguf_io.default_hparams(n_layers=2), vocab)
    pcm = synth.make_pcm(2, 5.0)
    audio = tmp_path / "a.pcm"
    pcm.tofile(audio)
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=1)
    try:
        toks, _ = eng.transcribe([pcm])
        y = toks[0][:12]
        assert len(y) >= 4
        loglik, best, frames, lps = eng.align([pcm], [y])[0]
    finally:
        eng.close()
    text = tmp_path / "t.txt"
    text.write_text("ids:" + ",".join(str(t) for t in y) + "\n")
    r = subprocess.run([str(BIN / "nemotron-align-amd"), str(model), str(audio), str(text), "--f32", "--print-tokens"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    lines = r.stdout.strip().splitlines()
    kv = dict(ln.split(None, 1) for ln in lines if ln.split()[0] in ("loglik", "best", "tokens", "frames"))
    assert float(kv["loglik"]) == pytest.approx(loglik, abs=1e-5) and float(kv["best"]) == pytest.approx(best, abs=1e-5)
    assert [int(x) for x in kv["tokens"].split()] == y and [int(x) for x in kv["frames"].split()] == frames
    # word rows: a word starts at a piece with the word-boundary mark (and at token 0)
    starts = [i for i, t in enumerate(y) if i == 0 or vocab[t].startswith("▁")]
    rows = [ln.split(None, 3) for ln in lines if ln.split()[0] not in ("loglik", "best", "tokens", "frames")]
    assert len(rows) == len(starts)
    for k, i0 in enumerate(starts):
        i1 = starts[k + 1] if k + 1 < len(starts) else len(y)
        assert float(rows[k][0]) == pytest.approx(frames[i0] * 0.08, abs=1e-3)
        assert float(rows[k][1]) == pytest.approx((frames[i1 - 1] + 1) * 0.08, abs=1e-3)
        assert float(rows[k][2]) == pytest.approx(math.exp(min(float(x) for x in lps[i0:i1])), abs=6e-5)       # printed with four decimals
