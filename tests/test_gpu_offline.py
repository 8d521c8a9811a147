"""Offline full-context transcription on the MI355X (nasr_engine_transcribe / _mel): whole utterances, batched and ragged,
against the numpy restatement of the reference's offline encoder (tests/offline_ref.py) and the oracle's greedy decode."""
import numpy as np
import pytest

from nemotron_asr_amd import capi, synth
from oracle import binding as ob
from tests import offline_ref as orf

pytestmark = pytest.mark.gpu


def mel_for(T, rng):
    """a log-mel of the fewest frames that give T encoder frames"""
    n = max(1, 8 * (T - 3))
    while orf.enc_frames(n) < T:
        n += 1
    assert orf.enc_frames(n) == T
    return rng.standard_normal((n, 128)).astype(np.float32)


@pytest.fixture(scope="module")
def f32_two_layers(weights2):
    eng = capi.Engine(weights2, n_layers=2, dtype=capi.DTYPE_F32, max_streams=2)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def oracle2(weights2):
    return ob.OracleModel(weights2, 2)


def test_f32_ragged_batch_matches_restatement(f32_two_layers, oracle2, weights2):
    rng = np.random.default_rng(11)
    lens = [1, 2, 63, 64, 65, 300]
    mels = [mel_for(T, rng) for T in lens]
    eng = f32_two_layers
    eng.set_debug(True)
    for group in (mels, [mel_for(2048, rng)]):
        toks, frames = eng.transcribe_mel(group)
        for u, mel in enumerate(group):
            sub, outs, enc = orf.encode(oracle2, weights2, mel, 2)
            T = sub.shape[0]
            got_sub = eng.offline_tap(capi.TAP_SUBSAMPLED, u)
            assert got_sub.shape == sub.shape
            assert np.abs(got_sub - sub).max() < 2e-3
            for l in range(2):
                got = eng.offline_tap(capi.TAP_LAYER_OUT, u, l)
                assert np.abs(got - outs[l]).max() < 2e-3, (T, l, np.abs(got - outs[l]).max())
            got_enc = eng.offline_tap(capi.TAP_ENCODER_OUT, u)
            assert np.abs(got_enc - enc).max() < 2e-3
            want_t, want_f = orf.greedy(oracle2, enc)
            assert toks[u] == want_t, T
            assert frames[u] == want_f, T
            if ob.have_ref() and T <= 300:
                assert toks[u] == ob.ref_greedy(weights2, enc)
    eng.set_debug(False)


def test_limits(f32_two_layers, oracle2, weights2):
    eng = f32_two_layers
    rng = np.random.default_rng(5)
    n_over = 8 * 2048
    assert orf.enc_frames(n_over) == 2049
    with pytest.raises(capi.NasrError, match="2048"):
        eng.transcribe_mel([mel_for(4, rng), rng.standard_normal((n_over, 128)).astype(np.float32)])
    mel1 = mel_for(1, rng)
    toks, frames = eng.transcribe_mel([np.zeros((0, 128), np.float32), mel1])
    assert toks[0] == [] and frames[0] == []
    _, _, enc = orf.encode(oracle2, weights2, mel1, 2)
    assert toks[1] == orf.greedy(oracle2, enc)[0]
    assert eng.transcribe_mel([np.zeros((0, 128), np.float32)]) == ([[]], [[]])


def test_bf16_batch_equals_alone_bit_for_bit(weights2):
    rng = np.random.default_rng(7)
    mels = [mel_for(T, rng) for T in (1, 2, 63, 64, 65, 300)]
    eng = capi.Engine(weights2, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    try:
        eng.set_debug(True)

        def run(group):
            toks, frames = eng.transcribe_mel(group)
            encs = [eng.offline_tap(capi.TAP_ENCODER_OUT, u) for u in range(len(group))]
            return toks, frames, encs

        batch = run(mels)
        alone = [run([m]) for m in mels]
        eng.set_option("offline_rows", 70)
        split = run(mels)
        for u in range(len(mels)):
            for got in (batch, split):
                assert got[0][u] == alone[u][0][0]
                assert got[1][u] == alone[u][1][0]
                assert np.array_equal(got[2][u], alone[u][2][0])
    finally:
        eng.close()


def test_multilingual_prompts_f32():
    w = synth.make_weights(n_layers=1, num_prompts=128)
    oracle = ob.OracleModel(w, 1, num_prompts=128)
    rng = np.random.default_rng(3)
    mels = [mel_for(40, rng), mel_for(57, rng)]
    prompts = [3, 101]
    eng = capi.Engine(w, n_layers=1, dtype=capi.DTYPE_F32, max_streams=1, num_prompts=128)
    try:
        eng.set_debug(True)
        toks, _ = eng.transcribe_mel(mels, prompts=prompts)
        for u, (mel, p) in enumerate(zip(mels, prompts)):
            _, _, enc = orf.encode(oracle, w, mel, 1, prompt=p, num_prompts=128)
            got = eng.offline_tap(capi.TAP_ENCODER_OUT, u)
            assert np.abs(got - enc).max() < 2e-3
            assert toks[u] == orf.greedy(oracle, enc, p)[0]
    finally:
        eng.close()


@pytest.mark.parametrize("pipeline", [0, 4])
def test_streams_untouched_by_offline_calls(weights2, pipeline):
    rng = np.random.default_rng(9)
    pcm = (rng.standard_normal(16000 * 3) * 3000).astype(np.int16)
    off_mels = [mel_for(30, rng), mel_for(90, rng)]
    counters = ("graph_shapes", "graph_evictions", "graph_execs")

    def run(interleave):
        eng = capi.Engine(weights2, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=2)
        try:
            eng.set_option("pipeline", pipeline)
            s = eng.stream(right_context=1)
            out = []
            for k in range(0, pcm.size, 4000):
                out += eng.step([s], [pcm[k:k + 4000]])[0]
                if interleave:
                    before = [eng.counter(c) for c in counters]
                    eng.transcribe_mel(off_mels)
                    assert [eng.counter(c) for c in counters] == before
            out += eng.finalize([s])[0]
            return out, s.tap(capi.TAP_K_CACHE, 1), s.tap(capi.TAP_CONV_CACHE, 0)
        finally:
            eng.close()

    a, b = run(False), run(True)
    assert a[0] == b[0]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


BF16_MAX, BF16_MEAN = 3e-2, 5e-3          # bf16 engine against the f32 reference arithmetic
EPS_MARGIN = 0.05                          # tests/test_gpu_speech.py: bf16 score noise on the speech checkpoint (DESIGN §2 margin rule)


def test_bf16_attention_path_matches_f32_reference(weights2):
    """k_off_attn_bf16 (band skew, P.V key order, online softmax), the bf16 front end, depthwise conv and folded residual GEMMs
    against the float64 restatement: every layer tap of the ragged batch, the 2048-frame utterance included."""
    rng = np.random.default_rng(13)
    groups = [[mel_for(T, rng) for T in (1, 2, 63, 64, 65, 300)], [mel_for(2048, rng)]]
    oracle = ob.OracleModel(weights2, 2)
    eng = capi.Engine(weights2, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    try:
        eng.set_debug(True)
        for group in groups:
            eng.transcribe_mel(group)
            diffs = {}                                     # tap -> |bf16 - f32 restatement| of every row of the group
            for u, mel in enumerate(group):
                sub, outs, enc = orf.encode(oracle, weights2, mel, 2)
                pairs = [("sub", eng.offline_tap(capi.TAP_SUBSAMPLED, u), sub)] + \
                        [(f"layer{l}", eng.offline_tap(capi.TAP_LAYER_OUT, u, l), outs[l]) for l in range(2)]
                for name, got, want in pairs:
                    assert got.shape == want.shape
                    diffs.setdefault(name, []).append(np.abs(got - want).ravel())
            # INTEGRATION.md's metric: max over every element, mean over the whole output (not over one row of 1024 values)
            for name, d in diffs.items():
                d = np.concatenate(d)
                assert d.max() < BF16_MAX and d.mean() < BF16_MEAN, (name, len(group), d.max(), d.mean())
    finally:
        eng.close()


def test_bf16_batch_with_prompts_equals_alone_at_large_m():
    """bit identity across batch composition at M above the wide-tile threshold, prompt-fusion GEMMs included"""
    w = synth.make_weights(n_layers=1, num_prompts=128)
    rng = np.random.default_rng(17)
    mels = [mel_for(T, rng) for T in (1, 65, 700, 1500)]
    prompts = [5, 0, 77, -1]
    eng = capi.Engine(w, n_layers=1, dtype=capi.DTYPE_BF16, max_streams=1, num_prompts=128)
    try:
        eng.set_debug(True)

        def run(idx):
            toks, frames = eng.transcribe_mel([mels[i] for i in idx], prompts=[prompts[i] for i in idx])
            return toks, frames, [eng.offline_tap(capi.TAP_ENCODER_OUT, u) for u in range(len(idx))]

        batch = run(range(4))
        alone = [run([i]) for i in range(4)]
        eng.set_option("offline_rows", 800)
        split = run(range(4))
        for u in range(4):
            for got in (batch, split):
                assert got[0][u] == alone[u][0][0] and got[1][u] == alone[u][1][0]
                assert np.array_equal(got[2][u], alone[u][2][0])
    finally:
        eng.close()


def test_pcm_entry_equals_mel_entry(f32_two_layers, weights2):
    """nasr_engine_transcribe: the device preprocessor over each whole utterance = orc_preproc_process(whole pcm)"""
    rng = np.random.default_rng(21)
    pcms = [(rng.standard_normal(n) * 2000).astype(np.int16) for n in (100, 255, 256, 4000, 16000 * 7 + 37, MAX_PUSH_PLUS)]
    eng = f32_two_layers
    eng.set_debug(True)
    toks, frames = eng.transcribe(pcms)
    mels = []
    for u, p in enumerate(pcms):
        pp = ob.OraclePreproc(weights2["preprocessor.featurizer.fb"], weights2["preprocessor.featurizer.window"])
        want = pp.process(p)
        got = eng.offline_tap(capi.TAP_MEL, u)
        assert got.shape == want.shape, (p.size, got.shape, want.shape)
        if want.size:
            assert np.abs(got - want).max() < 2e-5
        mels.append(want)
    toks_m, frames_m = eng.transcribe_mel(mels)
    assert toks == toks_m and frames == frames_m
    dev = [(eng.upload(p), p.size) for p in pcms]
    assert eng.transcribe(dev, flags=capi.FLAG_PCM_DEVICE) == (toks, frames)
    with pytest.raises(capi.NasrError, match="2048"):
        eng.transcribe([np.zeros(16000 * 164, np.int16)])
    eng.set_debug(False)


MAX_PUSH_PLUS = 1280 * 256 * 2 + 999      # three internal sub-pushes of the preprocessor


def test_speech_checkpoint_24_layers_bf16_tokens_equal_f32():
    """24 layers, speech checkpoint, 4 utterances x 20 s through the PCM entry: the bf16 engine's encoder output within the bf16
    tolerance of the f32 engine's (pinned to the restatement by the tests above), and its tokens equal, or every difference at an
    oracle decision whose top-2 margin is below EPS_MARGIN (decision log of the oracle decoding the f32 encoder output)."""
    W = synth.make_weights(24, margins="speech")
    pcms = [synth.make_speech_pcm(s, 20.0)[0] for s in range(4)]
    res = {}
    for dt in (capi.DTYPE_F32, capi.DTYPE_BF16):
        eng = capi.Engine(W, n_layers=24, dtype=dt, max_streams=1)
        try:
            eng.set_debug(True)
            toks, frames = eng.transcribe(pcms)
            res[dt] = (toks, frames, [eng.offline_tap(capi.TAP_ENCODER_OUT, u) for u in range(len(pcms))])
        finally:
            eng.close()
    om = ob.OracleModel(W, 24)
    n_tok = 0
    for u in range(len(pcms)):
        ref, got = res[capi.DTYPE_F32][2][u], res[capi.DTYPE_BF16][2][u]
        d = np.abs(got - ref)
        assert d.max() < BF16_MAX and d.mean() < BF16_MEAN, (u, d.max(), d.mean())
        st = ob.OracleStream(om, 0)
        st.enable_decision_log()
        want = st.decode(ref)
        wframes = st.token_frames()[:len(want)]
        assert want == res[capi.DTYPE_F32][0][u]
        n_tok += len(want)
        rep = ob.token_timing_report(st.decision_log(), want, wframes, res[capi.DTYPE_BF16][0][u], res[capi.DTYPE_BF16][1][u])
        if not rep["tokens_equal"]:
            fd = rep["first_divergence"]
            assert fd is not None and fd["margin"] < EPS_MARGIN, rep
        for s in rep["shifts"]:
            assert s["margin"] < EPS_MARGIN, rep
    assert n_tok >= 40
