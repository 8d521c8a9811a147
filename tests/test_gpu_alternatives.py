"""Top-K token alternatives from the device RNN-T decode (engine option "token_alternatives" = K), through the C ABI.

Value, on the scheme of tests/test_gpu_logprobs.py: the engine's OWN encoder rows (NASR_TAP_ENCODER_OUT per one-chunk call,
nasr_engine_offline_tap offline) go to the oracle's decoder + joint (oracle.binding.OracleModel.decoder_joint), the greedy rules
are replayed in Python, and the top-K (stable: the lower id first among equal logits) and the log-softmax are taken in float64.
The output layer is sharpened with GAIN = 30 as there.

Ids are compared at every emission where the oracle's gaps between ranks 0 .. K are all above GAP_MIN = 1e-3 (30 x the 3.1e-5
deviation of the engine's logits from the oracle's at this gain); a smaller gap leaves the emission out of the id comparison (at
most 5 % of a case's tokens), but the values of the ranks whose ids do agree are still compared.  |ln P - oracle| is held to
LP_BOUND = 2e-4, the project's bound of tests/test_gpu_logprobs.py (4 x the 3.1e-5 measured for the top entry; the lower ranks
come from the same logit arithmetic and the same (m, log s)).  Measured on the MI355X: profiles/token_alternatives.md."""
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi, gguf_io, synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

BLANK, V = 1024, 1025
LOG_V = math.log(V)
LP_BOUND = 2e-4
GAP_MIN = 1e-3
GAIN = 30.0
BIN = Path(__file__).resolve().parent.parent / "nemotron-asr.cpp_amd" / "bin"


@pytest.fixture(scope="module")
def W2():
    return synth.make_weights(n_layers=2)


@pytest.fixture(scope="module")
def WS(W2):
    """the joint's output layer centred over the vocabulary and scaled (tests/test_gpu_logprobs.py::_sharpened)"""
    w = dict(W2)
    wo = np.asarray(W2["joint.joint_net.2.weight"], np.float64)
    bo = np.asarray(W2["joint.joint_net.2.bias"], np.float64)
    w["joint.joint_net.2.weight"] = ((wo - wo.mean(axis=0, keepdims=True)) * GAIN).astype(np.float32)
    w["joint.joint_net.2.bias"] = ((bo - bo.mean()) * GAIN).astype(np.float32)
    return w


def _with_blank_bias(W, delta):
    w = dict(W)
    b = np.array(W["joint.joint_net.2.bias"], np.float32, copy=True)
    b[BLANK] += delta
    w["joint.joint_net.2.bias"] = b
    return w


# ---- the oracle side ------------------------------------------------------------------------------------------------------------------
def replay(om, enc, tokens=None, frames=None):
    """the greedy loop of the reference (src/nemo-stream.cpp:840-930) over encoder rows with the oracle's decoder + joint; with
    tokens / frames given it FOLLOWS them instead of taking the arg-max (phrase boosting: the engine's own emissions, raw logits).
    Returns tokens, frames, iterations and per emission the float64 log-softmax of the raw logits."""
    enc = np.asarray(enc, np.float32).reshape(-1, 1024)
    h, c, prev = np.zeros(1280, np.float32), np.zeros(1280, np.float32), BLANK
    out = dict(tokens=[], frames=[], lsm=[], iterations=0)

    def emit(tok, f, logits, hn, cn):
        x = logits.astype(np.float64)
        out["tokens"].append(int(tok)); out["frames"].append(int(f)); out["lsm"].append(x - np.logaddexp.reduce(x))
        return int(tok), hn, cn

    if tokens is None:
        for f, row in enumerate(enc):
            for _ in range(10):
                out["iterations"] += 1
                logits, hn, cn = om.decoder_joint(prev, h, c, row)
                best = int(np.argmax(logits))                      # first maximum
                if best == BLANK:
                    break
                prev, h, c = emit(best, f, logits, hn, cn)
    else:
        for tok, f in zip(tokens, frames):
            logits, hn, cn = om.decoder_joint(prev, h, c, enc[f])
            prev, h, c = emit(tok, f, logits, hn, cn)
    return out


def compare(got, rep, K, what, min_compared):
    """ids under the gap rule, values under LP_BOUND; returns the largest value deviation"""
    ids, lps = got["ids"], got["lps"]
    n = len(rep["tokens"])
    assert ids.shape == (n, K) and lps.shape == (n, K) and ids.dtype == np.int32 and lps.dtype == np.float32, what
    assert np.isfinite(lps).all() and (lps <= 0).all() and (lps[:, 0] >= -LOG_V - 1e-5).all(), what
    left_out, compared, worst, worst0, min_gap = 0, 0, 0.0, 0.0, np.inf
    for i in range(n):
        lsm = rep["lsm"][i]
        order = np.argsort(-lsm, kind="stable")[:K + 1]
        gaps = -np.diff(lsm[order])
        min_gap = min(min_gap, float(gaps.min()))
        if (gaps > GAP_MIN).all():
            assert ids[i].tolist() == order[:K].tolist(), (what, i, ids[i], order, gaps)
            compared += 1
        else:
            left_out += 1
        agree = ids[i] == order[:K]
        dev = np.abs(lps[i].astype(np.float64) - lsm[order[:K]])
        if agree.any():
            worst = max(worst, float(dev[agree].max()))
        if agree[0]:
            worst0 = max(worst0, float(dev[0]))
    print(f"token_alternatives {what}: K = {K}, {n} tokens, {compared} compared by id, {left_out} left out, smallest oracle gap {min_gap:.2e}, "
          f"max |ln P - oracle| = {worst:.3e} (entry 0 alone: {worst0:.3e})")
    assert left_out <= 0.05 * n, (what, left_out, n)
    assert compared >= min_compared, (what, compared)
    return worst


def assert_rows_well_formed(ids, lps, K):
    """strictly descending keys: values never rise along a row, equal values (equal logit bits) have rising ids, so ids are distinct"""
    assert ids.shape == lps.shape and ids.shape[1] == K
    assert np.isfinite(lps).all() and (lps <= 0).all() and (ids >= 0).all() and (ids < V).all()
    d = np.diff(lps, axis=1)
    assert (d <= 0).all()
    assert (np.diff(ids, axis=1)[d == 0] > 0).all()
    assert all(len(set(r.tolist())) == K for r in ids)
    assert (lps[:, 0] >= -LOG_V - 1e-5).all()
    if K == 8:
        assert (np.exp(lps.astype(np.float64)).sum(axis=1) <= 1 + 1e-5).all()


# ---- the engine side ------------------------------------------------------------------------------------------------------------------
def drive(W, dtype, B, R, n_push, spots, options, seed=700, phrases=None, bonus=None, n_layers=2):
    """one chunk per call + the tail flush; per spot stream: tokens, frames, iterations, alternatives, the encoder rows it decoded"""
    T, n = 1 + R, synth.shift_samples(R)
    pcms = [synth.make_pcm(seed + b, n_push * n / 16000 + 0.35) for b in range(B)]          # + 0.35 s: a tail for finalize
    eng = capi.Engine(W, n_layers=n_layers, dtype=dtype, max_streams=B)
    for k, v in options:
        eng.set_option(k, v)
    if phrases is not None:
        eng.set_boost_phrases(phrases, bonus)
    sts = [eng.stream(R) for _ in range(B)]
    toks = [[] for _ in range(B)]
    enc = {b: [] for b in spots}
    chunks = {b: 0 for b in spots}
    for o in range(0, pcms[0].size, n):
        for b, t in enumerate(eng.step(sts, [p[o:o + n] for p in pcms])):
            toks[b] += t
        for b in spots:
            c = sts[b].progress().chunks
            assert c - chunks[b] <= 1
            if c > chunks[b]:
                enc[b].append(sts[b].tap(capi.TAP_ENCODER_OUT).reshape(-1, 1024)[:T].copy())
            chunks[b] = c
    n_valid = {b: min(max((sts[b].progress().mel_frames_buffered - 9) // 8, 0), T) for b in spots}
    for b, t in enumerate(eng.finalize(sts)):
        toks[b] += t
    out = {}
    lp_on = dict(options).get("token_logprobs", 0)
    for b in spots:
        if n_valid[b] > 0:
            enc[b].append(sts[b].tap(capi.TAP_ENCODER_OUT).reshape(-1, 1024)[:n_valid[b]].copy())
        ids, lps = sts[b].token_alternatives()
        out[b] = dict(tokens=toks[b], frames=sts[b].token_frames(), iterations=sts[b].stats().decode_iterations, ids=ids, lps=lps,
                      tlp=sts[b].token_logprobs() if lp_on else None, enc=np.concatenate(enc[b]), tail_frames=n_valid[b])
    eng.close()
    return out


def check_greedy(got, om, K, what, min_compared):
    rep = replay(om, got["enc"])
    assert got["tokens"] == rep["tokens"] and got["frames"] == rep["frames"] and got["iterations"] == rep["iterations"], what
    assert (got["ids"][:, 0] == np.asarray(rep["tokens"])).all(), what           # no boosting: entry 0 is the emitted token
    assert_rows_well_formed(got["ids"], got["lps"], K)
    return compare(got, rep, K, what, min_compared), rep


_cache = {}


def one_stream(W, dtype, K):
    """1 stream x R = 0 x 30 pushes, tail flush included (shared by the value, K = 8 and prefix tests)"""
    if (dtype, K) not in _cache:
        _cache[(dtype, K)] = drive(W, dtype, 1, 0, 30, (0,), (("token_alternatives", K),))[0]
    return _cache[(dtype, K)]


# ---- value ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [capi.DTYPE_F32, capi.DTYPE_BF16])
def test_value_one_stream_small_joint_kernel(WS, dtype):
    """1 stream x R = 0: one row per step, k_dec_joint (65 slices per row), the tail flush included"""
    worst, _ = check_greedy(one_stream(WS, dtype, 4), ob.OracleModel(WS, 2), 4, f"1 x R=0 dtype {dtype}", 15)
    assert worst < LP_BOUND, worst


def test_value_k8_one_stream_and_k4_is_its_prefix(WS):
    k8, k4 = one_stream(WS, capi.DTYPE_BF16, 8), one_stream(WS, capi.DTYPE_BF16, 4)
    worst, _ = check_greedy(k8, ob.OracleModel(WS, 2), 8, "1 x R=0 K=8", 15)
    assert worst < LP_BOUND, worst
    assert k4["tokens"] == k8["tokens"]
    assert k4["ids"].tobytes() == np.ascontiguousarray(k8["ids"][:, :4]).tobytes()
    assert k4["lps"].tobytes() == np.ascontiguousarray(k8["lps"][:, :4]).tobytes()


def test_value_64_streams_tiled_joint_kernel(WS):
    """64 streams x R = 13: 896 rows per step, k_dec_joint_tiled (17 slices per row); the tail flush decodes fewer frames per stream"""
    spots = (0, 21, 42, 63)
    out = drive(WS, capi.DTYPE_BF16, 64, 13, 3, spots, (("token_alternatives", 4),))
    om = ob.OracleModel(WS, 2)
    assert sum(out[b]["tail_frames"] for b in spots) > 0
    worst, total = 0.0, 0
    for b in spots:
        d, rep = check_greedy(out[b], om, 4, f"64 x R=13 stream {b}", 0)
        worst, total = max(worst, d), total + len(rep["tokens"])
    assert total >= 20
    assert worst < LP_BOUND, worst


def test_value_ten_symbols_per_frame(WS):
    """blank bias -1e9: every frame runs into the 10-symbol cap; each symbol is ranked at the decoder state of ITS iteration"""
    W = _with_blank_bias(WS, -1e9)
    got = drive(W, capi.DTYPE_F32, 1, 0, 4, (0,), (("token_alternatives", 4),), seed=950)[0]
    worst, rep = check_greedy(got, ob.OracleModel(W, 2), 4, "blank bias -1e9 R=0", 15)
    per_frame = np.bincount(np.asarray(rep["frames"], np.int64))
    assert set(per_frame[per_frame > 0].tolist()) == {10}
    assert not (got["ids"] == BLANK).any()                                        # at -1e9 blank is the last of the 1025
    assert worst < LP_BOUND, worst


def test_value_offline_ragged_batch_over_two_decode_windows(WS):
    """one offline call, three utterances of ragged lengths, the longest spanning two 256-frame decode windows"""
    secs = (22.5, 8.0, 0.9)
    pcms = [synth.make_pcm(300 + i, s) for i, s in enumerate(secs)]
    eng = capi.Engine(WS, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    eng.set_option("token_alternatives", 4)
    eng.set_debug(True)
    toks, frames = eng.transcribe(pcms)
    om = ob.OracleModel(WS, 2)
    worst, total = 0.0, 0
    for u in range(len(pcms)):
        enc = eng.offline_tap(capi.TAP_ENCODER_OUT, u)
        if u == 0:
            assert enc.shape[0] > 256
        ids, lps = eng.offline_token_alternatives(u)
        got = dict(tokens=toks[u], frames=frames[u], ids=ids, lps=lps, enc=enc)
        got["iterations"] = replay(om, enc)["iterations"]                         # an offline call reports no iteration count
        d, rep = check_greedy(got, om, 4, f"offline utterance {u} ({enc.shape[0]} frames)", 0)
        worst, total = max(worst, d), total + len(rep["tokens"])
    assert total >= 20 and max(frames[0]) >= 256                                  # tokens of the second window are there
    eng.transcribe(pcms[2:])                                                      # the values belong to the LAST call
    with pytest.raises(capi.NasrError):
        eng.offline_token_alternatives(1)
    assert eng.offline_token_alternatives(0)[0].shape == (len(toks[2]), 4)
    eng.close()
    assert worst < LP_BOUND, worst


# ---- bit-for-bit properties -------------------------------------------------------------------------------------------------------------
def run(W, B, R, n_push, options, seed=500, dtype=capi.DTYPE_BF16, phrases=None, bonus=None):
    n = synth.shift_samples(R)
    pcms = [synth.make_pcm(seed + b, n_push * n / 16000 + 0.35) for b in range(B)]
    eng = capi.Engine(W, n_layers=2, dtype=dtype, max_streams=B)
    for k, v in options:
        eng.set_option(k, v)
    if phrases is not None:
        eng.set_boost_phrases(phrases, bonus)
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
               alts=[s.token_alternatives() for s in sts] if opt.get("token_alternatives", 0) else None,
               tlp=[s.token_logprobs() for s in sts] if opt.get("token_logprobs", 0) else None,
               graph_replays=eng.counter("graph_replays"), pipelined=eng.counter("pipelined_steps"))
    eng.close()
    return res


def same_decode(a, b):
    return a["tokens"] == b["tokens"] and a["frames"] == b["frames"] and a["iterations"] == b["iterations"] and a["state"] == b["state"]


def same_bits(a, b):
    return all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() for x, y in zip(a["alts"], b["alts"]))


@pytest.mark.parametrize("B,R,n_push", [(1, 0, 24), (64, 13, 3)])
def test_option_changes_nothing_but_adds_the_rows_and_is_deterministic(WS, B, R, n_push):
    on = (("token_alternatives", 8), ("token_logprobs", 1))
    off = run(WS, B, R, n_push, ())
    base = run(WS, B, R, n_push, on)
    assert sum(len(t) for t in base["tokens"]) >= 5 and base["graph_replays"] > 0
    assert same_decode(off, base)                                              # tokens, frames, iteration counts, decoder state: bit-identical to the option off
    alone = run(WS, B, R, n_push, on[:1])                                      # without "token_logprobs": the same decode, the same rows
    assert same_decode(off, alone) and same_bits(base, alone)
    eager = run(WS, B, R, n_push, on + (("graph", 0),))
    assert eager["graph_replays"] == 0 and same_decode(base, eager) and same_bits(base, eager)       # graph replay == eager launches
    pipe = run(WS, B, R, n_push, on + (("pipeline", 4),))
    assert pipe["pipelined"] > 0 and same_decode(base, pipe) and same_bits(base, pipe)               # pipelined == synchronous
    again = run(WS, B, R, n_push, on)
    assert same_bits(base, again)                                              # a second engine: no run-to-run variation
    if B == 1:
        grouped = run(WS, B, R, n_push, on + (("pipeline", 8),))
        assert same_decode(base, grouped) and same_bits(base, grouped)
    for b in range(B):
        ids, lps = base["alts"][b]
        assert ids.shape == (len(base["tokens"][b]), 8)
        if ids.shape[0] == 0:
            continue
        assert_rows_well_formed(ids, lps, 8)
        assert ids[:, 0].tolist() == base["tokens"][b]                         # no boosting: entry 0 is the token ...
        assert np.ascontiguousarray(lps[:, 0]).tobytes() == base["tlp"][b].tobytes()      # ... and its value is the token's log-probability, to the byte


# ---- with phrase boosting ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,R,n_push,seed", [(1, 0, 30, 700), (16, 13, 3, 700)])
def test_ranking_stays_the_models_under_phrase_boosting(WS, B, R, n_push, seed):
    """a one-token phrase [x] for the runner-up x of the emission with the smallest gap, bonus = gap + 1.0 rounded to one decimal (the
    single-token pattern of tests/test_gpu_boost.py::choose_phrases): x is emitted where the model preferred another token.  The replay
    follows the engine's own emissions and ranks the RAW logits.  k_dec_joint at 1 stream, k_dec_joint_tiled at 16 x 14 rows."""
    K = 4
    om = ob.OracleModel(WS, 2)
    base_opts = (("token_alternatives", K), ("token_logprobs", 1))
    opts = base_opts + (("phrase_boost", 64),)
    plain = drive(WS, capi.DTYPE_F32, B, R, n_push, (0,), base_opts, seed=seed)[0]
    empty = drive(WS, capi.DTYPE_F32, B, R, n_push, (0,), opts, seed=seed)[0]
    # the option on and no phrases set: everything equals boosting off
    assert empty["tokens"] == plain["tokens"] and empty["frames"] == plain["frames"] and empty["iterations"] == plain["iterations"]
    assert empty["ids"].tobytes() == plain["ids"].tobytes() and empty["lps"].tobytes() == plain["lps"].tobytes()
    assert empty["tlp"].tobytes() == plain["tlp"].tobytes()
    rep = replay(om, plain["enc"])
    assert rep["tokens"] == plain["tokens"]
    cands = []
    for i, lsm in enumerate(rep["lsm"]):
        o = np.argsort(-lsm, kind="stable")[:2]
        if o[1] != BLANK:
            cands.append((float(lsm[o[0]] - lsm[o[1]]), int(o[1])))
    gap, x = min(cands)
    bonus = round(gap + 1.0, 1)
    got = drive(WS, capi.DTYPE_F32, B, R, n_push, (0,), opts, seed=seed, phrases=[[x]], bonus=[bonus])[0]
    assert got["enc"].tobytes() == plain["enc"].tobytes()                       # the encoder does not see the decode
    follow = replay(om, got["enc"], got["tokens"], got["frames"])
    worst = compare(got, follow, K, f"{B} x R={R} boosted [{x}] +{bonus}", 15 if B == 1 else 5)
    assert worst < LP_BOUND, worst
    assert_rows_well_formed(got["ids"], got["lps"], K)
    toks = np.asarray(got["tokens"])
    moved = got["ids"][:, 0] != toks
    print(f"token_alternatives boosted: {int(moved.sum())} of {toks.size} tokens are not the model's first choice")
    assert moved.any() and (toks[moved] == x).all()
    # wherever the token is among the K its value is the token's own log-probability, to the byte
    hit = got["ids"] == toks[:, None]
    assert hit.any(axis=1).sum() >= toks.size - int(moved.sum())
    assert got["lps"][hit].tobytes() == got["tlp"][hit.any(axis=1)].tobytes()


# ---- ring, reset, errors ------------------------------------------------------------------------------------------------------------------
def test_range_ring_reset_and_errors(WS):
    R, T, K = 13, 14, 4
    W = _with_blank_bias(WS, -1e9)                                             # ten tokens per frame: the ring wraps quickly
    n = synth.shift_samples(R) * 8                                             # eight chunks per call = 1 120 tokens
    pcm = synth.make_pcm(77, 4 * n / 16000 + 0.05)
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=2)
    for bad in (9, -1):
        with pytest.raises(capi.NasrError, match="token_alternatives must be 0 .. 8"):
            eng.set_option("token_alternatives", bad)
    eng.set_option("token_alternatives", 0)
    eng.set_option("token_alternatives", K)
    st = eng.stream(R)
    toks = eng.step([st], [pcm[:n]], tok_cap=2048)[0]
    assert len(toks) % 10 == 0 and len(toks) >= 7 * T * 10
    with pytest.raises(capi.NasrError, match="token_alternatives must be set before the first step"):
        eng.set_option("token_alternatives", 0)
    ids, lps = st.token_alternatives()
    assert ids.shape == (len(toks), K) and ids[:, 0].tolist() == toks
    assert_rows_well_formed(ids, lps, K)
    assert np.unique(lps).size > 100                                           # values, not a fill pattern
    # first / count clip like the frames
    a, b = st.token_alternatives(10, 5)
    assert a.tobytes() == ids[10:15].tobytes() and b.tobytes() == lps[10:15].tobytes() and len(st.token_frames(10, 5)) == 5
    a, b = st.token_alternatives(len(toks) - 3, 50)
    assert a.tobytes() == ids[-3:].tobytes() and b.tobytes() == lps[-3:].tobytes() and len(st.token_frames(len(toks) - 3, 50)) == 3
    assert st.token_alternatives(len(toks), 4)[0].shape[0] == 0 and st.token_alternatives(len(toks) + 7, 4)[1].shape[0] == 0
    with pytest.raises(capi.NasrError, match="negative"):
        st.token_alternatives(-1, 2)
    # past the ring
    for k in range(1, 4):
        toks += eng.step([st], [pcm[k * n:(k + 1) * n]], tok_cap=2048)[0]
    assert len(toks) > 4096 + 100
    with pytest.raises(capi.NasrError, match="older than the 4096-token device ring"):
        st.token_alternatives(0, 1)
    a, b = st.token_alternatives(len(toks) - 4096, 4096)
    assert a.shape == (4096, K) and a[:, 0].tolist() == toks[-4096:]
    assert_rows_well_formed(a, b, K)
    # reset restarts the numbering and reproduces the same bytes
    st.reset()
    assert st.token_alternatives()[0].shape[0] == 0
    again = eng.step([st], [pcm[:n]], tok_cap=2048)[0]
    assert again == toks[:len(again)]
    a, b = st.token_alternatives()
    assert a.tobytes() == ids.tobytes() and b.tobytes() == lps.tobytes()
    st.reset(reference=True)                                                   # both reset modes restart the numbering
    assert st.token_alternatives()[0].shape[0] == 0
    eng.close()
    # option off: both getters fail and name the option
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    st = eng.stream(0)
    eng.step([st], [pcm[:1280 * 4]])
    with pytest.raises(capi.NasrError, match="token_alternatives"):
        st.token_alternatives(0, 1)
    with pytest.raises(capi.NasrError, match="token_alternatives"):
        eng.offline_token_alternatives(0)
    with pytest.raises(capi.NasrError, match="token_alternatives must be set before the first step"):
        eng.set_option("token_alternatives", 4)
    eng.close()
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    eng.transcribe([pcm[:16000]])
    with pytest.raises(capi.NasrError, match="token_alternatives must be set before the first step or offline call"):
        eng.set_option("token_alternatives", 4)
    eng.close()


# ---- the command-line tool ----------------------------------------------------------------------------------------------------------------
def test_cli_alternatives(tmp_path, WS):
    """nemotron-asr-amd --alternatives 3: the same first line and TOKENS line, and one `alt i id:p id:p id:p` line per token between them"""
    vocab = gguf_io.synthetic_vocab()
    model = tmp_path / "model.gguf"
    gguf_io.write_gguf(model, WS, gguf_io.default_hparams(n_layers=2), vocab)
    audio = tmp_path / "a.pcm"
    synth.make_pcm(2, 5.0).tofile(audio)
    cli = str(BIN / "nemotron-asr-amd")

    def cli_run(*flags):
        r = subprocess.run([cli, str(model), str(audio), "80", "0", "--f32", "--print-tokens", *flags], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-800:]
        return r.stdout.splitlines()

    plain = cli_run()
    alt = cli_run("--alternatives", "3")
    assert alt[0] == plain[0] and alt[-1] == plain[-1]
    toks = [int(x) for x in plain[-1].split()[1:]]
    assert len(toks) >= 2
    lines = [ln for ln in alt if ln.startswith("alt ")]
    assert len(lines) == len(toks) and len(alt) == len(plain) + len(toks)
    for i, ln in enumerate(lines):
        m = re.fullmatch(r"alt (\d+)((?: \d+:\d\.\d{4}){3})", ln)
        assert m and int(m.group(1)) == i, ln
        pairs = [p.split(":") for p in m.group(2).split()]
        assert int(pairs[0][0]) == toks[i]
        ps = [float(p[1]) for p in pairs]
        assert all(0.0 <= p <= 1.0 for p in ps) and ps == sorted(ps, reverse=True)
    bad = subprocess.run([cli, str(model), str(audio), "80", "0", "--f32", "--alternatives", "9"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "token_alternatives" in bad.stderr
