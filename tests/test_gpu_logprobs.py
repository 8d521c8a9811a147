"""Per-token log-probabilities from the device RNN-T decode (engine option "token_logprobs"), through the C ABI.

Value: the engine's OWN encoder rows (NASR_TAP_ENCODER_OUT per one-chunk call, nasr_engine_offline_tap offline) go to the oracle's
decoder + joint (oracle.binding.OracleModel.decoder_joint), the greedy rules are replayed in Python and the log-softmax is taken in
float64.  That isolates the decode, which is f32 in both engine dtypes, so one bound serves f32 and bf16 engines.

LP_BOUND, measured on the MI355X (profiles/token_logprobs.md): the largest |lp_engine - lp_oracle| over the cases of
test_value_* was MEASURED_MAX = 3.1e-5 (offline, the 12-frame utterance; streaming cases 1.1e-5 .. 2.6e-5; 1.5e-6 on the
unsharpened checkpoint); the bound is 4 x that, rounded up to one digit = 2e-4 (the engine sums the K = 640 / 1024 products of
the decoder and the joint in another order than the oracle, so its logits differ by a few f32 ulp of their partial sums).  A
MEASURED deviation above 1e-4 (ten times the 1e-5 logit deviation stated for the decode) would be a defect to explain, not a
tolerance to raise.

End to end at the benchmarked precision (bf16, 24 layers, speech checkpoint) against the F32 oracle's own stream, measured:
19 tokens compared, max |d lp| = 0.0104, mean 0.0024, none left out (profiles/token_logprobs.md); bound 0.2."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi, gguf_io, synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

BLANK, V = 1024, 1025
LOG_V = math.log(V)
MEASURED_MAX = 3.1e-5         # MI355X, see the docstring
LP_BOUND = 2e-4               # 4 x MEASURED_MAX = 1.24e-4, rounded up to one digit
# rows of the sharpened output layer: 30 x the random checkpoint's (norm 1), 3.5 x the largest row of the speech checkpoint's read-out (8.5).
# The engine's logits differ from the oracle's by f32 rounding of the 640 hidden activations times these weights, so the deviation of lp
# scales with this gain (measured: 1.5e-6 at gain 1, 3.1e-5 at 30, 1.3e-4 at 300); it is kept at the scale of a trained joint.
GAIN = 30.0
BIN = Path(__file__).resolve().parent.parent / "nemotron-asr.cpp_amd" / "bin"


@pytest.fixture(scope="module")
def W2():
    return synth.make_weights(n_layers=2)


def _sharpened(W, gain):
    """the joint's output layer centred over the vocabulary (every logit of a row moves by the same amount: arg-max and softmax are
    unchanged in exact arithmetic) and scaled: the near-tie checkpoint's logits share a large common part and are ~1e-3 apart, so every
    lp would sit near -ln 1025; centred and scaled they are a few units apart around 0, like a trained joint's"""
    w = dict(W)
    wo = np.asarray(W["joint.joint_net.2.weight"], np.float64)
    bo = np.asarray(W["joint.joint_net.2.bias"], np.float64)
    w["joint.joint_net.2.weight"] = ((wo - wo.mean(axis=0, keepdims=True)) * gain).astype(np.float32)
    w["joint.joint_net.2.bias"] = ((bo - bo.mean()) * gain).astype(np.float32)
    return w


def _with_blank_bias(W, delta):
    w = dict(W)
    b = np.array(W["joint.joint_net.2.bias"], np.float32, copy=True)
    b[BLANK] += delta
    w["joint.joint_net.2.bias"] = b
    return w


class Replay:
    """the greedy loop of the reference (src/nemo-stream.cpp:840-930) over encoder rows, with the oracle's decoder + joint"""

    def __init__(self, om):
        self.om, self.h, self.c, self.prev = om, np.zeros(1280, np.float32), np.zeros(1280, np.float32), BLANK
        self.tokens, self.lps, self.frames, self.n_frames, self.iterations = [], [], [], 0, 0

    def decode(self, enc):
        for row in np.asarray(enc, np.float32).reshape(-1, 1024):
            for _ in range(10):
                self.iterations += 1
                logits, hn, cn = self.om.decoder_joint(self.prev, self.h, self.c, row)
                best = int(np.argmax(logits))                      # first maximum
                if best == BLANK:
                    break
                x = logits.astype(np.float64)
                self.tokens.append(best)
                self.lps.append(float(x[best] - np.logaddexp.reduce(x)))
                self.frames.append(self.n_frames)
                self.prev, self.h, self.c = best, hn, cn
            self.n_frames += 1


def _stream_case(W, L, dtype, B, R, n_push, spots, options=(), seed=700):
    """one chunk per call + the tail flush; returns (engine streams' results, replays) for the spot streams"""
    T, n = 1 + R, synth.shift_samples(R)
    pcms = [synth.make_pcm(seed + b, n_push * n / 16000 + 0.35) for b in range(B)]          # + 0.35 s: a tail for finalize
    eng = capi.Engine(W, n_layers=L, dtype=dtype, max_streams=B)
    eng.set_option("token_logprobs", 1)
    for k, v in options:
        eng.set_option(k, v)
    om = ob.OracleModel(W, L)
    sts = [eng.stream(R) for _ in range(B)]
    reps = {b: Replay(om) for b in spots}
    toks = [[] for _ in range(B)]
    chunks = {b: 0 for b in spots}
    for o in range(0, pcms[0].size, n):
        for b, t in enumerate(eng.step(sts, [p[o:o + n] for p in pcms])):
            toks[b] += t
        for b in spots:
            c = sts[b].progress().chunks
            assert c - chunks[b] <= 1
            if c > chunks[b]:
                reps[b].decode(sts[b].tap(capi.TAP_ENCODER_OUT).reshape(-1, 1024)[:T])
            chunks[b] = c
    n_valid = {b: min(max((sts[b].progress().mel_frames_buffered - 9) // 8, 0), T) for b in spots}
    tail_tokens = 0
    for b, t in enumerate(eng.finalize(sts)):
        toks[b] += t
        tail_tokens += len(t)
    for b in spots:
        if n_valid[b] > 0:
            reps[b].decode(sts[b].tap(capi.TAP_ENCODER_OUT).reshape(-1, 1024)[:n_valid[b]])
    out = {}
    for b in spots:
        out[b] = dict(tokens=toks[b], frames=sts[b].token_frames(), lps=sts[b].token_logprobs(), iterations=sts[b].stats().decode_iterations)
    eng.close()
    return out, reps, dict(tail_frames=sum(n_valid.values()), tail_tokens=tail_tokens)


def _compare(got, rep, what):
    assert got["tokens"] == rep.tokens, what
    assert got["frames"] == rep.frames and got["iterations"] == rep.iterations, what
    lp = np.asarray(got["lps"], np.float64)
    assert lp.shape == (len(rep.tokens),)
    assert np.isfinite(lp).all() and (lp <= 0).all() and (lp >= -LOG_V - 1e-5).all(), what
    d = float(np.abs(lp - np.asarray(rep.lps)).max()) if lp.size else 0.0
    print(f"token_logprobs {what}: {lp.size} tokens, max |lp_engine - lp_oracle| = {d:.3e}, lp range [{lp.min() if lp.size else 0:.4f}, {lp.max() if lp.size else 0:.4f}]")
    return d, lp.size


def test_value_one_stream_small_joint_kernel(W2):
    """1 stream x R = 0: one row per step, k_dec_joint (65 parts per row), f32 and bf16 engines, the tail flush included"""
    W = _sharpened(W2, GAIN)
    worst = 0.0
    for dtype in (capi.DTYPE_F32, capi.DTYPE_BF16):
        out, reps, info = _stream_case(W, 2, dtype, 1, 0, 30, (0,))
        d, n = _compare(out[0], reps[0], f"1 x R=0 dtype {dtype}")
        assert n >= 5
        worst = max(worst, d)
    assert worst < LP_BOUND, worst


def test_value_64_streams_tiled_joint_kernel(W2):
    """64 streams x R = 13: 896 rows per step, k_dec_joint_tiled (17 parts per row); the tail flush decodes fewer frames per stream"""
    W = _sharpened(W2, GAIN)
    spots = (0, 21, 42, 63)
    out, reps, info = _stream_case(W, 2, capi.DTYPE_BF16, 64, 13, 3, spots)
    assert info["tail_frames"] > 0
    worst, total = 0.0, 0
    for b in spots:
        d, n = _compare(out[b], reps[b], f"64 x R=13 stream {b}")
        worst, total = max(worst, d), total + n
    assert total >= 20
    assert worst < LP_BOUND, worst


@pytest.mark.parametrize("R,delta", [(0, -1e9), (13, -0.2)])
def test_value_several_symbols_per_frame(W2, R, delta):
    """a blank bias that makes frames emit several symbols (-1e9: every frame runs into the 10-symbol cap, tests/test_gpu_round5.py):
    the log-probability of each symbol is taken at the decoder state of ITS iteration"""
    W = _with_blank_bias(_sharpened(W2, GAIN) if delta < -1 else W2, delta)
    out, reps, info = _stream_case(W, 2, capi.DTYPE_F32, 1, R, 4, (0,), seed=950)
    d, n = _compare(out[0], reps[0], f"blank bias {delta} R={R}")
    per_frame = np.bincount(np.asarray(reps[0].frames, np.int64))
    assert per_frame.max() >= 2 and n >= 10, per_frame
    if delta < -1:
        assert set(per_frame[per_frame > 0].tolist()) == {10}
    assert d < LP_BOUND, d


def test_value_offline_ragged_batch_over_two_decode_windows(W2):
    """one offline call, three utterances of ragged lengths, the longest spanning two 256-frame decode windows"""
    W = _sharpened(W2, GAIN)
    secs = (22.5, 8.0, 0.9)
    pcms = [synth.make_pcm(300 + i, s) for i, s in enumerate(secs)]
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    eng.set_option("token_logprobs", 1)
    eng.set_debug(True)
    toks, frames = eng.transcribe(pcms)
    om = ob.OracleModel(W, 2)
    worst, total = 0.0, 0
    for u in range(len(pcms)):
        enc = eng.offline_tap(capi.TAP_ENCODER_OUT, u)
        if u == 0:
            assert enc.shape[0] > 256
        rep = Replay(om)
        rep.decode(enc)
        got = dict(tokens=toks[u], frames=frames[u], lps=eng.offline_token_logprobs(u), iterations=rep.iterations)
        d, n = _compare(got, rep, f"offline utterance {u} ({enc.shape[0]} frames)")
        worst, total = max(worst, d), total + n
    assert total >= 20 and max(frames[0]) >= 256                     # tokens of the second window are there
    # the values belong to the LAST call
    eng.transcribe(pcms[2:])
    with pytest.raises(capi.NasrError):
        eng.offline_token_logprobs(1)
    assert eng.offline_token_logprobs(0).size == len(toks[2])
    eng.close()
    assert worst < LP_BOUND, worst


def test_end_to_end_bf16_speech_checkpoint_vs_f32_oracle_stream():
    """bf16 engine, speech checkpoint, 24 layers, 2 streams x R = 0 x 6 s against the F32 oracle's own stream (its encoder, its
    tokens).  Token sequences must be equal; a token emitted at another frame than the oracle's is scored at another frame's logits
    and is left out (at most 2 in total); for the rest max |d lp| < 0.2 (bf16 logit noise max 0.087 on this
    checkpoint, and lp is a difference of two quantities that each move by at most that)."""
    L, R, B = 24, 0, 2
    W = synth.make_weights(L, margins="speech")
    n = synth.shift_samples(R)
    pcms = [synth.make_speech_pcm(b, 6.0)[0] for b in range(B)]
    eng = capi.Engine(W, n_layers=L, dtype=capi.DTYPE_BF16, max_streams=B)
    eng.set_option("token_logprobs", 1)
    sts = [eng.stream(R) for _ in range(B)]
    toks = [[] for _ in range(B)]
    for o in range(0, pcms[0].size, n):
        for b, t in enumerate(eng.step(sts, [p[o:o + n] for p in pcms])):
            toks[b] += t
    for b, t in enumerate(eng.finalize(sts)):
        toks[b] += t
    gframes = [s.token_frames() for s in sts]
    glps = [s.token_logprobs() for s in sts]
    eng.close()
    om = ob.OracleModel(W, L)
    left_out, diffs = 0, []
    for b in range(B):
        ost = ob.OracleStream(om, R)
        sub, lay = ost.enable_taps()
        rep, ref = Replay(om), []
        for o in range(0, pcms[b].size, n):
            c0 = ost.total_chunks
            ref += ost.process(pcms[b][o:o + n])
            if ost.total_chunks > c0:
                rep.decode(lay[L - 1][:1])
        c0 = ost.total_chunks
        ref += ost.finalize()
        if ost.total_chunks > c0:
            rep.decode(lay[L - 1][:1])
        assert rep.tokens == ref and rep.frames == ost.token_frames()        # the replay IS the oracle's stream
        assert toks[b] == ref, b                                              # token-exact on this checkpoint
        assert len(ref) >= 5
        for i in range(len(ref)):
            if gframes[b][i] != rep.frames[i]:
                left_out += 1
            else:
                diffs.append(abs(float(glps[b][i]) - rep.lps[i]))
        assert np.isfinite(glps[b]).all() and (glps[b] <= 0).all() and (glps[b] >= -LOG_V - 1e-5).all()
    diffs = np.asarray(diffs)
    print(f"token_logprobs end to end bf16 vs F32 oracle: {diffs.size} tokens compared, max |d lp| = {diffs.max():.4f}, mean = {diffs.mean():.5f}, left out = {left_out}")
    assert left_out <= 2, left_out
    assert diffs.max() < 0.2, diffs.max()


# ---- bit-for-bit properties ---------------------------------------------------------------------------------------------------------
def _run(W, B, R, n_push, options, per_call=1, seed=500, dtype=capi.DTYPE_BF16):
    n = synth.shift_samples(R) * per_call
    n_calls = n_push // per_call
    pcms = [synth.make_pcm(seed + b, n_calls * n / 16000 + 0.35) for b in range(B)]
    eng = capi.Engine(W, n_layers=2, dtype=dtype, max_streams=B)
    for k, v in options:
        eng.set_option(k, v)
    sts = [eng.stream(R) for _ in range(B)]
    toks = [[] for _ in range(B)]
    for o in range(0, pcms[0].size, n):
        for b, t in enumerate(eng.step(sts, [p[o:o + n] for p in pcms])):
            toks[b] += t
    for b, t in enumerate(eng.finalize(sts)):
        toks[b] += t
    lp_on = dict(options).get("token_logprobs", 0)
    res = dict(tokens=toks, frames=[s.token_frames() for s in sts], iterations=[s.stats().decode_iterations for s in sts],
               state=[s.tap(capi.TAP_DEC_STATE).tobytes() for s in sts],
               lps=[s.token_logprobs() for s in sts] if lp_on else None,
               graph_replays=eng.counter("graph_replays"), pipelined=eng.counter("pipelined_steps"))
    eng.close()
    return res


def _same_decode(a, b):
    return a["tokens"] == b["tokens"] and a["frames"] == b["frames"] and a["iterations"] == b["iterations"] and a["state"] == b["state"]


def _same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a["lps"], b["lps"]))


@pytest.mark.parametrize("B,R,n_push", [(1, 0, 24), (64, 13, 3)])
def test_option_changes_nothing_but_adds_the_values_and_is_deterministic(W2, B, R, n_push):
    W = _sharpened(W2, GAIN)
    on = (("token_logprobs", 1),)
    off = _run(W, B, R, n_push, ())
    base = _run(W, B, R, n_push, on)
    assert sum(len(t) for t in base["tokens"]) >= 5 and base["graph_replays"] > 0
    assert _same_decode(off, base)                                             # tokens, frames, iteration counts, decoder state: bit-identical to the option off
    eager = _run(W, B, R, n_push, on + (("graph", 0),))
    assert eager["graph_replays"] == 0 and _same_decode(base, eager) and _same_bits(base, eager)      # graph replay == eager launches
    pipe = _run(W, B, R, n_push, on + (("pipeline", 4),))
    assert pipe["pipelined"] > 0 and _same_decode(base, pipe) and _same_bits(base, pipe)              # pipelined == synchronous
    again = _run(W, B, R, n_push, on)
    assert _same_bits(base, again)                                             # a second engine: no run-to-run variation
    if B == 1:
        # multi-chunk pushes put several frames of the stream into one decode (another row count, possibly another joint kernel): the
        # same tokens, values within the bound of the value tests
        # (f32 engines: at bf16 the encoder GEMMs of another row count round differently, which is not the decode's doing)
        base32 = _run(W, B, R, n_push, on, dtype=capi.DTYPE_F32)
        multi = _run(W, B, R, n_push, on, per_call=4, dtype=capi.DTYPE_F32)
        assert multi["tokens"] == base32["tokens"] and multi["frames"] == base32["frames"]
        d = float(np.abs(multi["lps"][0] - base32["lps"][0]).max())
        print(f"token_logprobs multi-chunk vs chunk by chunk (f32 engine): max |d lp| = {d:.3e}")
        assert d < LP_BOUND
        grouped = _run(W, B, R, n_push, on + (("pipeline", 8),))
        assert _same_decode(base, grouped) and _same_bits(base, grouped)
    else:
        # a stream alone (14 rows: k_dec_joint) and in the batch of 64 (896 rows: k_dec_joint_tiled)
        # (f32 engines, as above)
        base32 = _run(W, B, R, n_push, on, dtype=capi.DTYPE_F32)
        alone = _run(W, 1, R, n_push, on, dtype=capi.DTYPE_F32)
        assert alone["tokens"][0] == base32["tokens"][0] and alone["frames"][0] == base32["frames"][0]
        d = float(np.abs(alone["lps"][0] - base32["lps"][0]).max())
        print(f"token_logprobs stream alone vs in a batch of 64 (f32 engine): max |d lp| = {d:.3e}")
        assert d < LP_BOUND


def test_range_ring_reset_and_errors(W2):
    """every value finite and in [-ln 1025 - 1e-5, 0]; first / count clip like the frames; reset restarts the numbering; a token older
    than the 4096-token ring is refused; the option is taken only before the first step and the getters name it when it is off"""
    R, T = 13, 14
    W = _with_blank_bias(_sharpened(W2, GAIN), -1e9)                          # ten tokens per frame: the ring wraps quickly
    n = synth.shift_samples(R) * 8                                             # eight chunks per call = 1 120 tokens
    pcm = synth.make_pcm(77, 4 * n / 16000 + 0.05)
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=2)
    eng.set_option("token_logprobs", 0)
    eng.set_option("token_logprobs", 1)
    with pytest.raises(capi.NasrError, match="token_logprobs must be 0 or 1"):
        eng.set_option("token_logprobs", 2)
    st = eng.stream(R)
    toks = eng.step([st], [pcm[:n]], tok_cap=2048)[0]
    assert len(toks) % 10 == 0 and len(toks) >= 7 * T * 10           # the first push completes seven or eight chunks
    with pytest.raises(capi.NasrError, match="token_logprobs must be set before the first step"):
        eng.set_option("token_logprobs", 0)
    lps = st.token_logprobs()
    assert lps.size == len(toks) and np.isfinite(lps).all() and (lps <= 0).all() and (lps >= -LOG_V - 1e-5).all()
    assert np.unique(lps).size > 100                                           # values, not a fill pattern
    # first / count clipping as for the frames
    assert st.token_logprobs(10, 5).tobytes() == lps[10:15].tobytes() and len(st.token_frames(10, 5)) == 5
    assert st.token_logprobs(len(toks) - 3, 50).tobytes() == lps[-3:].tobytes() and len(st.token_frames(len(toks) - 3, 50)) == 3
    assert st.token_logprobs(len(toks), 4).size == 0 and st.token_logprobs(len(toks) + 7, 4).size == 0
    with pytest.raises(capi.NasrError, match="negative"):
        st.token_logprobs(-1, 2)
    # past the ring
    for k in range(1, 4):
        toks += eng.step([st], [pcm[k * n:(k + 1) * n]], tok_cap=2048)[0]
    assert len(toks) > 4096 + 100
    with pytest.raises(capi.NasrError, match="older than the 4096-token device ring"):
        st.token_logprobs(0, 1)
    with pytest.raises(capi.NasrError, match="older than the 4096-token device ring"):
        st.token_frames(0, 1)
    recent = st.token_logprobs(len(toks) - 4096, 4096)
    assert recent.size == 4096 and np.isfinite(recent).all() and (recent <= 0).all() and (recent >= -LOG_V - 1e-5).all()
    # reset restarts the numbering
    st.reset()
    assert st.token_logprobs().size == 0
    again = eng.step([st], [pcm[:n]], tok_cap=2048)[0]
    assert again == toks[:len(again)]
    assert st.token_logprobs().tobytes() == lps.tobytes()
    eng.close()
    # option off: both getters fail and name the option
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    st = eng.stream(0)
    eng.step([st], [pcm[:1280 * 4]])
    with pytest.raises(capi.NasrError, match="token_logprobs"):
        st.token_logprobs(0, 1)
    with pytest.raises(capi.NasrError, match="token_logprobs"):
        eng.offline_token_logprobs(0)
    with pytest.raises(capi.NasrError, match="before the first step"):
        eng.set_option("token_logprobs", 1)
    eng.close()
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    eng.transcribe([pcm[:16000]])
    with pytest.raises(capi.NasrError, match="before the first step or offline call"):
        eng.set_option("token_logprobs", 1)
    eng.close()


def test_cli_confidence(tmp_path):
    """nemotron-asr-amd --confidence: the same transcript, then once more with one [d.dd] behind every word; with --timestamps both
    marks on one line"""
    import re
    n_layers = 2
    W = _sharpened(synth.make_weights(n_layers=n_layers), GAIN)
    vocab = gguf_io.synthetic_vocab()
    model = tmp_path / "model.gguf"
    gguf_io.write_gguf(model, W, gguf_io.default_hparams(n_layers=n_layers), vocab)
    pcm = synth.make_pcm(2, 5.0)
    audio = tmp_path / "a.pcm"
    pcm.tofile(audio)
    cli = str(BIN / "nemotron-asr-amd")

    def run(*flags):
        r = subprocess.run([cli, str(model), str(audio), "80", "0", "--f32", "--print-tokens", *flags], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-800:]
        return r.stdout.splitlines()

    plain = run()
    conf = run("--confidence")
    assert conf[0] == plain[0] and conf[-1] == plain[-1] and len(conf) == len(plain) + 1
    toks = [int(x) for x in plain[-1].split()[1:]]
    n_words = sum(1 for i, t in enumerate(toks) if vocab[t].startswith("▁") or i == 0)
    assert n_words >= 2
    marks = re.findall(r"\[(\d\.\d\d)\]", conf[-2])
    assert len(marks) == n_words and all(0.0 <= float(m) <= 1.0 for m in marks)
    assert re.sub(r"\[\d\.\d\d\]", "", conf[-2]) == plain[0]
    both = run("--confidence", "--timestamps")
    assert len(both) == len(plain) + 1
    assert re.findall(r"\[(\d\.\d\d)\]", both[-2]) == marks
    stamped = run("--timestamps")
    assert re.sub(r"\[\d\.\d\d\]", "", both[-2]) == stamped[-2]
