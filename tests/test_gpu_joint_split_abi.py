"""Engine option "joint_split" through the C ABI: the joint's output layer as three bf16 MFMA products of split operands wherever the
decode took k_dec_joint_tiled (more than 64 rows an iteration, and the beam search), on a 2-layer bf16 engine with the speech checkpoint.  The option's
rules and counter; tokens, emission frames and N-best order equal the engine without it, streaming (8 streams x R = 13: 112 rows), offline and beam; the
log-probabilities agree within twice the split's logit bound of the row,
  (3 2^-16 + 3 640 2^-23) (|out_w| x + |out_b|) + |out_w| (u |e + g|),  x = relu(e + g),
which this file restates in float64 from the engine's own encoder rows and the oracle's prediction network (ln P = logit - lse moves by at most the
token's error plus the largest error of the row); one stream at R = 0 (k_dec_joint, at most 64 rows) is bit-identical."""
import numpy as np
import pytest

from nemotron_asr_amd import capi, synth
from oracle import binding as ob
from tests.test_gpu_parity import N_LAYERS

pytestmark = pytest.mark.gpu
BLANK = 1024
PLANE_BYTES = 65 * 20 * 2048


@pytest.fixture(scope="module")
def weights():
    return synth.make_weights(N_LAYERS, margins="speech")


def _engine(W, n_streams, on):
    eng = capi.Engine(W, n_layers=N_LAYERS, dtype=capi.DTYPE_BF16, max_streams=n_streams)
    eng.set_option("token_logprobs", 1)
    eng.set_option("joint_split", on)
    eng.set_debug(True)
    assert eng.counter("joint_plane_bytes") == (PLANE_BYTES if on else 0)
    return eng


def _stream_run(eng, pcms, R):
    """-> tokens, frames and log-probabilities of every stream, and per stream the encoder rows of every completed chunk"""
    piece, sts = synth.shift_samples(R), [eng.stream(R) for _ in pcms]
    toks, enc, chunks = [[] for _ in pcms], [[] for _ in pcms], 0
    for k in range(pcms[0].size // piece):
        for b, t in enumerate(eng.step(sts, [p[k * piece:(k + 1) * piece] for p in pcms])):
            toks[b] += t
        if sts[0].stats().chunks > chunks:
            chunks += 1
            for b, st in enumerate(sts):
                enc[b].append(st.tap(capi.TAP_ENCODER_OUT).reshape(-1, 1024)[:1 + R].copy())
    with pytest.raises(capi.NasrError, match="before the first step or offline call"):
        eng.set_option("joint_split", 0)
    out = toks, [st.token_frames() for st in sts], [np.asarray(st.token_logprobs(), np.float64) for st in sts], enc
    eng.close()
    return out


def _lp_tolerances(W, om, enc_chunks):
    """the greedy rules over one stream's encoder rows with the oracle's decoder -> its tokens and, per token, twice the largest logit bound of the row"""
    f = np.float64
    we, be, wp, bp = (W[n].astype(f) for n in ("joint.enc.weight", "joint.enc.bias", "joint.pred.weight", "joint.pred.bias"))
    awo, abo = np.abs(W["joint.joint_net.2.weight"]).astype(f), np.abs(W["joint.joint_net.2.bias"]).astype(f)
    h, c, prev, toks, tol = np.zeros(1280, np.float32), np.zeros(1280, np.float32), BLANK, [], []
    for row in np.concatenate(enc_chunks):
        for _ in range(10):
            logits, hn, cn = om.decoder_joint(prev, h, c, row)
            if int(np.argmax(logits)) == BLANK:
                break
            eg = we @ row.astype(f) + be + wp @ hn[640:].astype(f) + bp
            bound = (3 * 2.0 ** -16 + 3 * 640 * 2.0 ** -23) * (awo @ np.maximum(eg, 0) + abo) + awo @ (2.0 ** -24 * np.abs(eg))
            prev, h, c = int(np.argmax(logits)), hn, cn
            toks.append(prev)
            tol.append(2 * bound.max())
    return toks, np.array(tol)


def test_option_rules(weights):
    eng = _engine(weights, 1, 0)
    for v in (-1, 2):
        with pytest.raises(capi.NasrError, match="0 or 1"):
            eng.set_option("joint_split", v)
    eng.set_option("joint_split", 1)
    assert eng.counter("joint_plane_bytes") == PLANE_BYTES
    eng.set_option("joint_split", 0)
    assert eng.counter("joint_plane_bytes") == 0
    eng.close()


def test_streaming_tiled_branch_same_tokens_and_bounded_logprobs(weights):
    B, R, pushes = 8, 13, 4
    piece = synth.shift_samples(R)
    pcms = [synth.make_speech_pcm(b, pushes * piece / 16000.0 + 0.1)[0][:pushes * piece] for b in range(B)]
    off, on = _stream_run(_engine(weights, B, 0), pcms, R), _stream_run(_engine(weights, B, 1), pcms, R)
    assert off[0] == on[0] and off[1] == on[1] and sum(len(t) for t in on[0]) >= B
    om, worst = ob.OracleModel(weights, N_LAYERS), 0.0
    for b in range(B):
        toks, tol = _lp_tolerances(weights, om, on[3][b])
        assert toks == on[0][b] and on[2][b].shape == off[2][b].shape == tol.shape
        d = np.abs(on[2][b] - off[2][b])
        worst = max(worst, float((d / tol).max()) if len(d) else 0.0)
        assert (d <= tol).all(), (b, d, tol)
    print(f"RATIO joint_split lp: {worst:.4f} of 2 x the row's logit bound")


def test_small_kernel_is_untouched(weights):
    R, pushes = 0, 40
    piece = synth.shift_samples(R)
    pcms = [synth.make_speech_pcm(3, pushes * piece / 16000.0 + 0.1)[0][:pushes * piece]]
    off, on = _stream_run(_engine(weights, 1, 0), pcms, R), _stream_run(_engine(weights, 1, 1), pcms, R)
    assert off[0] == on[0] and off[1] == on[1] and len(on[0][0]) > 0
    assert np.array_equal(off[2][0].view(np.uint64), on[2][0].view(np.uint64))


def test_offline_and_beam_calls_equal_the_engine_without_the_option(weights):
    pcms = [synth.make_speech_pcm(b, s)[0] for b, s in ((0, 3.0), (1, 4.0))]          # 2 x 50 frames: the tiled branch
    got = []
    for on in (0, 1):
        eng = _engine(weights, 2, on)
        res = [eng.transcribe(pcms), [[h[1:3] for h in u] for u in eng.transcribe_beam(pcms, beam=2)]]
        with pytest.raises(capi.NasrError, match="before the first step or offline call"):
            eng.set_option("joint_split", 1 - on)
        eng.close()
        got.append(res)
    assert got[0] == got[1] and all(len(t) > 0 for t in got[0][0][0]) and all(len(u) > 0 for u in got[0][1])
