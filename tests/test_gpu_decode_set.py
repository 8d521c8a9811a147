"""The order in which the five decode options are set does not matter (csrc/nasr_decode_set.h: one working set, allocated by what the
options in force require, whichever came first).

Two f32 engines get "lm_fusion", "token_logprobs", "phrase_boost", "token_alternatives" and "frame_blank_logprobs" in opposite orders, then
the same phrase set, the same language model (tests/golden/lm_tiny.arpa, restated as tests/test_gpu_greedy_lm.py restates it) and the same
weights.  Each decodes one live stream (R = 0, four one-chunk calls and the tail flush) and one offline call of two utterances of different
lengths.  Everything the decode leaves -- tokens, token frames, token log-probabilities, alternatives (ids and values) and the per-frame
blank log-probabilities -- is equal byte for byte between the two engines, on both paths."""
import math

import numpy as np
import pytest

from nemotron_asr_amd import capi, synth
from tests import lm_ref
from tests.test_gpu_boost import SEEDS, W, drive, make_pcms  # noqa: F401 (W: fixture)

pytestmark = pytest.mark.gpu

K = 4
SEED = SEEDS[(1, 0)]
ORDER = ("lm_fusion", "token_logprobs", "phrase_boost", "token_alternatives", "frame_blank_logprobs")
VALUE = {"lm_fusion": 1, "token_logprobs": 1, "phrase_boost": 64, "token_alternatives": K, "frame_blank_logprobs": 1}
PHRASES, PHRASE_BONUS = [[0, 1], [3], [700, 5]], [2.0, 1.5, 3.0]
LM_WEIGHT, LM_BONUS = 2.0, 8.0      # the bonus lifts every non-blank token: the four frames emit


def tiny_lm():
    ln10 = math.log(10.0)
    c = lambda x: float(np.float32(float(np.float32(x)) * ln10))
    BOS, EOS = lm_ref.BOS, lm_ref.EOS
    g = {(BOS,): (c(-99), c(-0.30103)), (EOS,): (c(-1.0), 0.0), (0,): (c(-0.5), c(-0.25)), (1,): (c(-0.75), c(-0.125)), (3,): (c(-1.25), c(0.0625)),
         (700,): (c(-1.5), c(-0.5)), (BOS, 0): (c(-0.25), c(-0.125)), (0, 1): (c(-0.5), c(-0.25)), (1, EOS): (c(-0.625), 0.0), (3, 700): (c(-0.875), 0.0),
         (1, 3): (c(-0.375), c(0.03125)), (BOS, 0, 1): (c(-0.125), 0.0), (0, 1, EOS): (c(-0.0625), 0.0), (0, 1, 3): (c(-0.1875), 0.0)}
    return g, 3, c(-2.5)


def run(W, order):
    eng = capi.Engine(W, n_layers=2, dtype=capi.DTYPE_F32, max_streams=1)
    for key in order:
        eng.set_option(key, VALUE[key])
    g, lm_order, unk = tiny_lm()
    eng.set_lm(g, order=lm_order, unk_logprob=unk)
    eng.set_greedy_lm_weights(LM_WEIGHT, LM_BONUS)
    eng.set_boost_phrases(PHRASES, PHRASE_BONUS)
    n = synth.shift_samples(0)
    st = eng.stream(0)
    live_tokens = drive(eng, [st], [p[:4 * n] for p in make_pcms(1, 0, 4, SEED)], 0, {})[0]
    ids, alps = st.token_alternatives()
    out = {"live tokens": live_tokens, "live frames": st.token_frames(), "live logprobs": st.token_logprobs().tobytes(),
           "live alternative ids": ids.tobytes(), "live alternative values": alps.tobytes(), "live frame blank": st.frame_blank_logprobs().tobytes()}
    toks, frames = eng.transcribe([synth.make_pcm(SEED + 1, 0.7), synth.make_pcm(SEED + 2, 0.45)])
    out["offline tokens"], out["offline frames"] = toks, frames
    for u in range(2):
        ids, alps = eng.offline_token_alternatives(u)
        out[f"offline logprobs {u}"] = eng.offline_token_logprobs(u).tobytes()
        out[f"offline alternative ids {u}"], out[f"offline alternative values {u}"] = ids.tobytes(), alps.tobytes()
        out[f"offline frame blank {u}"] = eng.offline_frame_blank_logprobs(u).tobytes()
    eng.close()
    return out


def test_option_order_does_not_matter(W):
    a = run(W, ORDER)                      # "lm_fusion" first, "token_logprobs" before "token_alternatives"
    b = run(W, ORDER[::-1])                # ... last, ... after
    n_live, n_off = len(a["live tokens"]), [len(t) for t in a["offline tokens"]]
    print(f"decode_set: {n_live} live tokens, {n_off} offline tokens, {len(a['live frame blank']) // 4} live frames")
    assert n_live >= 2 and sum(n_off) >= 2
    assert len(a["live logprobs"]) == 4 * n_live and len(a["live alternative ids"]) == 4 * K * n_live and len(a["live frame blank"]) > 0
    assert all(len(a[f"offline logprobs {u}"]) == 4 * n_off[u] and len(a[f"offline frame blank {u}"]) > 0 for u in range(2))
    assert a.keys() == b.keys()
    for what in a:
        assert a[what] == b[what], what
