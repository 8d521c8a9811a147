"""The six offline entries (nasr_engine_transcribe / _align / _transcribe_beam and their _mel twins) side by side: what every one of
them does around its own work -- the empty call, the refused flag, the length limit and what a refused call leaves behind, and the PCM
entry against the mel entry fed the log-mel the PCM call produced.  Utterances of 0, 1 and 5 encoder frames; what each entry computes
is pinned by its own suite (test_gpu_offline, test_gpu_align, test_gpu_beam*)."""
import ctypes as C

import numpy as np
import pytest

from nemotron_asr_amd import capi, synth
from tests import offline_ref as orf
from tests.test_gpu_offline import mel_for

pytestmark = pytest.mark.gpu

FRAMES = (0, 1, 5)
TRANSCRIPTS = [[], [3], [3, 4]]
BEAM = dict(beam=2, max_symbols=2)
ENTRIES = ("transcribe", "transcribe_mel", "align", "align_mel", "transcribe_beam", "transcribe_beam_mel")
N_MEL_OVER = 8 * 2048


def mel_frames(n_samples):
    """log-mel frames of a whole utterance: 256 zero samples in front, 512-sample frames every 160 (nasr_offline_plan.h)"""
    return 0 if n_samples < 256 else 1 + (n_samples - 256) // 160


def samples_for(T):
    """the fewest samples that give T encoder frames"""
    n_mel = 0
    while orf.enc_frames(n_mel) < T:
        n_mel += 1
    assert orf.enc_frames(n_mel) == T
    n = 0 if n_mel == 0 else 256 + (n_mel - 1) * 160
    assert mel_frames(n) == n_mel and (n == 0 or mel_frames(n - 1) == n_mel - 1)
    return n


def is_pcm(entry):
    return not entry.endswith("_mel")


def kind(entry):
    return "align" if entry.startswith("align") else "beam" if "beam" in entry else "greedy"


def call(eng, entry, inputs, transcripts=None, flags=0):
    """the entry's result in a form that compares bit for bit"""
    fn = getattr(eng, entry)
    if kind(entry) == "greedy":
        return fn(inputs, flags=flags)
    if kind(entry) == "align":
        res = fn(inputs, TRANSCRIPTS if transcripts is None else transcripts, flags=flags)
        return [(np.float64(ll).tobytes(), np.float64(best).tobytes(), frames, lps.tobytes()) for ll, best, frames, lps in res]
    res = fn(inputs, flags=flags, **BEAM)
    return [[(np.float64(score).tobytes(), toks, frames, lps.tobytes()) for score, toks, frames, lps in hyps] for hyps in res]


def read_out_gone(eng, entry):
    """the read-out that only the entry's own kind of call leaves: gone after a refused call"""
    if kind(entry) == "align":
        with pytest.raises(capi.NasrError, match="no lattice"):
            eng.align_lattice(0)
    if kind(entry) == "beam":
        with pytest.raises(capi.NasrError, match="no beam hypotheses"):
            eng.beam_hypothesis(0, 0)


@pytest.fixture(scope="module")
def eng(weights2):
    e = capi.Engine(weights2, n_layers=2, dtype=capi.DTYPE_BF16, max_streams=1)
    e.set_debug(True)                                             # the lattice read-out and TAP_MEL need it
    yield e
    e.close()


@pytest.fixture(scope="module")
def good():
    """{pcm or not: the three utterances}"""
    rng = np.random.default_rng(29)
    mels = [np.zeros((0, 128), np.float32) if T == 0 else mel_for(T, rng) for T in FRAMES]
    pcms = [synth.make_pcm(s, (samples_for(T) if T else 100) / 16000.0) for s, T in enumerate(FRAMES)]      # T = 0: too short for one mel frame
    assert [orf.enc_frames(mel_frames(p.size)) for p in pcms] == list(FRAMES)
    return {False: mels, True: pcms}


@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_call(eng, entry):
    assert call(eng, entry, [], transcripts=[]) == (([], []) if kind(entry) == "greedy" else [])
    fn = getattr(capi.lib(), "nasr_engine_" + entry)
    if kind(entry) == "greedy":
        assert fn(eng.h, 0, None, None, None, None, None, None, None, 0) == 0
    elif kind(entry) == "align":
        assert fn(eng.h, 0, None, None, None, None, None, None, None, None, None, 0) == 0
    else:
        assert fn(eng.h, 0, None, None, None, C.byref(capi.BeamParams(2, 0, 2, 0)), None, 0) == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_no_sync_is_refused(eng, good, entry):
    with pytest.raises(capi.NasrError, match="NO_SYNC"):
        call(eng, entry, good[is_pcm(entry)], flags=capi.FLAG_NO_SYNC)


@pytest.mark.parametrize("entry", ENTRIES)
def test_over_long_input_is_refused_and_leaves_the_engine_as_it_was(eng, good, entry):
    inputs = good[is_pcm(entry)]
    before = call(eng, entry, inputs)
    assert len(before) == (2 if kind(entry) == "greedy" else len(FRAMES))
    if is_pcm(entry):
        n_mel = next(n for n in range(N_MEL_OVER + 1) if orf.enc_frames(n) == 2049)
        over = np.zeros(256 + (n_mel - 1) * 160, np.int16)
        assert orf.enc_frames(mel_frames(over.size)) == 2049 and orf.enc_frames(mel_frames(over.size - 1)) == 2048
    else:
        over = np.zeros((N_MEL_OVER, 128), np.float32)
        assert orf.enc_frames(N_MEL_OVER) == 2049
    with pytest.raises(capi.NasrError, match="2048"):
        call(eng, entry, [inputs[2], over], transcripts=[[3], [3]])
    read_out_gone(eng, entry)                                     # not asserted for the transcribe entries
    assert call(eng, entry, inputs) == before


@pytest.mark.parametrize("entry", [e for e in ENTRIES if is_pcm(e)])
def test_pcm_entry_equals_mel_entry_on_its_own_mel(eng, good, entry):
    got = call(eng, entry, good[True])
    mels = [eng.offline_tap(capi.TAP_MEL, u) for u in range(len(FRAMES))]
    assert [m.shape[0] for m in mels] == [mel_frames(p.size) for p in good[True]]
    assert call(eng, entry + "_mel", mels) == got
