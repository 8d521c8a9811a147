"""The audio input conversion's entry points are exported, and the two count functions -- host arithmetic -- work without a GPU."""
import ctypes as C

import pytest

import __graft_entry__ as ge
from tests import resample_ref as rr


@pytest.fixture(scope="module")
def capi():
    ge.load_package()
    from nemotron_asr_amd import capi
    return capi


def test_new_symbols_are_exported(capi):
    for name in ("nasr_stream_set_audio_format", "nasr_engine_step_audio", "nasr_engine_convert_audio", "nasr_audio_out_ready", "nasr_audio_out_total"):
        assert name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert capi.check_exports()
    assert capi.TAP_PCM16 == 8 and (capi.AUDIO_S16, capi.AUDIO_F32, capi.AUDIO_MULAW, capi.AUDIO_ALAW) == (0, 1, 2, 3)
    assert C.sizeof(capi.AudioFormat) == 16


def test_counts_without_a_gpu(capi):
    for fin in rr.RATES:
        f = capi.audio_format(fin, "f32", 2, "mix")
        for n in list(range(0, 400)) + [17920, 53760, 10 ** 9]:
            assert capi.audio_out_ready(f, n) == rr.out_ready(fin, n)
            assert capi.audio_out_total(f, n) == rr.out_total(fin, n)
    f = capi.audio_format(16000)
    assert capi.audio_out_ready(f, 1234) == capi.audio_out_total(f, 1234) == 1234
    # 2 ms at 48 kHz, 4 ms at 8 kHz
    assert capi.audio_out_ready(capi.audio_format(48000), 97) == 1 and capi.audio_out_ready(capi.audio_format(48000), 96) == 0
    assert capi.audio_out_ready(capi.audio_format(8000), 33) == 1 and capi.audio_out_ready(capi.audio_format(8000), 32) == 0


@pytest.mark.parametrize("bad", [(12345, "s16", 1, 0), (0, "s16", 1, 0), (48000, 4, 1, 0), (48000, -1, 1, 0), (48000, "s16", 0, 0),
                                 (48000, "s16", 9, 0), (48000, "s16", 2, 2), (48000, "s16", 2, -2)])
def test_bad_formats_are_refused(capi, bad):
    f = capi.audio_format(*bad)
    for fn in (capi.audio_out_ready, capi.audio_out_total):
        with pytest.raises(capi.NasrError):
            fn(f, 100)
    with pytest.raises(capi.NasrError):
        capi.audio_out_ready(capi.audio_format(48000), -1)
