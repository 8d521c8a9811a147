"""Frame history of live streams (engine option "frame_history"), host side (no GPU): the five entry points are declared with the stated
signatures, exported and bound; the option, its values, its memory and the fork / snapshot sentences are documented; every entry fails
cleanly -- a message, no crash -- on null arguments.  What needs an engine (the option's accepted and refused values, the entries on an
engine without the option) is in tests/test_gpu_history.py, as engines need a device."""
import ctypes as C
import re
from pathlib import Path

from nemotron_asr_amd import capi

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
NAMES = ("nasr_stream_history_range", "nasr_stream_get_history", "nasr_engine_history_transcribe", "nasr_engine_history_beam", "nasr_engine_history_align")


def _decl(text):
    """a declaration as a regular expression: any white space where the text has some"""
    return r"\s*".join(re.escape(tok) for tok in re.findall(r"\w+|[^\w\s]", text))


def test_header_declares_the_stated_signatures():
    assert re.search(r"#define NASR_ABI_VERSION 1\b", HEADER)
    for decl in (
        "int nasr_stream_history_range(const nasr_stream *s, int64_t *first_out, int32_t *count_out);",
        "int nasr_stream_get_history(const nasr_stream *s, int64_t first, int32_t count, float *out);",
        "int nasr_engine_history_transcribe(nasr_engine *e, nasr_stream *const *streams, int B, const int64_t *first, const int32_t *count, "
        "int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens, int32_t *const *frames_out, uint32_t flags);",
        "int nasr_engine_history_beam(nasr_engine *e, nasr_stream *const *streams, int B, const int64_t *first, const int32_t *count, "
        "const nasr_beam_params *params, int32_t *n_hyps, uint32_t flags);",
        "int nasr_engine_history_align(nasr_engine *e, nasr_stream *const *streams, int B, const int64_t *first, const int32_t *count, "
        "const int32_t *const *tokens, const int32_t *n_tokens, double *loglik_out, double *best_out, int32_t *const *frames_out, "
        "float *const *token_logprobs_out, uint32_t flags);",
    ):
        assert re.search(_decl(decl), HEADER), decl


def test_library_exports_and_binding():
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS
        assert getattr(L, name).argtypes is not None          # AttributeError if the library does not export it
    assert capi.check_exports() and L.nasr_abi_version() == 1
    assert [len(getattr(L, n).argtypes) for n in NAMES] == [3, 4, 10, 8, 12]
    assert L.nasr_engine_history_beam.argtypes[3] == C.POINTER(C.c_int64) and L.nasr_engine_history_beam.argtypes[5] == C.POINTER(capi.BeamParams)
    for name in ("history_range", "history"):
        assert callable(getattr(capi.Stream, name))
    for name in ("history_transcribe", "history_beam", "history_align"):
        assert callable(getattr(capi.Engine, name))
    assert capi.Engine.history_transcribe(None, [], []) == ([], []) and capi.Engine.history_beam(None, [], []) == [] and capi.Engine.history_align(None, [], [], []) == []
    assert capi.HISTORY_ROW == 640


def test_option_counters_and_contracts_are_documented():
    options = HEADER[:HEADER.index("int nasr_engine_set_option")]
    at = options.index('"frame_history"')
    text = options[at:]
    assert "64 .. 2048" in text and "multiples of 64" in text and "2 560" in text and "2.7 GB" in text and "REJECTED" in text
    counters = HEADER[HEADER.index("int nasr_engine_set_boost_phrases"):HEADER.index("int nasr_engine_get_counter")]
    assert '"history_calls"' in counters and '"history_frames"' in counters
    fork = HEADER[HEADER.index("nasr_stream_fork: *out"):HEADER.index("int nasr_stream_fork")]
    snap = HEADER[HEADER.index("nasr_stream_save: writes"):HEADER.index("int nasr_engine_snapshot_bound")]
    assert '"frame_history"' in fork and "empty" in fork and '"frame_history"' in snap and "does not travel" in snap
    rules = (ROOT / "nemotron-asr.cpp_amd" / "csrc" / "nasr_history.h").read_text()
    for name in ("retained(", "window_kept(", "ring_runs("):
        assert name in rules


def test_null_arguments_fail_with_a_message():
    L = capi.lib()
    first, count = C.c_int64(0), C.c_int32(0)
    one = (C.c_int32 * 1)(0)
    calls = {
        "range": lambda: L.nasr_stream_history_range(None, C.byref(first), C.byref(count)),
        "get": lambda: L.nasr_stream_get_history(None, 0, 0, None),
        "transcribe": lambda: L.nasr_engine_history_transcribe(None, None, 1, None, None, None, None, one, None, 0),
        "beam": lambda: L.nasr_engine_history_beam(None, None, 1, None, None, None, one, 0),
        "align": lambda: L.nasr_engine_history_align(None, None, 1, None, None, None, one, None, None, None, None, 0),
    }
    for name, call in calls.items():
        assert call() < 0, name
        msg = L.nasr_last_error().decode()
        assert "null" in msg.lower(), (name, msg)
