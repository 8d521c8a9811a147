"""Phrase boosting, host side (no GPU): the C ABI declares and exports the two new entry points and the new flag, the option and
the counter are documented where the others are, the Python binding has the methods, and the ABI version stays 1 (additions only)."""
import re
from pathlib import Path

from nemotron_asr_amd import capi

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
NAMES = ("nasr_engine_set_boost_phrases", "nasr_stream_set_boost")


def test_header_declares_and_library_exports_the_entry_points():
    assert re.search(r"#define NASR_ABI_VERSION 1\b", HEADER)
    assert re.search(r"int\s+nasr_engine_set_boost_phrases\s*\(\s*nasr_engine \*e,\s*int n_phrases,\s*const int32_t \*const \*tokens,\s*"
                     r"const int32_t \*lens,\s*const float \*bonus\s*\)\s*;", HEADER)
    assert re.search(r"int\s+nasr_stream_set_boost\s*\(\s*nasr_stream \*s,\s*int enable\s*\)\s*;", HEADER)
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS
        getattr(L, name)                      # raises if the library does not export it
    assert capi.check_exports()
    assert L.nasr_abi_version() == 1


def test_flag_is_a_new_bit():
    flags = dict(re.findall(r"(NASR_FLAG_\w+)\s*=\s*1u << (\d+)", HEADER))
    assert flags["NASR_FLAG_NO_BOOST"] == "3" and len(set(flags.values())) == len(flags)
    assert capi.FLAG_NO_BOOST == 1 << 3


def test_option_and_counter_are_documented_and_binding_has_the_methods():
    options_comment = HEADER[:HEADER.index("int nasr_engine_set_option")]
    assert '"phrase_boost"' in options_comment
    counters_comment = HEADER[HEADER.index("int nasr_engine_set_option"):HEADER.index("int nasr_engine_get_counter")]
    assert '"boost_states"' in counters_comment
    for getter in ("int nasr_stream_get_token_logprobs", "int nasr_engine_offline_token_logprobs"):      # the new range at both getters
        comment = HEADER[:HEADER.index(getter)].rsplit("/*", 1)[1]
        assert "boost" in comment
    assert callable(capi.Stream.set_boost) and callable(capi.Engine.set_boost_phrases)


def test_option_and_counter_names_are_known_to_the_library():
    """the library's own strings: an engine cannot be created without a GPU, but the names it compares against are in its image"""
    image = Path(capi.lib()._name).read_bytes()
    for name in (b"phrase_boost\0", b"boost_states\0"):
        assert name in image
