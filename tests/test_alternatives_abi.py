"""Top-K token alternatives, host side (no GPU): the C ABI declares and exports the two new entry points, the Python binding lists
them and has the methods, the option is documented with its neighbours, and the ABI version stays 1 (additions only)."""
import re
from pathlib import Path

from nemotron_asr_amd import capi

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
NAMES = ("nasr_stream_get_token_alternatives", "nasr_engine_offline_token_alternatives")


def test_header_declares_and_library_exports_the_entry_points():
    assert re.search(r"#define NASR_ABI_VERSION 1\b", HEADER)
    assert re.search(r"int\s+nasr_stream_get_token_alternatives\s*\(\s*const nasr_stream \*s,\s*int64_t first,\s*int32_t count,\s*int32_t \*ids_out,\s*float \*logprobs_out\s*\)\s*;", HEADER)
    assert re.search(r"int\s+nasr_engine_offline_token_alternatives\s*\(\s*nasr_engine \*e,\s*int u,\s*int32_t \*ids_out,\s*float \*logprobs_out,\s*int32_t cap\s*\)\s*;", HEADER)
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS
        getattr(L, name)                      # raises if the library does not export it
    assert capi.check_exports()
    assert L.nasr_abi_version() == 1


def test_option_is_documented_and_binding_has_the_methods():
    options_comment = HEADER[:HEADER.index("int nasr_engine_set_option")]
    assert '"token_alternatives"' in options_comment and '"token_logprobs"' in options_comment and '"phrase_boost"' in options_comment
    assert callable(capi.Stream.token_alternatives) and callable(capi.Engine.offline_token_alternatives)


def test_cli_usage_names_the_flag():
    src = (ROOT / "nemotron-asr.cpp_amd" / "host" / "transcribe_stream.cpp").read_text()
    usage = src[src.index("static void usage"):src.index("int main")]
    assert "--alternatives K" in usage and "alt <i> <id>:<p>" in usage
