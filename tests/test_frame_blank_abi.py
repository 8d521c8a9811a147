"""Per-frame blank log-probabilities, host side (no GPU): the C ABI declares and exports the two new entry points, the Python
binding lists them, the option is documented and the ABI version stays 1 (additions only)."""
import re
from pathlib import Path

from nemotron_asr_amd import capi

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
NAMES = ("nasr_stream_get_frame_blank_logprobs", "nasr_engine_offline_frame_blank_logprobs")


def test_header_declares_and_library_exports_the_entry_points():
    assert re.search(r"#define NASR_ABI_VERSION 1\b", HEADER)
    assert re.search(r"int\s+nasr_stream_get_frame_blank_logprobs\s*\(\s*const nasr_stream \*s,\s*int64_t first,\s*int32_t count,\s*float \*out\s*\)\s*;", HEADER)
    assert re.search(r"int\s+nasr_engine_offline_frame_blank_logprobs\s*\(\s*nasr_engine \*e,\s*int u,\s*float \*out,\s*int32_t cap\s*\)\s*;", HEADER)
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS
        getattr(L, name)                      # raises if the library does not export it
    assert capi.check_exports()
    assert L.nasr_abi_version() == 1


def test_option_is_documented_and_binding_has_the_methods():
    options_comment = HEADER[:HEADER.index("int nasr_engine_set_option")]
    assert '"frame_blank_logprobs"' in options_comment
    assert callable(capi.Stream.frame_blank_logprobs) and callable(capi.Engine.offline_frame_blank_logprobs)


def test_endpoint_header_is_pure_host_code():
    src = (ROOT / "nemotron-asr.cpp_amd" / "csrc" / "nasr_endpoint.h").read_text()
    assert "hip" not in src.replace("HIP so that", "").lower()
    for name in ("struct Config", "struct State", "struct Event", "inline bool advance"):
        assert name in src
