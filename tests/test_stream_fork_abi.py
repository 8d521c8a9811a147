"""Stream fork and tail preview, host side (no GPU): the C ABI declares and exports the two new entry points, the Python binding lists
them with their signatures, the counters are documented and the ABI version stays 1 (additions only)."""
import ctypes as C
import re
from pathlib import Path

from nemotron_asr_amd import capi

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
NAMES = ("nasr_stream_fork", "nasr_engine_preview")


def test_header_declares_and_library_exports_the_entry_points():
    assert re.search(r"#define NASR_ABI_VERSION 1\b", HEADER)
    assert re.search(r"int\s+nasr_stream_fork\s*\(\s*nasr_stream \*src,\s*nasr_stream \*\*out\s*\)\s*;", HEADER)
    assert re.search(r"int\s+nasr_engine_preview\s*\(\s*nasr_engine \*e,\s*nasr_stream \*const \*streams,\s*int B,\s*int32_t \*const \*tokens_out,\s*"
                     r"const int32_t \*tokens_cap,\s*int32_t \*n_tokens,\s*int32_t \*const \*frames_out\s*\)\s*;", HEADER)
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS
        getattr(L, name)                      # raises if the library does not export it
    assert capi.check_exports()
    assert L.nasr_abi_version() == 1


def test_binding_signatures_and_methods():
    L = capi.lib()
    vp, ip = C.c_void_p, C.POINTER(C.c_int32)
    assert list(L.nasr_stream_fork.argtypes) == [vp, C.POINTER(vp)]
    assert list(L.nasr_engine_preview.argtypes) == [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), ip, ip, C.POINTER(vp)]
    assert callable(capi.Stream.fork) and callable(capi.Engine.preview)


def test_contract_and_counters_are_documented():
    fork_doc = HEADER[HEADER.index("nasr_stream_fork:"):HEADER.index("int nasr_stream_fork")]
    for word in ("inherits", "Identical twin", "Isolation", "Failures", "stream pool exhausted (max_streams=%d)", "allocates nothing"):
        assert word in fork_doc, word
    preview_doc = HEADER[HEADER.index("nasr_engine_preview:"):HEADER.index("int nasr_engine_preview")]
    for word in ("free slots", "dropped", "frames_out", "0 tokens"):
        assert word in preview_doc, word
    counters_doc = HEADER[HEADER.index("/* diagnostics:"):HEADER.index("int nasr_engine_get_counter")]
    assert '"stream_forks"' in counters_doc and '"stream_previews"' in counters_doc
