"""Stream snapshots, host side (no GPU): the C ABI declares and exports the three new entry points, the Python binding lists them with
their signatures, the counters are documented, the contract is written down and the ABI version stays 1 (additions only)."""
import ctypes as C
import inspect
import re
from pathlib import Path

from nemotron_asr_amd import capi, sharding

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
NAMES = ("nasr_engine_snapshot_bound", "nasr_stream_save", "nasr_stream_restore")


def test_header_declares_and_library_exports_the_entry_points():
    assert re.search(r"#define NASR_ABI_VERSION 1\b", HEADER)
    assert re.search(r"int\s+nasr_engine_snapshot_bound\s*\(\s*nasr_engine \*e,\s*int64_t \*bytes_out\s*\)\s*;", HEADER)
    assert re.search(r"int\s+nasr_stream_save\s*\(\s*nasr_stream \*s,\s*void \*buf,\s*int64_t cap,\s*int64_t \*bytes_out\s*\)\s*;", HEADER)
    assert re.search(r"int\s+nasr_stream_restore\s*\(\s*nasr_engine \*e,\s*const void \*buf,\s*int64_t bytes,\s*nasr_stream \*\*out\s*\)\s*;", HEADER)
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS
        getattr(L, name)                      # raises if the library does not export it
    assert capi.check_exports()
    assert L.nasr_abi_version() == 1


def test_binding_signatures_and_methods():
    L = capi.lib()
    vp, lp = C.c_void_p, C.POINTER(C.c_int64)
    assert list(L.nasr_engine_snapshot_bound.argtypes) == [vp, lp]
    assert list(L.nasr_stream_save.argtypes) == [vp, vp, C.c_int64, lp]
    assert list(L.nasr_stream_restore.argtypes) == [vp, vp, C.c_int64, C.POINTER(vp)]
    assert callable(capi.Stream.save) and callable(capi.Engine.restore) and callable(capi.Engine.snapshot_bound)
    assert list(inspect.signature(sharding.migrate).parameters) == ["stream", "dst_engine"]
    # the calls that need no device: null arguments are refused with a message, and *out is cleared
    out, n = vp(1), C.c_int64(7)
    assert L.nasr_stream_restore(None, None, 0, C.byref(out)) < 0 and out.value is None and b"null" in L.nasr_last_error()
    assert L.nasr_stream_save(None, None, 0, C.byref(n)) < 0 and b"null" in L.nasr_last_error()
    assert L.nasr_engine_snapshot_bound(None, C.byref(n)) < 0


def test_contract_and_counters_are_documented():
    doc = HEADER[HEADER.index("nasr_stream_save: writes"):HEADER.index("int nasr_engine_snapshot_bound")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)                              # the comment's line breaks are not part of the wording
    for word in ("What travels", "Identical twin", "Isolation", "Failures", "Options and graphs", "stream pool exhausted (max_streams=%d)", "integrity-checked, not authenticated",
                 "forged blob", "bounded sample", "lowest free slot", "no slot is held", "*bytes_out is still set", '"stream_saves"', '"stream_restores"'):
        assert word in doc, word
    counters_doc = HEADER[HEADER.index("/* diagnostics:"):HEADER.index("int nasr_engine_get_counter")]
    assert '"stream_saves"' in counters_doc and '"stream_restores"' in counters_doc
    design = (ROOT / "DESIGN.md").read_text()
    section = design[design.index("## 19."):]
    for word in ("k_stream_pack", "k_stream_unpack", "nasr_snapshot.h", "Out of scope", "prev_token", "boost_state", "sample"):
        assert word in section, word
    assert "stream snapshot" in (ROOT / "README.md").read_text().lower()
