"""CPU-side checks of the forced-alignment ABI: the three entry points are declared, exported and bound (no compute call, no GPU)."""
import ctypes as C
import re
from pathlib import Path

from nemotron_asr_amd import capi

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("nasr_engine_align_mel", "nasr_engine_align", "nasr_engine_align_lattice")


def test_align_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
    L = capi.lib()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in capi.EXPORTS
        fn = getattr(L, name)                                   # AttributeError if the library does not export it
        assert fn.argtypes is not None
    assert len(L.nasr_engine_align_mel.argtypes) == len(L.nasr_engine_align.argtypes) == 12
    assert L.nasr_engine_align_mel.argtypes[7] == C.POINTER(C.c_double)
    assert L.nasr_engine_align_lattice.restype is C.c_int64 and len(L.nasr_engine_align_lattice.argtypes) == 5
    m = re.search(r"#define\s+NASR_ALIGN_MAX_TOKENS\s+(\d+)", header)
    assert m and int(m.group(1)) == capi.ALIGN_MAX_TOKENS == 1024


def test_python_binding_has_the_calls():
    for name in ("align_mel", "align", "align_lattice"):
        assert callable(getattr(capi.Engine, name))
    assert capi.Engine.align_mel(None, [], []) == [] and capi.Engine.align(None, [], []) == []       # nothing to do: no engine call
