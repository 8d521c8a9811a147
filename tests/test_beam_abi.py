"""CPU-side checks of the beam-search ABI: the three entry points are declared, exported and bound, and nasr_beam_params has the layout the
header states (no compute call, no GPU)."""
import ctypes as C
import inspect
import re
from pathlib import Path

from nemotron_asr_amd import capi

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("nasr_engine_transcribe_beam_mel", "nasr_engine_transcribe_beam", "nasr_engine_beam_hypothesis")


def test_beam_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
    L = capi.lib()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in capi.EXPORTS
        fn = getattr(L, name)                                   # AttributeError if the library does not export it
        assert fn.argtypes is not None
    assert len(L.nasr_engine_transcribe_beam_mel.argtypes) == len(L.nasr_engine_transcribe_beam.argtypes) == 8
    assert L.nasr_engine_transcribe_beam.argtypes[5] == C.POINTER(capi.BeamParams)
    assert len(L.nasr_engine_beam_hypothesis.argtypes) == 8 and L.nasr_engine_beam_hypothesis.argtypes[7] == C.POINTER(C.c_double)


def test_params_struct_layout():
    header = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
    m = re.search(r"typedef struct nasr_beam_params \{(.*?)\} nasr_beam_params;", header, re.S)
    assert m
    fields = re.findall(r"int32_t\s+(\w+);", m.group(1))
    assert fields == ["beam", "nbest", "max_symbols", "reserved"] == [f[0] for f in capi.BeamParams._fields_]
    assert C.sizeof(capi.BeamParams) == 16 and [getattr(capi.BeamParams, f).offset for f in fields] == [0, 4, 8, 12]
    assert (capi.BEAM_MAX, capi.BEAM_MAX_SYMBOLS, capi.BEAM_DEFAULT_SYMBOLS) == (8, 10, 4)
    rules = (ROOT / "nemotron-asr.cpp_amd" / "csrc" / "nasr_beam.h").read_text()
    assert re.search(r"WMAX = 8, SMAX = 10, S_DEFAULT = 4", rules)
    assert "NOT the greedy decode" in rules and "NOT the greedy decode" in header and "boosting" in rules and "NOT applied" in header


def test_python_binding_has_the_calls():
    for name in ("transcribe_beam_mel", "transcribe_beam", "beam_hypothesis"):
        assert callable(getattr(capi.Engine, name))
    assert capi.Engine.transcribe_beam_mel(None, []) == [] and capi.Engine.transcribe_beam(None, []) == []      # nothing to do: no engine call
    sig = inspect.signature(capi.Engine.transcribe_beam_mel)
    assert list(sig.parameters)[1:5] == ["mels", "beam", "nbest", "max_symbols"]
