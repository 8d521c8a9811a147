"""CPU-side checks of the boosted beam search's ABI (no compute call, no GPU): nasr_engine_beam_hypothesis_boost is declared, exported and
bound; NASR_FLAG_BEAM_BOOST sits on the next free bit of the step-flags enum; the ABI version and nasr_beam_params are what they were; the
header, nasr_beam.h and capi state that boosting is applied in flagged beam calls only."""
import ctypes as C
import inspect
import re
from pathlib import Path

from nemotron_asr_amd import capi

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "nemotron-asr.cpp_amd"


def test_symbol_flag_and_version():
    header = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
    L = capi.lib()
    name = "nasr_engine_beam_hypothesis_boost"
    assert re.search(rf"\b{name}\s*\(", header) and name in capi.EXPORTS
    dp = C.POINTER(C.c_double)
    assert L.nasr_engine_beam_hypothesis_boost.argtypes == [C.c_void_p, C.c_int, C.c_int, dp, dp, C.POINTER(C.c_float), C.c_int32]
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"(NASR_FLAG_\w+)\s*=\s*1u << (\d+)", header)}
    assert flags["NASR_FLAG_BEAM_BOOST"] == 4 and sorted(flags.values()) == [0, 1, 2, 3, 4]           # the next free bit
    assert capi.FLAG_BEAM_BOOST == 1 << 4 and capi.FLAG_NO_BOOST == 1 << 3
    assert L.nasr_abi_version() == 1
    assert [f[0] for f in capi.BeamParams._fields_] == ["beam", "nbest", "max_symbols", "reserved"] and C.sizeof(capi.BeamParams) == 16
    assert callable(capi.Engine.beam_hypothesis_boost)
    for fn in (capi.Engine.transcribe_beam_mel, capi.Engine.transcribe_beam):
        par = inspect.signature(fn).parameters
        assert par["boost"].default is False and list(par)[-2:] == ["lm", "boost"]


def test_the_three_statements_are_updated():
    header = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
    beam = (PKG / "csrc" / "nasr_beam.h").read_text()
    py = (PKG / "capi.py").read_text()
    assert "NOT applied in beam calls" not in header and "NOT applied unless the call carries" in header and "Phrase boosting is not applied:" not in beam and "phrase boosting is not applied (include" not in py
    for text in (header, beam):
        assert "NASR_FLAG_BEAM_BOOST" in text and "No retraction" in text or "no retraction" in text
    assert "prune_allowed" in beam and "boost_states" in beam and "expand_boost" in beam
