"""CPU-side checks of the greedy LM fusion's ABI (no compute call, no GPU): the two entry points and NASR_FLAG_NO_LM are declared, exported and
bound with the flag in the next free bit; the setters refuse a null handle with a message; the range and missing-option refusals are worded
like their phrase-boost counterparts (their behaviour on a live engine is in tests/test_gpu_greedy_lm.py::test_rejections); and the three
command-line tools take --lm without --beam: given a model file that does not exist they get as far as loading it instead of stopping at
their usage text."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

import pytest

from nemotron_asr_amd import capi

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "nemotron-asr.cpp_amd"
BIN = PKG / "bin"
NAMES = ("nasr_engine_set_greedy_lm_weights", "nasr_stream_set_lm")


def test_symbols_and_the_flag_are_declared_exported_and_bound():
    header = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
    L = capi.lib()
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in capi.EXPORTS
    assert L.nasr_engine_set_greedy_lm_weights.argtypes[1:] == [C.c_float, C.c_float]
    assert L.nasr_stream_set_lm.argtypes[1:] == [C.c_int]
    assert callable(capi.Engine.set_greedy_lm_weights) and callable(capi.Stream.set_lm)
    assert list(inspect.signature(capi.Engine.set_greedy_lm_weights).parameters)[1:] == ["weight", "token_bonus"]
    assert "beam only" not in (capi.Engine.set_lm.__doc__ or "") and "lm_fusion" in capi.Engine.set_lm.__doc__
    flags = {m.group(1): 1 << int(m.group(2)) for m in re.finditer(r"(NASR_FLAG_\w+)\s*=\s*1u << (\d+)", header)}
    flags.update({m.group(1): int(m.group(2), 16) for m in re.finditer(r"(NASR_FLAG_\w+)\s*=\s*(0x[0-9a-fA-F]+)u", header)})
    assert flags["NASR_FLAG_NO_LM"] == 1 << 5 == max(flags.values()) and sorted(flags.values()) == [1 << b for b in range(6)]      # the next free bit
    assert capi.FLAG_NO_LM == 1 << 5 and capi.FLAG_NO_LM not in (capi.FLAG_NO_BOOST, capi.FLAG_BEAM_BOOST)
    assert L.nasr_abi_version() == 1
    capi.check_exports()


def test_setters_refuse_null_handles_and_word_their_errors_like_boosting():
    L = capi.lib()
    L.nasr_last_error.restype = C.c_char_p
    assert L.nasr_engine_set_greedy_lm_weights(None, 1.0, 0.0) < 0 and b"null engine" in L.nasr_last_error()
    assert L.nasr_stream_set_lm(None, 1) < 0 and b"null stream" in L.nasr_last_error()
    abi = (PKG / "csrc" / "nasr_abi.hip").read_text()
    assert abi.count('engine option \\"lm_fusion\\" is off (set it to 1 before the first step or offline call)') == 2
    # the refusal of a late change exists once, for every decode option, and "lm_fusion" is one of the options routed to it
    assert abi.count('"%s must be set before the first step or offline call (the decode kernels are already chosen)", key') == 1
    routed = re.search(r"DECODE_OPTIONS\[\] = \{([^}]*)\};", abi).group(1)
    assert '"lm_fusion"' in routed and "else if (is_decode_option(key)) { ApiGuard api_guard; if (set_decode_option(e, key, value)) return -1; }" in abi
    assert "NASR_FLAG_NO_LM belongs to the offline entries; a stream is switched with nasr_stream_set_lm" in abi
    rules = (PKG / "csrc" / "nasr_lm.h").read_text()
    for name in ("struct Greedy", "NASR_LP_HD float lmbias", "NASR_LP_HD int32_t greedy_start", "STATE_DISABLED = -1", "ROW_COLS = 1040"):
        assert name in rules, name


@pytest.mark.parametrize("tool,args", [("nemotron-transcribe-amd", ["a.pcm"]), ("nemotron-asr-amd", ["a.pcm", "80", "0"]), ("nemo-server-amd", [])])
def test_clis_accept_lm_without_beam(tmp_path, tool, args):
    exe = BIN / tool
    assert exe.exists(), "build() makes the host tools"
    (tmp_path / "a.pcm").write_bytes(b"\0" * 3200)
    lm = ["--lm", str(ROOT / "tests" / "golden" / "lm_tiny.arpa"), "--lm-weight", "0.5", "--token-bonus", "1"]
    r = subprocess.run([str(exe), str(tmp_path / "missing.gguf")] + [str(tmp_path / a) if a.endswith(".pcm") else a for a in args] + lm,
                       capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 1
    assert "Usage" not in r.stderr and "Unknown flag" not in r.stderr and "goes with --beam" not in r.stderr, r.stderr[-600:]
    assert "model" in r.stderr.lower(), r.stderr[-600:]          # it got as far as loading the model
    r = subprocess.run([str(exe), str(tmp_path / "missing.gguf")] + [str(tmp_path / a) if a.endswith(".pcm") else a for a in args] + lm[2:],
                       capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 1 and "go with --lm" in r.stderr       # the weights alone are refused before anything is loaded


def test_offline_cli_wants_an_explicit_weight_for_the_greedy_decode(tmp_path):
    """nemotron-transcribe-amd --lm without --beam and without --lm-weight: 0.5 is the beam search's default and the greedy decode's own is 0,
    so the tool asks for the weight instead of guessing one -- before it loads anything, and no longer with "--lm goes with --beam" """
    (tmp_path / "a.pcm").write_bytes(b"\0" * 3200)
    r = subprocess.run([str(BIN / "nemotron-transcribe-amd"), str(tmp_path / "missing.gguf"), str(tmp_path / "a.pcm"), "--lm", str(ROOT / "tests" / "golden" / "lm_tiny.arpa")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "needs --lm-weight" in r.stderr and "goes with --beam" not in r.stderr and "model" not in r.stderr.lower().replace("language model", "")
