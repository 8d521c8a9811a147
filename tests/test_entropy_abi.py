"""Entropy-based token confidence (engine option "token_entropy"), host side (no GPU): the two getters are declared with the stated
signatures, exported and bound; the option, its values and the snapshot sentence are documented; the getters fail cleanly -- a message,
no crash -- on null arguments; the host mirror and both command-line tools know the measure.  What needs an engine -- the option's
accepted and refused values on a live engine, the refusal after the decode has started, the getters' error when the option is off, the
range checks -- is in tests/test_gpu_entropy.py, as engines need a device; the rule for the values itself (nasr_ent::valid_milli) is
checked on the host in tests/test_entropy_math.py."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

from nemotron_asr_amd import capi

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "nemotron_asr_amd.h").read_text()
HOST = ROOT / "nemotron-asr.cpp_amd" / "host"
BIN = ROOT / "nemotron-asr.cpp_amd" / "bin"
NAMES = ("nasr_stream_get_token_entropies", "nasr_engine_offline_token_entropies")


def _decl(text):
    return r"\s*".join(re.escape(tok) for tok in re.findall(r"\w+|[^\w\s]", text))


def test_header_declares_the_stated_signatures():
    assert re.search(r"#define NASR_ABI_VERSION 1\b", HEADER)              # an added getter does not move the version (as the last ones did not)
    for decl in ("int nasr_stream_get_token_entropies(const nasr_stream *s, int64_t first, int32_t count, float *out);",
                 "int nasr_engine_offline_token_entropies(nasr_engine *e, int u, float *out, int32_t cap);"):
        assert re.search(_decl(decl), HEADER), decl


def test_library_exports_and_binding():
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS
        assert getattr(L, name).argtypes is not None                       # AttributeError if the library does not export it
    assert capi.check_exports() and L.nasr_abi_version() == 1
    fp = C.POINTER(C.c_float)
    assert list(L.nasr_stream_get_token_entropies.argtypes) == [C.c_void_p, C.c_int64, C.c_int32, fp]
    assert list(L.nasr_engine_offline_token_entropies.argtypes) == [C.c_void_p, C.c_int, fp, C.c_int32]
    # the same shapes as the log-probability getters beside them
    assert list(L.nasr_stream_get_token_entropies.argtypes) == list(L.nasr_stream_get_token_logprobs.argtypes)
    assert list(L.nasr_engine_offline_token_entropies.argtypes) == list(L.nasr_engine_offline_token_logprobs.argtypes)
    assert list(inspect.signature(capi.Stream.token_entropies).parameters) == list(inspect.signature(capi.Stream.token_logprobs).parameters) == ["self", "first", "count"]
    assert list(inspect.signature(capi.Engine.offline_token_entropies).parameters) == ["self", "u"]


def test_null_arguments_fail_with_a_message():
    L = capi.lib()
    out = (C.c_float * 4)()
    for name, call in (("stream", lambda: L.nasr_stream_get_token_entropies(None, 0, 4, out)), ("stream, no buffer", lambda: L.nasr_stream_get_token_entropies(None, 0, 0, None)),
                       ("offline", lambda: L.nasr_engine_offline_token_entropies(None, 0, out, 4))):
        assert call() < 0, name
        assert "null" in L.nasr_last_error().decode().lower(), name


def test_option_values_and_contracts_are_documented():
    options = HEADER[:HEADER.index("int nasr_engine_set_option")]
    text = options[options.index('"token_entropy" (0 default'):]
    text = text[:text.index('"frame_history" (0 default')]
    for word in ("round(1000 alpha)", "1000 = Shannon", "333", "50 .. 900", "1100 .. 4000", "refused", "REJECTED", "bit-identical"):
        assert word in text, word
    snap = HEADER[HEADER.index("nasr_stream_save: writes"):HEADER.index("int nasr_engine_snapshot_bound")]
    assert "token_entropy" in snap
    getter = HEADER[HEADER.index("per-token entropy"):HEADER.index("int nasr_stream_get_token_entropies")]
    assert "[0, ln 1025]" in getter and "MODEL" in getter and "4096" in getter
    abi = (ROOT / "nemotron-asr.cpp_amd" / "csrc" / "nasr_abi.hip").read_text()
    assert re.search(r'DECODE_OPTIONS\[\] = \{[^}]*"token_entropy"', abi)  # taken before the first decode, with the other decode options
    rule = (ROOT / "nemotron-asr.cpp_amd" / "csrc" / "nasr_entropy.h").read_text()
    assert "MILLI_MIN = 50" in rule and "MILLI_MAX = 4000" in rule and "BAND_LO = 900" in rule and "BAND_HI = 1100" in rule


def test_host_mirror_and_tools_know_the_measure():
    mirror = (HOST / "nemo_amd.h").read_text()
    assert "bool nemo_set_token_entropy(nemo_context *ctx, float alpha);" in mirror
    assert "std::vector<float> nemo_stream_get_token_entropies(nemo_stream_context *sctx);" in mirror
    for tool in ("nemotron-asr-amd", "nemotron-transcribe-amd"):
        r = subprocess.run([str(BIN / tool)], capture_output=True, text=True, timeout=30)      # no arguments: the usage text
        assert r.returncode != 0
        for flag in ("--confidence-method", "--confidence-alpha", "--confidence-norm", "--confidence-agg", "max_prob|entropy|tsallis", "lin|exp", "min|mean|prod"):
            assert flag in r.stderr, (tool, flag)
