"""ctypes binding of the C ABI in include/nemotron_asr_amd.h (the HIP engine).

This is plumbing only: every call goes straight into libnemotron_asr_amd.so.  There is no
CPU fallback: if the library is missing or no MI355X is visible the calls raise."""
from __future__ import annotations

import ctypes as C
import os
import struct
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("NASR_LIB_PATH") or HERE / "libnemotron_asr_amd.so")   # NASR_LIB_PATH: a diagnostic build of the same ABI

DTYPE_F32, DTYPE_BF16 = 0, 1
TYPE_F32, TYPE_F16, TYPE_Q4_0, TYPE_Q8_0 = 0, 1, 2, 8
FLAG_PCM_DEVICE, FLAG_NO_SYNC = 1, 2
FLAG_AUDIO_S16 = 4
DIAR_VAD_BF16 = 0x100       # OR into Diar's dtype: MarbleNet on the bf16 MFMA
DIAR_VAD_F16 = 0x200        # ... on the f16 MFMA with IEEE-half activation planes
RESET_FRESH, RESET_REFERENCE = 0, 1
TAP_MEL, TAP_SUBSAMPLED, TAP_LAYER_OUT, TAP_ENCODER_OUT, TAP_K_CACHE, TAP_V_CACHE, TAP_CONV_CACHE, TAP_DEC_STATE = range(8)
TAP_PCM16 = 8               # the 16 kHz samples the last step / step_audio / finalize call handed to the front end (debug)
AUDIO_S16, AUDIO_F32, AUDIO_MULAW, AUDIO_ALAW = range(4)
AUDIO_ENCODINGS = {"s16": AUDIO_S16, "f32": AUDIO_F32, "mulaw": AUDIO_MULAW, "alaw": AUDIO_ALAW}
AUDIO_DTYPES = {AUDIO_S16: np.int16, AUDIO_F32: np.float32, AUDIO_MULAW: np.uint8, AUDIO_ALAW: np.uint8}
AUDIO_RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)

EXPORTS = [
    "nasr_last_error", "nasr_abi_version", "nasr_tensor_to_f32", "nasr_engine_create", "nasr_engine_create_ex", "nasr_engine_destroy",
    "nasr_stream_create", "nasr_stream_reset", "nasr_stream_reset_ex", "nasr_stream_destroy", "nasr_stream_set_prompt",
    "nasr_stream_get_stats", "nasr_stream_get_progress", "nasr_stream_get_token_frames", "nasr_engine_step", "nasr_engine_step_mel", "nasr_engine_finalize",
    "nasr_engine_collect", "nasr_engine_set_option", "nasr_engine_set_debug", "nasr_stream_get_tap", "nasr_engine_profile",
    "nasr_engine_profile_read", "nasr_engine_hip_stream", "nasr_engine_lend_stream", "nasr_device_alloc", "nasr_device_free",
    "nasr_device_upload", "nasr_engine_synchronize", "nasr_engine_get_counter", "nasr_stream_debug_fill_kv",
    "nasr_diar_create", "nasr_diar_destroy", "nasr_diar_set_stream", "nasr_diar_vad", "nasr_diar_embed", "nasr_diar_logmel", "nasr_diar_last_gpu_ms",
    "nasr_engine_transcribe_mel", "nasr_engine_transcribe", "nasr_engine_offline_tap",
    "nasr_stream_get_token_logprobs", "nasr_engine_offline_token_logprobs",
    "nasr_engine_set_boost_phrases", "nasr_stream_set_boost",
    "nasr_stream_get_token_alternatives", "nasr_engine_offline_token_alternatives",
    "nasr_engine_align_mel", "nasr_engine_align", "nasr_engine_align_lattice",
    "nasr_stream_get_frame_blank_logprobs", "nasr_engine_offline_frame_blank_logprobs",
    "nasr_stream_set_audio_format", "nasr_engine_step_audio", "nasr_engine_convert_audio", "nasr_audio_out_ready", "nasr_audio_out_total",
    "nasr_engine_transcribe_beam_mel", "nasr_engine_transcribe_beam", "nasr_engine_beam_hypothesis",
    "nasr_engine_set_lm", "nasr_engine_set_lm_weights", "nasr_engine_beam_hypothesis_lm",
    "nasr_engine_beam_hypothesis_boost",
    "nasr_engine_set_greedy_lm_weights", "nasr_stream_set_lm",
    "nasr_stream_fork", "nasr_engine_preview",
    "nasr_engine_snapshot_bound", "nasr_stream_save", "nasr_stream_restore",
    "nasr_stream_history_range", "nasr_stream_get_history",
    "nasr_engine_history_transcribe", "nasr_engine_history_beam", "nasr_engine_history_align",
    "nasr_stream_get_token_entropies", "nasr_engine_offline_token_entropies",
]
HISTORY_ROW = 640                    # csrc/nasr_history.h: f32 values of one kept frame (the joint's encoder projection)
SNAPSHOT_HEADER_BYTES = 144          # csrc/nasr_snapshot.h: the mirror section follows (R first, the audio format at +60)
ALIGN_MAX_TOKENS = 1024
BEAM_MAX, BEAM_MAX_SYMBOLS, BEAM_DEFAULT_SYMBOLS = 8, 10, 4
LM_MAX_ORDER, LM_BOS, LM_EOS = 5, 1025, 1026
FLAG_NO_BOOST = 1 << 3
FLAG_BEAM_BOOST = 1 << 4
FLAG_NO_LM = 1 << 5
BOOST_MAX_STATES, BOOST_MAX_PHRASE_LEN, BOOST_MAX_BONUS = 4096, 32, 1.0e4
OFFLINE_MAX_FRAMES = 2048


class HParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_mels", "d_model", "n_heads", "d_head", "d_ff", "n_layers", "vocab_size", "decoder_dim",
        "joint_dim", "subsampling_factor", "att_left_context", "kernel_size", "num_prompts")]


class BeamParams(C.Structure):
    """nasr_beam_params: beam W in 1 .. 8, nbest N in 1 .. W (0 = W), max_symbols S in 1 .. 10 (0 = the default, 4)"""
    _fields_ = [(n, C.c_int32) for n in ("beam", "nbest", "max_symbols", "reserved")]


class LmDesc(C.Structure):
    """nasr_lm_desc: a back-off n-gram model over token ids for the beam search's shallow fusion"""
    _fields_ = [("order", C.c_int32), ("flags", C.c_int32), ("n_ngrams", C.c_int64), ("lengths", C.POINTER(C.c_int32)), ("tokens", C.POINTER(C.c_int32)),
                ("logprob", C.POINTER(C.c_float)), ("backoff", C.POINTER(C.c_float)), ("unk_logprob", C.c_float), ("weight", C.c_float),
                ("token_bonus", C.c_float), ("reserved", C.c_float)]


class WeightDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("type", C.c_int32), ("n_dims", C.c_int32),
                ("ne", C.c_int64 * 4), ("data", C.c_void_p)]


class StreamStats(C.Structure):
    _fields_ = [("samples_in", C.c_int64), ("chunks", C.c_int32), ("decode_iterations", C.c_int32),
                ("tokens", C.c_int32), ("cache_valid_len", C.c_int32), ("mel_frames_buffered", C.c_int32),
                ("reserved", C.c_int32)]


class AudioFormat(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sample_rate", "encoding", "channels", "channel")]


def audio_format(rate=16000, encoding="s16", channels=1, channel=0) -> AudioFormat:
    """channel: an index, or -1 / "mix" for the mean of the channels"""
    enc = AUDIO_ENCODINGS[encoding] if isinstance(encoding, str) else int(encoding)
    return AudioFormat(int(rate), enc, int(channels), -1 if channel == "mix" else int(channel))


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("total_ms", C.c_double),
                ("bytes", C.c_double), ("flops", C.c_double)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(f"{LIB_PATH} not built: run __graft_entry__.build() (no CPU fallback exists)")
        L = C.CDLL(str(LIB_PATH))
        vp, ip = C.c_void_p, C.POINTER(C.c_int32)
        L.nasr_last_error.restype = C.c_char_p
        L.nasr_engine_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(HParams), C.POINTER(WeightDesc), C.c_int, C.c_int]
        L.nasr_engine_create_ex.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(HParams), C.POINTER(WeightDesc), C.c_int, C.c_int, C.c_int]
        L.nasr_engine_destroy.argtypes = [vp]
        L.nasr_engine_destroy.restype = None
        L.nasr_tensor_to_f32.argtypes = [C.POINTER(WeightDesc), C.POINTER(C.c_float), C.c_int64]
        L.nasr_tensor_to_f32.restype = C.c_int64
        L.nasr_stream_create.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
        for n in ("reset", "destroy"):
            getattr(L, f"nasr_stream_{n}").argtypes = [vp]
        L.nasr_stream_set_prompt.argtypes = [vp, C.c_int]
        L.nasr_stream_reset_ex.argtypes = [vp, C.c_int]
        L.nasr_stream_debug_fill_kv.argtypes = [vp, C.c_float]
        L.nasr_stream_get_stats.argtypes = [vp, C.POINTER(StreamStats)]
        L.nasr_stream_get_progress.argtypes = [vp, C.POINTER(StreamStats)]
        L.nasr_diar_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(WeightDesc), C.c_int, C.c_int, C.c_int]
        L.nasr_diar_destroy.argtypes = [vp]
        L.nasr_diar_destroy.restype = None
        L.nasr_diar_vad.argtypes = [vp, C.c_int, C.POINTER(vp), ip, C.POINTER(vp), ip, ip, C.c_uint32]
        L.nasr_diar_embed.argtypes = [vp, C.c_int, C.POINTER(vp), ip, C.POINTER(C.c_float), C.c_uint32]
        L.nasr_diar_last_gpu_ms.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
        L.nasr_diar_logmel.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_int32, C.c_int, C.POINTER(C.c_float), C.c_int64, ip]
        L.nasr_stream_get_token_frames.argtypes = [vp, C.c_int64, C.c_int32, C.POINTER(C.c_int32)]
        L.nasr_engine_step.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), ip, C.POINTER(vp), ip, ip, C.c_uint32]
        L.nasr_engine_step_mel.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), ip, C.POINTER(vp), ip, ip, C.c_uint32]
        L.nasr_engine_finalize.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), ip, ip]
        L.nasr_engine_collect.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), ip, ip]
        L.nasr_stream_fork.argtypes = [vp, C.POINTER(vp)]
        L.nasr_engine_preview.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), ip, ip, C.POINTER(vp)]
        L.nasr_engine_snapshot_bound.argtypes = [vp, C.POINTER(C.c_int64)]
        L.nasr_stream_save.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int64)]
        L.nasr_stream_restore.argtypes = [vp, vp, C.c_int64, C.POINTER(vp)]
        L.nasr_engine_set_debug.argtypes = [vp, C.c_int]
        L.nasr_engine_set_option.argtypes = [vp, C.c_char_p, C.c_int]
        L.nasr_stream_get_tap.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int64]
        L.nasr_stream_get_tap.restype = C.c_int64
        L.nasr_engine_profile.argtypes = [vp, C.c_int]
        L.nasr_engine_profile_read.argtypes = [vp, C.POINTER(KernelStat), C.c_int]
        L.nasr_engine_hip_stream.argtypes = [vp]
        L.nasr_engine_hip_stream.restype = vp
        L.nasr_engine_lend_stream.argtypes = [vp, C.POINTER(vp)]
        L.nasr_diar_set_stream.argtypes = [vp, vp]
        L.nasr_device_alloc.argtypes = [vp, C.POINTER(vp), C.c_int64]
        L.nasr_device_free.argtypes = [vp, vp]
        L.nasr_device_upload.argtypes = [vp, vp, vp, C.c_int64]
        L.nasr_engine_synchronize.argtypes = [vp]
        L.nasr_engine_get_counter.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
        L.nasr_engine_transcribe_mel.argtypes = [vp, C.c_int, C.POINTER(vp), ip, ip, C.POINTER(vp), ip, ip, C.POINTER(vp), C.c_uint32]
        L.nasr_engine_transcribe.argtypes = [vp, C.c_int, C.POINTER(vp), ip, ip, C.POINTER(vp), ip, ip, C.POINTER(vp), C.c_uint32]
        L.nasr_engine_offline_tap.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int64]
        L.nasr_engine_offline_tap.restype = C.c_int64
        L.nasr_stream_get_token_logprobs.argtypes = [vp, C.c_int64, C.c_int32, C.POINTER(C.c_float)]
        L.nasr_engine_offline_token_logprobs.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_int32]
        L.nasr_stream_get_token_entropies.argtypes = [vp, C.c_int64, C.c_int32, C.POINTER(C.c_float)]
        L.nasr_engine_offline_token_entropies.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_int32]
        L.nasr_engine_set_boost_phrases.argtypes = [vp, C.c_int, C.POINTER(ip), ip, C.POINTER(C.c_float)]
        L.nasr_stream_set_boost.argtypes = [vp, C.c_int]
        L.nasr_stream_get_token_alternatives.argtypes = [vp, C.c_int64, C.c_int32, ip, C.POINTER(C.c_float)]
        L.nasr_engine_offline_token_alternatives.argtypes = [vp, C.c_int, ip, C.POINTER(C.c_float), C.c_int32]
        L.nasr_stream_get_frame_blank_logprobs.argtypes = [vp, C.c_int64, C.c_int32, C.POINTER(C.c_float)]
        L.nasr_engine_offline_frame_blank_logprobs.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_int32]
        dp = C.POINTER(C.c_double)
        L.nasr_engine_align_mel.argtypes = [vp, C.c_int, C.POINTER(vp), ip, ip, C.POINTER(vp), ip, dp, dp, C.POINTER(vp), C.POINTER(vp), C.c_uint32]
        L.nasr_engine_align.argtypes = [vp, C.c_int, C.POINTER(vp), ip, ip, C.POINTER(vp), ip, dp, dp, C.POINTER(vp), C.POINTER(vp), C.c_uint32]
        L.nasr_engine_align_lattice.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64]
        L.nasr_engine_align_lattice.restype = C.c_int64
        L.nasr_engine_transcribe_beam_mel.argtypes = [vp, C.c_int, C.POINTER(vp), ip, ip, C.POINTER(BeamParams), ip, C.c_uint32]
        L.nasr_engine_transcribe_beam.argtypes = [vp, C.c_int, C.POINTER(vp), ip, ip, C.POINTER(BeamParams), ip, C.c_uint32]
        L.nasr_engine_beam_hypothesis.argtypes = [vp, C.c_int, C.c_int, ip, ip, C.POINTER(C.c_float), C.c_int32, dp]
        L.nasr_engine_set_lm.argtypes = [vp, C.POINTER(LmDesc)]
        L.nasr_engine_set_lm_weights.argtypes = [vp, C.c_float, C.c_float]
        L.nasr_engine_set_greedy_lm_weights.argtypes = [vp, C.c_float, C.c_float]
        L.nasr_stream_set_lm.argtypes = [vp, C.c_int]
        L.nasr_engine_beam_hypothesis_lm.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.POINTER(C.c_float), C.c_int32]
        L.nasr_engine_beam_hypothesis_boost.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.POINTER(C.c_float), C.c_int32]
        lp = C.POINTER(C.c_int64)
        L.nasr_stream_history_range.argtypes = [vp, lp, ip]
        L.nasr_stream_get_history.argtypes = [vp, C.c_int64, C.c_int32, C.POINTER(C.c_float)]
        L.nasr_engine_history_transcribe.argtypes = [vp, C.POINTER(vp), C.c_int, lp, ip, C.POINTER(vp), ip, ip, C.POINTER(vp), C.c_uint32]
        L.nasr_engine_history_beam.argtypes = [vp, C.POINTER(vp), C.c_int, lp, ip, C.POINTER(BeamParams), ip, C.c_uint32]
        L.nasr_engine_history_align.argtypes = [vp, C.POINTER(vp), C.c_int, lp, ip, C.POINTER(vp), ip, dp, dp, C.POINTER(vp), C.POINTER(vp), C.c_uint32]
        L.nasr_stream_set_audio_format.argtypes = [vp, C.POINTER(AudioFormat)]
        L.nasr_engine_step_audio.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), ip, C.POINTER(vp), ip, ip, C.c_uint32]
        L.nasr_engine_convert_audio.argtypes = [vp, C.POINTER(AudioFormat), vp, C.c_int64, vp, C.c_int64, C.c_uint32]
        L.nasr_engine_convert_audio.restype = C.c_int64
        for n in ("ready", "total"):
            getattr(L, f"nasr_audio_out_{n}").argtypes = [C.POINTER(AudioFormat), C.c_int64]
            getattr(L, f"nasr_audio_out_{n}").restype = C.c_int64
        _lib = L
    return _lib


def audio_out_ready(fmt: AudioFormat, n_frames_in: int) -> int:
    """16 kHz samples a stream of this format has completed after n_frames_in input frames (host arithmetic, no GPU)"""
    return _chk(lib().nasr_audio_out_ready(C.byref(fmt), int(n_frames_in)))


def audio_out_total(fmt: AudioFormat, n_frames_in: int) -> int:
    """... and in all once the stream has ended (what finalize flushes is the difference)"""
    return _chk(lib().nasr_audio_out_total(C.byref(fmt), int(n_frames_in)))


def check_exports():
    """Every symbol include/nemotron_asr_amd.h declares is exported (no compute call)."""
    L = lib()
    for name in EXPORTS:
        getattr(L, name)
    assert L.nasr_abi_version() == 1
    return True


class NasrError(RuntimeError):
    pass


def _chk(rc):
    if rc < 0:
        raise NasrError(lib().nasr_last_error().decode())
    return rc


def default_hparams(n_layers=24, kernel_size=9, num_prompts=0) -> HParams:
    return HParams(n_mels=128, d_model=1024, n_heads=8, d_head=128, d_ff=4096, n_layers=n_layers,
                   vocab_size=1025, decoder_dim=640, joint_dim=640, subsampling_factor=8,
                   att_left_context=70, kernel_size=kernel_size, num_prompts=num_prompts)


class Stream:
    def __init__(self, engine: "Engine", right_context=0, prompt_index=-1, _fork_of: "Stream" = None, _blob: bytes = None):
        self.engine = engine
        h = C.c_void_p()
        if _blob is not None:
            buf = (C.c_char * len(_blob)).from_buffer_copy(_blob) if len(_blob) else None
            _chk(lib().nasr_stream_restore(engine.h, C.cast(buf, C.c_void_p), len(_blob), C.byref(h)))
            # accepted: the mirror's right_context and audio format are in their ranges
            right_context, = struct.unpack_from("<i", _blob, SNAPSHOT_HEADER_BYTES)
            fmt = AudioFormat(*struct.unpack_from("<4i", _blob, SNAPSHOT_HEADER_BYTES + 60))
            if (fmt.sample_rate, fmt.encoding, fmt.channels, fmt.channel) != (16000, AUDIO_S16, 1, 0):
                self.fmt = fmt
        elif _fork_of is None:
            _chk(lib().nasr_stream_create(engine.h, right_context, prompt_index, C.byref(h)))
        else:
            _chk(lib().nasr_stream_fork(_fork_of.h, C.byref(h)))
            self.fmt = _fork_of.fmt
        self.h = h
        self.R, self.T = right_context, 1 + right_context

    def fork(self) -> "Stream":
        """a new stream in the lowest free slot whose state is this one's at this moment (one device launch); the two are independent
        from then on and, given the same calls, give the same tokens, frames and read-outs"""
        return Stream(self.engine, self.R, _fork_of=self)

    def save(self) -> bytes:
        """the stream as one blob in host memory (nasr_stream_save: one device launch and one copy); the stream goes on living unchanged.
        Engine.restore(blob) -- of this engine, another one, another device's or a later process's -- makes its identical twin"""
        need = C.c_int64()
        lib().nasr_stream_save(self.h, None, 0, C.byref(need))          # buf == NULL: an error by contract that names the size and sets it
        if need.value <= 0:
            raise NasrError(lib().nasr_last_error().decode())
        buf = C.create_string_buffer(need.value)
        _chk(lib().nasr_stream_save(self.h, C.cast(buf, C.c_void_p), need.value, C.byref(need)))
        return buf.raw[:need.value]

    def reset(self, reference=False):
        """reference=True: nemo_stream_reset as the reference codes it (stale conv cache / preprocessor carry survive)"""
        _chk(lib().nasr_stream_reset_ex(self.h, RESET_REFERENCE if reference else RESET_FRESH))

    def set_prompt(self, prompt_index: int):
        _chk(lib().nasr_stream_set_prompt(self.h, prompt_index))

    fmt = None                      # AudioFormat once set_audio_format has succeeded (None: s16 16 kHz mono)

    def set_audio_format(self, rate, encoding="s16", channels=1, channel=0):
        """what this stream's audio looks like (before its first audio, or right after a reset); push it with Engine.step_audio"""
        f = audio_format(rate, encoding, channels, channel)
        _chk(lib().nasr_stream_set_audio_format(self.h, C.byref(f)))
        self.fmt = f

    def debug_fill_kv(self, value: float):
        """test hook: every K/V ring row of this stream's slot := +-value (stale rows must never reach a result)"""
        _chk(lib().nasr_stream_debug_fill_kv(self.h, float(value)))

    def destroy(self):
        if self.h:
            lib().nasr_stream_destroy(self.h)
            self.h = None

    def stats(self) -> StreamStats:
        s = StreamStats()
        _chk(lib().nasr_stream_get_stats(self.h, C.byref(s)))
        return s

    def progress(self) -> StreamStats:
        """host-mirror counters only: no device synchronisation"""
        s = StreamStats()
        _chk(lib().nasr_stream_get_progress(self.h, C.byref(s)))
        return s

    def token_frames(self, first=0, count=None) -> list:
        """absolute encoder-frame index (x 80 ms) of tokens [first, first + count) since create/reset"""
        if count is None:
            count = max(int(self.stats().tokens) - first, 0)
        out = np.zeros(max(count, 1), np.int32)
        n = _chk(lib().nasr_stream_get_token_frames(self.h, first, count, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out[:n].tolist()

    def token_logprobs(self, first=0, count=None) -> np.ndarray:
        """ln P(token) under the joint's softmax (blank included) of tokens [first, first + count) since create/reset, f32;
        needs engine option "token_logprobs" = 1 (set before the first step)"""
        if count is None:
            count = max(int(self.stats().tokens) - first, 0)
        out = np.zeros(max(count, 1), np.float32)
        n = _chk(lib().nasr_stream_get_token_logprobs(self.h, first, count, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out[:n].copy()

    def token_entropies(self, first=0, count=None) -> np.ndarray:
        """entropy of order alpha (nats, in [0, ln 1025]) of the joint's softmax where each of tokens [first, first + count) since
        create/reset was emitted, f32; needs engine option "token_entropy" = round(1000 alpha) (set before the first step)"""
        if count is None:
            count = max(int(self.stats().tokens) - first, 0)
        out = np.zeros(max(count, 1), np.float32)
        n = _chk(lib().nasr_stream_get_token_entropies(self.h, first, count, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out[:n].copy()

    def token_alternatives(self, first=0, count=None):
        """(ids [n][K] int32, lps [n][K] float32): the K most probable joint outputs (blank = 1024 included) where each of tokens
        [first, first + count) since create/reset was emitted, descending, with ln P under the joint's softmax; needs engine option
        "token_alternatives" = K (set before the first step)"""
        if count is None:
            count = max(int(self.stats().tokens) - first, 0)
        K = self.engine.token_alternatives
        ids = np.zeros((max(count, 1), max(K, 1)), np.int32)
        lps = np.zeros((max(count, 1), max(K, 1)), np.float32)
        n = _chk(lib().nasr_stream_get_token_alternatives(self.h, first, count, ids.ctypes.data_as(C.POINTER(C.c_int32)), lps.ctypes.data_as(C.POINTER(C.c_float))))
        return ids[:n].copy(), lps[:n].copy()

    def frame_blank_logprobs(self, first=0, count=None) -> np.ndarray:
        """ln P(blank) under the joint's softmax at the last joint evaluation of encoder frames [first, first + count) since create/reset
        (count None: up to the last frame decoded), f32; needs engine option "frame_blank_logprobs" = 1 (set before the first step)"""
        if count is None:
            count = max(_chk(lib().nasr_stream_get_frame_blank_logprobs(self.h, 0, 0, None)) - first, 0)
        out = np.zeros(max(count, 1), np.float32)
        n = _chk(lib().nasr_stream_get_frame_blank_logprobs(self.h, first, count, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out[:n].copy()

    def history_range(self):
        """(first, count): encoder frames [first, first + count) since create/reset whose encoder-projection rows this stream keeps
        (engine option "frame_history" = N, set before the first step)"""
        first, count = C.c_int64(0), C.c_int32(0)
        _chk(lib().nasr_stream_history_range(self.h, C.byref(first), C.byref(count)))
        return int(first.value), int(count.value)

    def history(self, first=0, count=None) -> np.ndarray:
        """the kept rows of frames [first, first + count), [count][640] f32 (count None: up to the last frame kept); no rows when the range
        is not wholly kept"""
        if count is None:
            f0, n = self.history_range()
            count = max(f0 + n - first, 0)
        out = np.zeros((max(count, 1), HISTORY_ROW), np.float32)
        n = _chk(lib().nasr_stream_get_history(self.h, first, count, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out[:n].copy()

    def set_boost(self, enable=True):
        """phrase boosting on / off for this stream (engine option "phrase_boost"); either way its boost history restarts"""
        _chk(lib().nasr_stream_set_boost(self.h, int(bool(enable))))

    def set_lm(self, enable=True):
        """greedy LM fusion on / off for this stream (engine option "lm_fusion"); either way its LM state restarts at the model's start"""
        _chk(lib().nasr_stream_set_lm(self.h, int(bool(enable))))

    def tap(self, which, index=0, cap=None) -> np.ndarray:
        cap = cap or 1024 * 260          # up to MAXNEW = 256 encoder frames of one launch, or a 70-row cache
        out = np.zeros(cap, np.float32)
        n = _chk(lib().nasr_stream_get_tap(self.h, which, index, out.ctypes.data_as(C.POINTER(C.c_float)), cap))
        return out[:n].copy()


def weight_descs(weights: dict):
    """name -> ndarray (F32) or (ggml type id, packed bytes, logical shape)  ->  (keep-alive list, WeightDesc array)"""
    keep, descs = [], (WeightDesc * len(weights))()
    for i, (name, v) in enumerate(weights.items()):
        if isinstance(v, tuple):
            tid, raw, shape = v
            raw = np.ascontiguousarray(raw)
        else:
            tid, raw, shape = TYPE_F32, np.ascontiguousarray(v, np.float32), v.shape
        keep.append(raw)
        d = descs[i]
        d.name = name.encode()
        d.type = tid
        d.n_dims = len(shape)
        for j, s in enumerate(reversed(shape)):     # ggml order: ne[0] fastest
            d.ne[j] = s
        for j in range(len(shape), 4):
            d.ne[j] = 1
        d.data = raw.ctypes.data
    return keep, descs


def tensor_to_f32(type_id: int, raw: np.ndarray, shape) -> np.ndarray:
    """what the engine computes with for one GGUF tensor (host-side dequantisation, no GPU)"""
    keep, descs = weight_descs({"t": (type_id, raw, tuple(shape))})
    out = np.zeros(int(np.prod(shape)), np.float32)
    n = lib().nasr_tensor_to_f32(C.byref(descs[0]), out.ctypes.data_as(C.POINTER(C.c_float)), out.size)
    if n < 0:
        raise NasrError(lib().nasr_last_error().decode())
    return out[:n].reshape(shape)


class Diar:
    """Diarization side-car (MarbleNet VAD + TitaNet-L embeddings) through the C ABI."""

    def __init__(self, weights: dict, dtype=DTYPE_BF16, max_windows=8192, max_segments=64, device=0):
        L = lib()
        keep, descs = weight_descs(weights)
        h = C.c_void_p()
        _chk(L.nasr_diar_create(C.byref(h), device, dtype, descs, len(weights), max_windows, max_segments))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().nasr_diar_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_stream(self, hip_stream):
        """run on a stream the caller owns (Engine.lend_stream): a hardware queue no ASR lane uses"""
        _chk(lib().nasr_diar_set_stream(self.h, C.c_void_p(hip_stream)))

    def vad(self, audios: list) -> list:
        """P(speech) of every 0.63 s window (10 ms shift) of each buffer (float32 in [-1, 1], or int16 PCM) -> float32 arrays"""
        B = len(audios)
        s16 = all(np.asarray(a).dtype == np.int16 for a in audios)
        bufs = [np.ascontiguousarray(a, np.int16 if s16 else np.float32) for a in audios]
        return self._vad([b.ctypes.data for b in bufs], [b.size for b in bufs], FLAG_AUDIO_S16 if s16 else 0)

    def vad_device_s16(self, ptrs: list, n_samples: list) -> list:
        """same, on s16 PCM that is already in HBM (device pointers, e.g. Engine.upload): the ASR streams' own audio"""
        return self._vad(ptrs, n_samples, FLAG_AUDIO_S16 | FLAG_PCM_DEVICE)

    def _vad(self, ptrs, sizes, flags):
        B = len(ptrs)
        n = (C.c_int32 * B)(*sizes)
        outs = [np.zeros(max(1, 1 + (sz - 10080) // 160 if sz >= 10080 else 1), np.float32) for sz in sizes]
        ap = (C.c_void_p * B)(*ptrs)
        op = (C.c_void_p * B)(*[o.ctypes.data for o in outs])
        caps = (C.c_int32 * B)(*[o.size for o in outs])
        nw = (C.c_int32 * B)()
        _chk(lib().nasr_diar_vad(self.h, B, ap, n, op, caps, nw, flags))
        return [outs[b][:nw[b]] for b in range(B)]

    def embed_device_s16(self, ptrs: list, lens: list = None) -> np.ndarray:
        """192-d embeddings of sub-segments given as device pointers to 24 000 s16 samples each"""
        S = len(ptrs)
        ln = (C.c_int32 * S)(*(lens or [24000] * S))
        ap = (C.c_void_p * S)(*ptrs)
        out = np.zeros((S, 192), np.float32)
        _chk(lib().nasr_diar_embed(self.h, S, ap, ln, out.ctypes.data_as(C.POINTER(C.c_float)), FLAG_AUDIO_S16 | FLAG_PCM_DEVICE))
        return out

    def last_gpu_ms(self, which: str) -> float:
        """device time of the last vad() / embed() call's launch sequence (HIP events on the side-car's stream)"""
        ms = C.c_float(0.0)
        _chk(lib().nasr_diar_last_gpu_ms(self.h, 0 if which == "vad" else 1, C.byref(ms)))
        return float(ms.value)

    def logmel(self, audio: np.ndarray, which: str = "vad", normalize: bool = False):
        """parity tap: diarize_compute_logmel of one buffer on the device front end -> ([80][t_padded], t_valid)"""
        a = np.ascontiguousarray(audio, np.float32)
        t_valid = a.size // 160
        t_pad = (t_valid + 15) // 16 * 16
        out = np.empty((80, t_pad), np.float32)
        tv = C.c_int32(0)
        _chk(lib().nasr_diar_logmel(self.h, 0 if which == "vad" else 1, a.ctypes.data_as(C.POINTER(C.c_float)), a.size,
                                    int(normalize), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(tv)))
        return out, tv.value

    def embed(self, segments: list, lens: list = None) -> np.ndarray:
        """192-d embeddings of 1.5 s sub-segments (each zero padded to 24 000 samples) -> [S][192]"""
        S = len(segments)
        bufs = []
        for a in segments:
            b = np.zeros(24000, np.float32)
            a = np.asarray(a, np.float32)[:24000]
            b[:a.size] = a
            bufs.append(b)
        ln = (C.c_int32 * S)(*[(lens[i] if lens else min(len(segments[i]), 24000)) for i in range(S)])
        ap = (C.c_void_p * S)(*[b.ctypes.data for b in bufs])
        out = np.zeros((S, 192), np.float32)
        _chk(lib().nasr_diar_embed(self.h, S, ap, ln, out.ctypes.data_as(C.POINTER(C.c_float)), 0))
        return out


class Engine:
    """weights: dict name -> ndarray (float32, or (type_id, raw bytes ndarray, shape) for quantised)."""

    def __init__(self, weights: dict, n_layers=24, dtype=DTYPE_BF16, max_streams=1, kernel_size=9,
                 num_prompts=0, device=0):
        L = lib()
        self.n_layers = n_layers
        hp = default_hparams(n_layers, kernel_size, num_prompts)
        keep, descs = weight_descs(weights)
        h = C.c_void_p()
        _chk(L.nasr_engine_create(C.byref(h), device, dtype, C.byref(hp), descs, len(weights), max_streams))
        self.h = h
        self._dev_allocs = []

    def close(self):
        if getattr(self, "h", None):
            lib().nasr_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def lend_stream(self) -> int:
        """the last of the engine's side-by-side HIP streams for another GPU client (Diar.set_stream); close that client first"""
        out = C.c_void_p()
        _chk(lib().nasr_engine_lend_stream(self.h, C.byref(out)))
        return out.value

    def stream(self, right_context=0, prompt_index=-1) -> Stream:
        return Stream(self, right_context, prompt_index)

    def restore(self, blob: bytes) -> Stream:
        """a new stream in the lowest free slot that continues exactly as the stream Stream.save() was called on would have"""
        return Stream(self, _blob=bytes(blob))

    def snapshot_bound(self) -> int:
        """the largest blob any stream of this engine can produce under the decode options now in force"""
        n = C.c_int64()
        _chk(lib().nasr_engine_snapshot_bound(self.h, C.byref(n)))
        return n.value

    token_alternatives = 0          # K of option "token_alternatives": the width of the rows the two alternatives getters return

    def set_option(self, key: str, value: int):
        _chk(lib().nasr_engine_set_option(self.h, key.encode(), int(value)))
        if key == "token_alternatives":
            self.token_alternatives = int(value)

    def set_debug(self, on=True):
        _chk(lib().nasr_engine_set_debug(self.h, int(on)))

    def counter(self, name: str) -> int:
        v = C.c_int64()
        _chk(lib().nasr_engine_get_counter(self.h, name.encode(), C.byref(v)))
        return v.value

    # ---- batched calls ---------------------------------------------------------------
    @staticmethod
    def _handles(streams):
        return (C.c_void_p * len(streams))(*[s.h for s in streams])

    def _tok_bufs(self, B, cap):
        bufs = [np.zeros(cap, np.int32) for _ in range(B)]
        ptrs = (C.c_void_p * B)(*[b.ctypes.data for b in bufs])
        caps = (C.c_int32 * B)(*([cap] * B))
        n = (C.c_int32 * B)()
        return bufs, ptrs, caps, n

    def _gather(self, streams, bufs, tptrs, caps, n, cap):
        """tokens of the call just made; a full buffer means more may be queued on the stream: collect until drained"""
        B = len(streams)
        out = [bufs[b][:n[b]].tolist() for b in range(B)]
        while any(n[b] >= cap for b in range(B)):
            _chk(lib().nasr_engine_collect(self.h, self._handles(streams), B, tptrs, caps, n))
            for b in range(B):
                out[b] += bufs[b][:n[b]].tolist()
        return out

    def step(self, streams, pcms, flags=0, tok_cap=None):
        """pcms: list of int16 ndarrays (host) or list of (device_ptr, n) when FLAG_PCM_DEVICE."""
        B = len(streams)
        if flags & FLAG_PCM_DEVICE:
            ptrs = (C.c_void_p * B)(*[p for p, _ in pcms])
            ns = (C.c_int32 * B)(*[n for _, n in pcms])
            total = max(n for _, n in pcms)
        else:
            arrs = [np.ascontiguousarray(p, np.int16) for p in pcms]
            ptrs = (C.c_void_p * B)(*[a.ctypes.data for a in arrs])
            ns = (C.c_int32 * B)(*[a.size for a in arrs])
            total = max(a.size for a in arrs)
        cap = tok_cap or (total // 1280 + 16) * 10
        bufs, tptrs, caps, n = self._tok_bufs(B, cap)
        _chk(lib().nasr_engine_step(self.h, self._handles(streams), B, ptrs, ns, tptrs, caps, n, flags))
        return self._gather(streams, bufs, tptrs, caps, n, cap) if not flags & FLAG_NO_SYNC else [[] for _ in range(B)]

    def step_audio(self, streams, arrays, flags=0, tok_cap=None):
        """arrays: per stream the interleaved input frames in the stream's own format (int16 / float32 / uint8 ndarrays, [frames] or
        [frames][channels]), or (device_ptr, n_frames) with FLAG_PCM_DEVICE."""
        B = len(streams)
        if flags & FLAG_PCM_DEVICE:
            ptrs = (C.c_void_p * B)(*[p for p, _ in arrays])
            frames = [int(n) for _, n in arrays]
        else:
            arrs, frames = [], []
            for s, a in zip(streams, arrays):
                f = s.fmt or audio_format()
                a = np.ascontiguousarray(a, AUDIO_DTYPES[f.encoding]).reshape(-1)
                if a.size % f.channels:
                    raise ValueError(f"{a.size} samples are not whole frames of {f.channels} channels")
                arrs.append(a)
                frames.append(a.size // f.channels)
            ptrs = (C.c_void_p * B)(*[a.ctypes.data for a in arrs])
        ns = (C.c_int32 * B)(*frames)
        cap = tok_cap or (max(frames) // 640 + 16) * 10           # 8 kHz input: 640 frames per 80 ms
        bufs, tptrs, caps, n = self._tok_bufs(B, cap)
        _chk(lib().nasr_engine_step_audio(self.h, self._handles(streams), B, ptrs, ns, tptrs, caps, n, flags))
        return self._gather(streams, bufs, tptrs, caps, n, cap) if not flags & FLAG_NO_SYNC else [[] for _ in range(B)]

    def convert_audio(self, fmt: AudioFormat, array) -> np.ndarray:
        """one-shot, stateless: a whole buffer in `fmt` -> its 16 kHz s16 samples (audio_out_total of them)"""
        a = np.ascontiguousarray(array, AUDIO_DTYPES[fmt.encoding]).reshape(-1)
        if a.size % fmt.channels:
            raise ValueError(f"{a.size} samples are not whole frames of {fmt.channels} channels")
        frames = a.size // fmt.channels
        out = np.zeros(max(audio_out_total(fmt, frames), 1), np.int16)
        n = _chk(lib().nasr_engine_convert_audio(self.h, C.byref(fmt), a.ctypes.data, frames, out.ctypes.data, out.size, 0))
        return out[:n].copy()

    def step_mel(self, streams, mels, flags=0):
        B = len(streams)
        arrs = [np.ascontiguousarray(m, np.float32) for m in mels]
        ptrs = (C.c_void_p * B)(*[a.ctypes.data for a in arrs])
        ns = (C.c_int32 * B)(*[a.shape[0] for a in arrs])
        cap = (max(a.shape[0] for a in arrs) // 8 + 16) * 10
        bufs, tptrs, caps, n = self._tok_bufs(B, cap)
        _chk(lib().nasr_engine_step_mel(self.h, self._handles(streams), B, ptrs, ns, tptrs, caps, n, flags))
        return self._gather(streams, bufs, tptrs, caps, n, cap) if not flags & FLAG_NO_SYNC else [[] for _ in range(B)]

    def finalize(self, streams):
        B = len(streams)
        bufs, tptrs, caps, n = self._tok_bufs(B, 256)
        _chk(lib().nasr_engine_finalize(self.h, self._handles(streams), B, tptrs, caps, n))
        return self._gather(streams, bufs, tptrs, caps, n, 256)

    def preview(self, streams, frames=False, cap=256):
        """the tokens finalize would add for each stream if it were called now, as a list of token lists (frames=True: a list of
        (tokens, absolute encoder frames)); the streams are not changed.  Needs len(streams) free slots"""
        B = len(streams)
        bufs, tptrs, caps, n = self._tok_bufs(B, cap)
        fbufs, fptrs, _, _ = self._tok_bufs(B, cap)
        _chk(lib().nasr_engine_preview(self.h, self._handles(streams), B, tptrs, caps, n, fptrs if frames else None))
        toks = [bufs[b][:min(n[b], cap)].tolist() for b in range(B)]
        return [(toks[b], fbufs[b][:len(toks[b])].tolist()) for b in range(B)] if frames else toks

    def collect(self, streams, cap=4096):
        B = len(streams)
        bufs, tptrs, caps, n = self._tok_bufs(B, cap)
        _chk(lib().nasr_engine_collect(self.h, self._handles(streams), B, tptrs, caps, n))
        return self._gather(streams, bufs, tptrs, caps, n, cap)

    # ---- offline full-context transcription of whole utterances --------------------------------
    def _offline(self, fn, ptrs, ns, frames_per_unit, prompts, tok_cap, flags):
        B = len(ns)
        pr = (C.c_int32 * B)(*[int(p) for p in prompts]) if prompts is not None else None
        caps_l = [tok_cap or (int(n) // frames_per_unit + 4) * 10 + 16 for n in ns]
        tb = [np.zeros(c, np.int32) for c in caps_l]
        fb = [np.zeros(c, np.int32) for c in caps_l]
        tp = (C.c_void_p * B)(*[t.ctypes.data for t in tb])
        fp = (C.c_void_p * B)(*[f.ctypes.data for f in fb])
        caps = (C.c_int32 * B)(*caps_l)
        n = (C.c_int32 * B)()
        _chk(fn(self.h, B, ptrs, (C.c_int32 * B)(*[int(v) for v in ns]), pr, tp, caps, n, fp, flags))
        k = [min(n[b], caps_l[b]) for b in range(B)]
        return [tb[b][:k[b]].tolist() for b in range(B)], [fb[b][:k[b]].tolist() for b in range(B)]

    def transcribe_mel(self, mels, prompts=None, tok_cap=None, flags=0):
        """mels: list of [n][128] float32 log-mel arrays (the preprocessor over each whole utterance).  Returns (tokens, frames):
        one list per utterance, frames = encoder-frame index of every token."""
        if len(mels) == 0:
            return [], []
        arrs = [np.ascontiguousarray(m, np.float32).reshape(-1, 128) for m in mels]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        return self._offline(lib().nasr_engine_transcribe_mel, ptrs, [a.shape[0] for a in arrs], 8, prompts, tok_cap, flags)

    def transcribe(self, pcms, prompts=None, tok_cap=None, flags=0):
        """pcms: list of int16 arrays, one whole utterance each (or (device_ptr, n) pairs with FLAG_PCM_DEVICE).  Returns (tokens, frames)."""
        if len(pcms) == 0:
            return [], []
        if flags & FLAG_PCM_DEVICE:
            ptrs = (C.c_void_p * len(pcms))(*[p for p, _ in pcms])
            ns = [n for _, n in pcms]
        else:
            arrs = [np.ascontiguousarray(p, np.int16) for p in pcms]
            ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
            ns = [a.size for a in arrs]
        return self._offline(lib().nasr_engine_transcribe, ptrs, ns, 1280, prompts, tok_cap, flags)

    def offline_tap(self, which, u, index=0):
        """after an offline call made with set_debug(True): tap `which` (TAP_MEL / TAP_SUBSAMPLED / TAP_LAYER_OUT / TAP_ENCODER_OUT) of utterance u"""
        width = 128 if which == TAP_MEL else 1024
        L = lib()
        cap = _chk(L.nasr_engine_offline_tap(self.h, which, u, index, None, 0))
        out = np.zeros(max(cap, 1), np.float32)
        n = _chk(L.nasr_engine_offline_tap(self.h, which, u, index, out.ctypes.data_as(C.POINTER(C.c_float)), cap))
        return out[:n].reshape(-1, width).copy()

    # ---- forced alignment / transcript scoring ----------------------------------------------------
    def _align(self, fn, ptrs, ns, tokens, prompts, flags):
        B = len(ns)
        if len(tokens) != B:
            raise ValueError("one transcript per utterance")
        pr = (C.c_int32 * B)(*[int(p) for p in prompts]) if prompts is not None else None
        toks = [np.ascontiguousarray(t, dtype=np.int32).reshape(-1) for t in tokens]
        tp = (C.c_void_p * B)(*[t.ctypes.data if t.size else None for t in toks])
        nt = (C.c_int32 * B)(*[t.size for t in toks])
        ll, best = np.zeros(B, np.float64), np.zeros(B, np.float64)
        fb = [np.zeros(max(t.size, 1), np.int32) for t in toks]
        lb = [np.zeros(max(t.size, 1), np.float32) for t in toks]
        fp = (C.c_void_p * B)(*[f.ctypes.data for f in fb])
        lp = (C.c_void_p * B)(*[x.ctypes.data for x in lb])
        dp = C.POINTER(C.c_double)
        self._align_n_tokens = None                            # a failed call leaves no lattice
        _chk(fn(self.h, B, ptrs, (C.c_int32 * B)(*[int(v) for v in ns]), pr, tp, nt, ll.ctypes.data_as(dp), best.ctypes.data_as(dp), fp, lp, flags))
        self._align_n_tokens = [t.size for t in toks]          # the row width of align_lattice
        return [(float(ll[b]), float(best[b]), fb[b][:toks[b].size].tolist(), lb[b][:toks[b].size].copy()) for b in range(B)]

    def align_mel(self, mels, tokens, prompts=None, flags=0):
        """forced alignment / scoring of known transcripts: mels as for transcribe_mel, tokens = one sequence of ids 0 .. 1023 per utterance.
        Returns per utterance (loglik = ln P(tokens | audio), best = the best path's score, frames = the encoder frame at which each token
        is emitted on that path, token_logprobs = ln P of each token there)."""
        if len(mels) == 0:
            return []
        arrs = [np.ascontiguousarray(m, np.float32).reshape(-1, 128) for m in mels]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        return self._align(lib().nasr_engine_align_mel, ptrs, [a.shape[0] for a in arrs], tokens, prompts, flags)

    def align(self, pcms, tokens, prompts=None, flags=0):
        """the same from int16 PCM, one whole utterance each (or (device_ptr, n) pairs with FLAG_PCM_DEVICE)"""
        if len(pcms) == 0:
            return []
        if flags & FLAG_PCM_DEVICE:
            ptrs = (C.c_void_p * len(pcms))(*[p for p, _ in pcms])
            ns = [n for _, n in pcms]
        else:
            arrs = [np.ascontiguousarray(p, np.int16) for p in pcms]
            ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
            ns = [a.size for a in arrs]
        return self._align(lib().nasr_engine_align, ptrs, ns, tokens, prompts, flags)

    _align_n_tokens = None

    def align_lattice(self, u, n_tokens=None):
        """after an align call made with set_debug(True): (lp_blank, lp_token) of utterance u, each [T][U + 1] float32.  U is the length
        of the transcript that call was given for utterance u (remembered by this object; n_tokens, if given, must agree)"""
        L = lib()
        n = _chk(L.nasr_engine_align_lattice(self.h, u, None, None, 0))
        known = self._align_n_tokens
        if known is None or not 0 <= u < len(known):
            raise NasrError(f"no lattice of utterance {u}: this object made no align call that holds it")
        if n_tokens is not None and int(n_tokens) != known[u]:
            raise ValueError(f"utterance {u} was aligned to {known[u]} tokens, not {n_tokens}")
        U = known[u]
        if n % (U + 1):
            raise NasrError(f"lattice of utterance {u}: {n} cells are no multiple of U + 1 = {U + 1}")
        b, t = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
        fp = C.POINTER(C.c_float)
        n = _chk(L.nasr_engine_align_lattice(self.h, u, b.ctypes.data_as(fp), t.ctypes.data_as(fp), n))
        return b[:n].reshape(-1, U + 1).copy(), t[:n].reshape(-1, U + 1).copy()

    # ---- beam search: N-best offline transcripts -------------------------------------------------
    def beam_hypothesis(self, u, rank):
        """hypothesis `rank` of utterance u of the last beam call: (score, tokens, frames, token_logprobs)"""
        L = lib()
        n = _chk(L.nasr_engine_beam_hypothesis(self.h, u, rank, None, None, None, 0, None))
        tok, fr, lp = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float32)
        score = C.c_double(0.0)
        ipt = C.POINTER(C.c_int32)
        n = _chk(L.nasr_engine_beam_hypothesis(self.h, u, rank, tok.ctypes.data_as(ipt), fr.ctypes.data_as(ipt), lp.ctypes.data_as(C.POINTER(C.c_float)), n, C.byref(score)))
        return float(score.value), tok[:n].tolist(), fr[:n].tolist(), lp[:n].copy()

    def beam_hypothesis_lm(self, u, rank):
        """the LM side of hypothesis `rank` of utterance u of the last beam call (made with a model attached): (lm_logprob, total,
        token_lm_logprobs) -- lm_logprob includes the EOS term when the model has one, the per-token values do not"""
        L = lib()
        n = _chk(L.nasr_engine_beam_hypothesis_lm(self.h, u, rank, None, None, None, 0))
        lps = np.zeros(max(n, 1), np.float32)
        lm, total = C.c_double(0.0), C.c_double(0.0)
        n = _chk(L.nasr_engine_beam_hypothesis_lm(self.h, u, rank, C.byref(lm), C.byref(total), lps.ctypes.data_as(C.POINTER(C.c_float)), n))
        return float(lm.value), float(total.value), lps[:n].copy()

    def beam_hypothesis_boost(self, u, rank):
        """the boost side of hypothesis `rank` of utterance u of the last beam call (made with boost=True / FLAG_BEAM_BOOST): (boost, total,
        token_bonuses) -- boost is the sum of the per-token phrase bonuses, total the key the search ranked by"""
        L = lib()
        n = _chk(L.nasr_engine_beam_hypothesis_boost(self.h, u, rank, None, None, None, 0))
        bon = np.zeros(max(n, 1), np.float32)
        boost, total = C.c_double(0.0), C.c_double(0.0)
        n = _chk(L.nasr_engine_beam_hypothesis_boost(self.h, u, rank, C.byref(boost), C.byref(total), bon.ctypes.data_as(C.POINTER(C.c_float)), n))
        return float(boost.value), float(total.value), bon[:n].copy()

    def set_lm(self, ngrams, order=0, unk_logprob=-20.0, weight=0.0, token_bonus=0.0):
        """attach a back-off n-gram language model (None detaches): every later beam call is fused with it, and with engine option "lm_fusion"
        the greedy decode of live streams and transcribe() too, by its own weights (set_greedy_lm_weights).  ngrams: {token tuple: logprob} or
        {token tuple: (logprob, backoff)} or an iterable of (tokens, logprob[, backoff]); natural logs; LM_BOS only first, LM_EOS only last.
        order 0 = the longest n-gram.  weight and token_bonus (the beam's) in [0, 100] (include/nemotron_asr_amd.h)."""
        if ngrams is None:
            _chk(lib().nasr_engine_set_lm(self.h, None))
            return
        items = []
        for it in (ngrams.items() if isinstance(ngrams, dict) else ngrams):
            toks, val = (it[0], it[1:]) if len(it) != 2 else it
            val = tuple(np.atleast_1d(np.asarray(val, np.float64)).tolist())
            items.append((tuple(int(t) for t in toks), float(val[0]), float(val[1]) if len(val) > 1 else 0.0))
        n = len(items)
        lengths = np.asarray([len(t) for t, _, _ in items], np.int32)
        tokens = np.asarray([k for t, _, _ in items for k in t] or [0], np.int32)
        lp = np.asarray([v for _, v, _ in items] or [0.0], np.float32)
        bo = np.asarray([b for _, _, b in items] or [0.0], np.float32)
        ipt, fpt = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        d = LmDesc(int(order) or int(lengths.max(initial=1)), 0, n, np.ascontiguousarray(lengths if n else np.zeros(1, np.int32)).ctypes.data_as(ipt),
                   tokens.ctypes.data_as(ipt), lp.ctypes.data_as(fpt), bo.ctypes.data_as(fpt), float(unk_logprob), float(weight), float(token_bonus), 0.0)
        _chk(lib().nasr_engine_set_lm(self.h, C.byref(d)))

    def set_lm_weights(self, weight, token_bonus=0.0):
        _chk(lib().nasr_engine_set_lm_weights(self.h, float(weight), float(token_bonus)))

    def set_greedy_lm_weights(self, weight, token_bonus=0.0):
        """the weights of the greedy decode's LM fusion (engine option "lm_fusion"), each in [0, 100]; the streams' LM states are kept"""
        _chk(lib().nasr_engine_set_greedy_lm_weights(self.h, float(weight), float(token_bonus)))

    def _beam(self, fn, ptrs, ns, beam, nbest, max_symbols, prompts, flags, lm=False, boost=False):
        if boost:
            flags |= FLAG_BEAM_BOOST
        B = len(ns)
        pr = (C.c_int32 * B)(*[int(p) for p in prompts]) if prompts is not None else None
        params = BeamParams(int(beam), int(nbest), int(max_symbols), 0)
        nh = (C.c_int32 * B)()
        _chk(fn(self.h, B, ptrs, (C.c_int32 * B)(*[int(v) for v in ns]), pr, C.byref(params), nh, flags))
        def one(b, r):
            h = self.beam_hypothesis(b, r)
            if lm:
                h += self.beam_hypothesis_lm(b, r)
            if boost:
                h += self.beam_hypothesis_boost(b, r)
            return h
        return [[one(b, r) for r in range(nh[b])] for b in range(B)]

    def transcribe_beam_mel(self, mels, beam=4, nbest=0, max_symbols=0, prompts=None, flags=0, lm=False, boost=False):
        """frame-synchronous beam search over whole utterances (mels as for transcribe_mel): per utterance the list, best first, of
        (score, tokens, frames, token_logprobs) of its nbest distinct transcripts (nbest 0 = beam; max_symbols 0 = the default).  Beam 1
        is not the greedy decode (include/nemotron_asr_amd.h).  lm=True (a model is attached, set_lm): each tuple gains (lm_logprob, total,
        token_lm_logprobs).  boost=True (engine option "phrase_boost", set_boost_phrases): the search is boosted (FLAG_BEAM_BOOST) and each
        tuple gains, after the LM fields, (boost, total, token_bonuses); without it phrase boosting is not applied."""
        if len(mels) == 0:
            return []
        arrs = [np.ascontiguousarray(m, np.float32).reshape(-1, 128) for m in mels]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        return self._beam(lib().nasr_engine_transcribe_beam_mel, ptrs, [a.shape[0] for a in arrs], beam, nbest, max_symbols, prompts, flags, lm, boost)

    def transcribe_beam(self, pcms, beam=4, nbest=0, max_symbols=0, prompts=None, flags=0, lm=False, boost=False):
        """the same from int16 PCM, one whole utterance each (or (device_ptr, n) pairs with FLAG_PCM_DEVICE)"""
        if len(pcms) == 0:
            return []
        if flags & FLAG_PCM_DEVICE:
            ptrs = (C.c_void_p * len(pcms))(*[p for p, _ in pcms])
            ns = [n for _, n in pcms]
        else:
            arrs = [np.ascontiguousarray(p, np.int16) for p in pcms]
            ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
            ns = [a.size for a in arrs]
        return self._beam(lib().nasr_engine_transcribe_beam, ptrs, ns, beam, nbest, max_symbols, prompts, flags, lm, boost)

    # ---- second pass over live streams' frame history (engine option "frame_history") -------------------
    def _history_fn(self, fn, streams, windows):
        """fn with the argument order of its offline twin: (engine, B, -, count[], -, ...) -> fn(engine, streams, B, first[], count[], ...)"""
        if len(windows) != len(streams):
            raise ValueError("one (first, count) window per stream")
        handles = self._handles(streams)
        firsts = (C.c_int64 * len(streams))(*[int(f) for f, _ in windows])
        return lambda h, B, _ptrs, counts, _prompts, *rest: fn(h, handles, B, firsts, counts, *rest)

    def history_transcribe(self, streams, windows, tok_cap=None, flags=0):
        """greedy second pass: a fresh decode of window (first, count) of each stream's kept frames, as transcribe() decodes an utterance.
        Returns (tokens, frames), frames relative to the window's first frame.  The same stream may appear several times."""
        if len(streams) == 0:
            return [], []
        fn = self._history_fn(lib().nasr_engine_history_transcribe, streams, windows)
        return self._offline(fn, None, [c for _, c in windows], 1, None, tok_cap, flags)

    def history_beam(self, streams, windows, beam=4, nbest=0, max_symbols=0, flags=0, lm=False, boost=False):
        """beam second pass over the windows: what transcribe_beam() returns, frames relative to each window's first frame"""
        if len(streams) == 0:
            return []
        fn = self._history_fn(lib().nasr_engine_history_beam, streams, windows)
        return self._beam(fn, None, [c for _, c in windows], beam, nbest, max_symbols, None, flags, lm, boost)

    def history_align(self, streams, windows, tokens, flags=0):
        """forced alignment / scoring of one transcript per window: what align() returns, frames relative to each window's first frame"""
        if len(streams) == 0:
            return []
        fn = self._history_fn(lib().nasr_engine_history_align, streams, windows)
        return self._align(fn, None, [c for _, c in windows], tokens, None, flags)

    def set_boost_phrases(self, phrases, bonus=None):
        """replace the engine's boost set (engine option "phrase_boost" = state capacity): phrases = sequences of 1 .. 32 non-blank token
        ids, bonus = one float for all or one per phrase, 0 < bonus <= 1e4 in natural-log units; () clears the set.  Resets every
        stream's boost history."""
        phrases = [np.ascontiguousarray(p, dtype=np.int32).reshape(-1) for p in phrases]
        n = len(phrases)
        if n == 0:
            _chk(lib().nasr_engine_set_boost_phrases(self.h, 0, None, None, None))
            return
        w = np.asarray(bonus, np.float32)
        w = np.ascontiguousarray(np.full(n, w, np.float32) if w.ndim == 0 else w)
        if bonus is None or w.shape != (n,):
            raise ValueError("bonus: one float, or one per phrase")
        ptrs = (C.POINTER(C.c_int32) * n)(*[p.ctypes.data_as(C.POINTER(C.c_int32)) for p in phrases])
        lens = np.asarray([p.size for p in phrases], np.int32)
        _chk(lib().nasr_engine_set_boost_phrases(self.h, n, ptrs, lens.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(C.POINTER(C.c_float))))

    def offline_token_alternatives(self, u):
        """(ids [n][K] int32, lps [n][K] float32) of every token of utterance u of the last offline call (engine option "token_alternatives" = K)"""
        L = lib()
        n = _chk(L.nasr_engine_offline_token_alternatives(self.h, u, None, None, 0))
        K = max(self.token_alternatives, 1)
        ids = np.zeros((max(n, 1), K), np.int32)
        lps = np.zeros((max(n, 1), K), np.float32)
        n = _chk(L.nasr_engine_offline_token_alternatives(self.h, u, ids.ctypes.data_as(C.POINTER(C.c_int32)), lps.ctypes.data_as(C.POINTER(C.c_float)), n))
        return ids[:n].copy(), lps[:n].copy()

    def offline_token_logprobs(self, u) -> np.ndarray:
        """ln P(token) of every token of utterance u of the last offline call (engine option "token_logprobs" = 1)"""
        L = lib()
        cap = _chk(L.nasr_engine_offline_token_logprobs(self.h, u, None, 0))
        out = np.zeros(max(cap, 1), np.float32)
        n = _chk(L.nasr_engine_offline_token_logprobs(self.h, u, out.ctypes.data_as(C.POINTER(C.c_float)), cap))
        return out[:n].copy()

    def offline_token_entropies(self, u) -> np.ndarray:
        """the entropy at every token of utterance u of the last offline greedy call (engine option "token_entropy" = round(1000 alpha))"""
        L = lib()
        cap = _chk(L.nasr_engine_offline_token_entropies(self.h, u, None, 0))
        out = np.zeros(max(cap, 1), np.float32)
        n = _chk(L.nasr_engine_offline_token_entropies(self.h, u, out.ctypes.data_as(C.POINTER(C.c_float)), cap))
        return out[:n].copy()

    def offline_frame_blank_logprobs(self, u) -> np.ndarray:
        """ln P(blank) at the last joint evaluation of every encoder frame of utterance u of the last offline call (engine option
        "frame_blank_logprobs" = 1)"""
        L = lib()
        cap = _chk(L.nasr_engine_offline_frame_blank_logprobs(self.h, u, None, 0))
        out = np.zeros(max(cap, 1), np.float32)
        n = _chk(L.nasr_engine_offline_frame_blank_logprobs(self.h, u, out.ctypes.data_as(C.POINTER(C.c_float)), cap))
        return out[:n].copy()

    # ---- measurement ------------------------------------------------------------------
    def profile(self, on=True):
        _chk(lib().nasr_engine_profile(self.h, int(on)))

    def profile_read(self):
        arr = (KernelStat * 64)()
        n = _chk(lib().nasr_engine_profile_read(self.h, arr, 64))
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches, total_ms=arr[i].total_ms,
                     bytes=arr[i].bytes, flops=arr[i].flops) for i in range(min(n, 64))]

    def synchronize(self):
        _chk(lib().nasr_engine_synchronize(self.h))

    def upload(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        _chk(lib().nasr_device_alloc(self.h, C.byref(p), arr.nbytes))
        _chk(lib().nasr_device_upload(self.h, p, arr.ctypes.data, arr.nbytes))
        self._dev_allocs.append(p)
        return p.value
