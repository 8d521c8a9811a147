/*
 * nemotron_asr_amd.h -- C ABI of the MI355X-native streaming Conformer-ASR forward path.
 *
 * Drop-in boundary for the hot path of m1el/nemotron-asr.cpp.  The
 * reference has no plugin/FFI seam: the seam is the set of call sites where its stream
 * manager touches ggml compute.  Each entry point below names the reference interface
 * it replaces (paths relative to the reference root).  Plain pointers and sizes only;
 * no C++ / torch types cross this boundary.  INTEGRATION.md shows the reference-side
 * binding a maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; nasr_last_error() gives the text
 *     (reference convention: nullptr/false/"" + fprintf(stderr); we never abort or throw)
 *   - an engine and its streams belong to ONE host thread (reference: one worker thread owns all
 *     backend state, src/nemo-server.cpp:6-10); one engine per GPU.  Several engines may live in
 *     one process, each on its own thread (the calls are serialised only while a step graph is
 *     being captured); nasr_last_error() is per thread
 *   - a push may carry any number of samples: when it completes several chunks of a stream they
 *     run as one launch sequence (up to 256 encoder frames per stream), with the results of
 *     chunk-by-chunk calls
 *   - PCM is s16le 16 kHz mono (src/transcribe_stream.cpp:13); mel is [frames][128] f32
 *     row-major (src/preprocessor.cpp:370-381); encoder out is [T][1024] f32
 *     (src/nemo-stream.cpp:1073-1075); tokens are int32 ids in [0, vocab-1)
 *   - all streams passed to one call must share right_context (static shapes per R,
 *     src/nemo-stream.h:15-20); each stream keeps its own caches and decoder state
 */
#ifndef NEMOTRON_ASR_AMD_H
#define NEMOTRON_ASR_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NASR_ABI_VERSION 1

typedef struct nasr_engine nasr_engine; /* device weights + stream pool  (reference: nemo_context, src/nemo-ggml.h:240-252) */
typedef struct nasr_stream nasr_stream; /* per-stream device state       (reference: nemo_stream_context, src/nemo-stream.h:177-262) */

/* compute dtype of the encoder GEMMs / caches */
enum { NASR_DTYPE_F32 = 0, NASR_DTYPE_BF16 = 1 };

/* tensor element types arriving at the seam = GGUF/ggml type ids
 * (scripts/convert_to_gguf.py:30-57).  Q8_0/Q4_0/F16 are dequantised at upload. */
enum { NASR_TYPE_F32 = 0, NASR_TYPE_F16 = 1, NASR_TYPE_Q4_0 = 2, NASR_TYPE_Q8_0 = 8 };

/* step flags */
enum {
    NASR_FLAG_PCM_DEVICE = 1u << 0, /* pcm[] are device pointers (inputs already resident in HBM) */
    NASR_FLAG_NO_SYNC    = 1u << 1, /* do not copy tokens back / synchronise; poll with nasr_engine_collect() */
    NASR_FLAG_AUDIO_S16  = 1u << 2, /* nasr_diar_*: audio[] point at s16 PCM (sample / 32768), e.g. the ASR streams' own buffers */
    NASR_FLAG_NO_BOOST   = 1u << 3, /* nasr_engine_transcribe / _transcribe_mel only: decode the utterances of this call without phrase boosting */
    NASR_FLAG_BEAM_BOOST = 1u << 4, /* nasr_engine_transcribe_beam / _beam_mel only: apply the engine's boost phrases inside the search (needs "phrase_boost") */
    NASR_FLAG_NO_LM      = 0x20u,   /* bit 5; nasr_engine_transcribe / _transcribe_mel only: decode the utterances of this call without greedy LM fusion ("lm_fusion") */
};

/* model hyper-parameters = the `nemo.*` GGUF keys read at src/nemo-ggml.cpp:108-142
 * (+ kernel_size inferred from conv_dw_w->ne[1], :357-360) */
typedef struct nasr_hparams {
    int32_t n_mels;             /* 128  */
    int32_t d_model;            /* 1024 */
    int32_t n_heads;            /* 8    */
    int32_t d_head;             /* 128  */
    int32_t d_ff;               /* 4096 */
    int32_t n_layers;           /* 24   */
    int32_t vocab_size;         /* 1025 (blank = vocab_size-1) */
    int32_t decoder_dim;        /* 640  */
    int32_t joint_dim;          /* 640  */
    int32_t subsampling_factor; /* 8    */
    int32_t att_left_context;   /* 70   */
    int32_t kernel_size;        /* 9    */
    int32_t num_prompts;        /* 0 (English) or 128 (multilingual) */
} nasr_hparams;

/* one host tensor handed over by the GGUF loader: replaces the
 * fread -> ggml_backend_tensor_set upload loop of src/nemo-ggml.cpp:257-283.
 * ne[] is in ggml order (ne[0] fastest), names are the PyTorch names of :296-398. */
typedef struct nasr_weight_desc {
    const char *name;
    int32_t     type;   /* NASR_TYPE_* */
    int32_t     n_dims;
    int64_t     ne[4];
    const void *data;   /* host memory, only read during nasr_engine_create */
} nasr_weight_desc;

/* host utility, no GPU involved: the f32 values nasr_engine_create derives from one GGUF tensor at upload (F16 / Q8_0 /
 * Q4_0 are dequantised: d * q per block of 32, layouts of scripts/convert_to_gguf.py:118-204).  Returns the number of
 * elements written or < 0. */
int64_t nasr_tensor_to_f32(const nasr_weight_desc *t, float *out, int64_t cap);

typedef struct nasr_stream_stats {
    int64_t samples_in;        /* PCM samples pushed                                       */
    int32_t chunks;            /* encoder steps run      (nemo_stream_context::total_chunks_processed) */
    int32_t decode_iterations; /* LSTM+joint evaluations (::total_decode_iterations)       */
    int32_t tokens;            /* tokens emitted so far                                    */
    int32_t cache_valid_len;   /* (::cache_valid_len)                                      */
    int32_t mel_frames_buffered;
    int32_t reserved;
} nasr_stream_stats;

/* per-kernel-class timing collected with HIP events when profiling is enabled */
typedef struct nasr_kernel_stat {
    char     name[48];
    int64_t  launches;
    double   total_ms;
    double   bytes;   /* algorithmic bytes moved by those launches (weights + activations) */
    double   flops;   /* algorithmic FLOPs of those launches */
} nasr_kernel_stat;

const char *nasr_last_error(void);
int nasr_abi_version(void);

/* ---- engine: replaces nemo_init_with_backend's device side (src/nemo-ggml.cpp:448-495:
 * backend init :35-81, tensor upload :238-292 incl. compute_pos_emb :17-32, :288-292)
 * and nemo_free (:521-540).  max_streams sizes the per-stream state pool. ------------- */
int  nasr_engine_create(nasr_engine **out, int device_id, int dtype, const nasr_hparams *hp,
                        const nasr_weight_desc *weights, int n_weights, int max_streams);
/* the same with the row capacity of one launch sequence stated: workspace_rows >= max_streams x 14 lets a call hand several whole chunks of EVERY
 * stream to the engine at once (B streams x G chunks x (1 + right_context) rows <= workspace_rows): a server working off a backlog then runs
 * GEMMs of G times the rows (host/nemo_server.cpp --backlog-chunks).  0 = the default, max(max_streams x 14, 256).  ~45 KB of HBM per row and step in flight. */
int  nasr_engine_create_ex(nasr_engine **out, int device_id, int dtype, const nasr_hparams *hp,
                           const nasr_weight_desc *weights, int n_weights, int max_streams, int workspace_rows);
void nasr_engine_destroy(nasr_engine *e);

/* ---- streams: replaces nemo_stream_init (src/nemo-stream.cpp:696-733 -> ::init :36-93:
 * zeroed K/V/conv caches :320-325, decoder state zero + prev_token = blank :55-56,
 * 9 zero mel frames :73-74, cache_valid_len = 0 :81), nemo_stream_reset (:1307-1311),
 * nemo_stream_free (:1313-1317), nemo_stream_set_language (:735-749). ------------------ */
int nasr_stream_create(nasr_engine *e, int right_context, int prompt_index, nasr_stream **out);
/* reset == a fresh stream: one launch clears the conv caches, decoder state, mel / audio buffers; the K/V rows go out of
 * sight behind cache_valid_len = 0 (results bit-identical to a new engine's: tests/test_gpu_parity.py) */
int nasr_stream_reset(nasr_stream *s);
/* nemo_stream_reset AS CODED in the reference (src/nemo-stream.cpp:95-115, :31-34, :1307-1311): transcript, decoder state,
 * mel buffer (9 zero frames), cache_valid_len and the counters are reset, but the conv cache and the K/V rows are left as
 * they are (stale K/V is hidden by the validity mask, the stale conv cache is NOT: the first kernel_size-1 frames after the
 * reset see it) and the per-stream preprocessor keeps its carry (un-framed samples, last_sample).  NASR_RESET_REFERENCE
 * reproduces exactly that; the host mirror's nemo_stream_reset() uses it. */
enum { NASR_RESET_FRESH = 0, NASR_RESET_REFERENCE = 1 };
int nasr_stream_reset_ex(nasr_stream *s, int mode);
int nasr_stream_destroy(nasr_stream *s);
int nasr_stream_set_prompt(nasr_stream *s, int prompt_index);
int nasr_stream_get_stats(const nasr_stream *s, nasr_stream_stats *out);
/* the host-mirror part of the stats only (samples_in, chunks, cache_valid_len, mel_frames_buffered; reserved = tokens decoded
 * but not yet handed over; decode_iterations = tokens = -1): no device synchronisation, no copy, does not complete a
 * pipelined step in flight -- for per-call bookkeeping on a server's hot path.  Like every call on a stream it belongs to the
 * engine's ONE host thread (it reads the host mirrors nasr_engine_step mutates, without a lock) */
int nasr_stream_get_progress(const nasr_stream *s, nasr_stream_stats *out);
/* timed_token.frame_idx (src/nemo-ggml.h:383-395; time = frame * 1280 / 16000 s): absolute encoder-frame
 * index of tokens [first, first + count) of this stream, counted from create/reset.  Only the most recent
 * 4096 tokens are kept on the device.  Returns the number written, < 0 on error. */
int nasr_stream_get_token_frames(const nasr_stream *s, int64_t first, int32_t count, int32_t *frames_out);
/* per-token confidence (the reference has no such output): ln P(token) of tokens [first, first + count) of this stream under the
 * joint's softmax over all 1025 outputs, at the frame and decoder state where each was emitted; f32, in [-ln 1025, 0] because the
 * token is the arg-max.  With phrase boosting (engine option "phrase_boost") the value stays the MODEL's probability, ln softmax of the raw
 * logits at the chosen token: a boosted token need not be the raw arg-max, so the range is then (-inf, 0] (any finite value <= 0).  Same contract as nasr_stream_get_token_frames: completes steps in flight, tokens counted from create/reset,
 * only the most recent 4096 kept, returns the number written, < 0 on error -- also when engine option "token_logprobs" is off. */
int nasr_stream_get_token_logprobs(const nasr_stream *s, int64_t first, int32_t count, float *out);
/* per-token entropy (the reference has no such output; engine option "token_entropy" = round(1000 alpha)): for tokens [first, first + count)
 * of this stream the entropy of order alpha, in nats, of the joint's softmax over all 1025 outputs at the frame and decoder state where each
 * was emitted -- alpha = 1: -sum p ln p (Shannon), else ln(sum p^alpha) / (1 - alpha) (Renyi; Tsallis follows from it, host/token_confidence.h).
 * f32 in [0, ln 1025].  With phrase boosting or LM fusion it stays the MODEL's (raw logits).  Same contract as
 * nasr_stream_get_token_logprobs: completes steps in flight, tokens counted from create/reset, only the most recent 4096 kept, returns the
 * number written, < 0 on error -- also when engine option "token_entropy" is off. */
int nasr_stream_get_token_entropies(const nasr_stream *s, int64_t first, int32_t count, float *out);
/* per-token alternatives (the reference has no such output; engine option "token_alternatives" = K): for tokens [first, first + count) of
 * this stream the K largest of the 1025 joint outputs (blank included: a blank among them means the model nearly emitted nothing there) at
 * the frame and decoder state where each token was emitted, as ids and ln P under the joint's softmax.  Descending logit, among equal logit
 * bits the lower id first -- the arg-max's tie rule, so without phrase boosting entry 0 is the token and its value is the token's
 * nasr_stream_get_token_logprobs value bit for bit; with boosting the ranking stays the MODEL's (raw logits) and the token need not be entry
 * 0, nor among the K.
 * [count][K] row-major; same contract as nasr_stream_get_token_logprobs: completes steps in flight, tokens counted from
 * create/reset, only the most recent 4096 kept, returns the number of TOKENS written, < 0 on error (also when the option is off) */
int nasr_stream_get_token_alternatives(const nasr_stream *s, int64_t first, int32_t count, int32_t *ids_out, float *logprobs_out);
/* per-frame blank log-probabilities (the reference has no such output; engine option "frame_blank_logprobs" = 1): for encoder frames
 * [first, first + count) of this stream, counted from create/reset (both reset modes restart the count at 0), ln P(blank) under the joint's
 * softmax over all 1025 outputs at the LAST joint evaluation the greedy decode made on that frame: usually the one where blank won, the value
 * then in [-ln 1025, 0]; on a frame left by the cap of 10 symbols the evaluation that emitted the 10th, the value then any finite number <= 0.
 * With phrase boosting it stays the MODEL's probability (blank never gets a bonus).  Frames of the nasr_engine_finalize tail are included.
 * Same contract as nasr_stream_get_token_logprobs: completes steps in flight, returns the number written, < 0 on error -- also when the option
 * is off.  Only the most recent 4096 frames are kept: a range whose first frame is older returns 0.  With out == NULL it returns the number of
 * frames decoded so far. */
int nasr_stream_get_frame_blank_logprobs(const nasr_stream *s, int64_t first, int32_t count, float *out);
/* phrase boosting for this stream (engine option "phrase_boost"; default: enabled).  Completes steps in flight.  Every call, with either
 * value, resets the stream's boost history (the emitted tokens a phrase can continue from), not its decoder state.  Fails when the option is off. */
int nasr_stream_set_boost(nasr_stream *s, int enable);

/* ---- the step: replaces nemo_stream_process_incremental (src/nemo-stream.cpp:1145-1206)
 * for B streams at once = nemo_preprocessor_process (src/preprocessor.cpp:330-395) +
 * every full chunk through process_mel_chunk_streaming (:1013-1128: encoder graph compute
 * :1063, decode_one_step per frame :1107-1118) + the mel-buffer shift (:1189-1195).
 * pcm[b] has n_samples[b] samples (0 allowed).  New token ids of stream b are written to
 * tokens_out[b][0..n_tokens[b]), n_tokens[b] <= tokens_cap[b].  Tokens that do not fit are never dropped: they stay queued
 * on the stream and come out of the next step / collect / finalize call (n_tokens[b] == tokens_cap[b] => call
 * nasr_engine_collect until it returns fewer).  With tokens_out == NULL the tokens are discarded and counted. */
int nasr_engine_step(nasr_engine *e, nasr_stream *const *streams, int B,
                     const int16_t *const *pcm, const int32_t *n_samples,
                     int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens,
                     uint32_t flags);

/* ---- audio input conversion on the device (the reference's answer to everything but s16le 16 kHz mono is "pipe it through ffmpeg
 * -ar 16000 -ac 1 -f s16le"): a stream can be told what its audio looks like, and the engine turns it into the 16 kHz s16 samples
 * nasr_engine_step takes, in one launch for all streams of a call, with streaming state: the samples do not depend on how the audio is
 * cut into pushes.  Rates 8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000 Hz; s16, f32 (a non-finite value reads as 0), G.711
 * mu-law and A-law; 1 .. 8 interleaved channels, of which `channel` >= 0 picks one and -1 takes the mean.  The resampler is a
 * Kaiser-windowed sinc (32 zero crossings per side, beta 9, roll-off 0.94: +-0.1 dB up to 0.87 of the lower Nyquist, -80 dB from 1.03 of it)
 * evaluated in f32 in a fixed order; csrc/nasr_resample.h states the arithmetic and is the host restatement the kernel is tested against
 * bit for bit.  Latency 32 periods of the lower rate: 2 ms at 48 kHz, 4 ms at 8 kHz.  16 kHz is converted without a filter. */
enum { NASR_AUDIO_S16 = 0, NASR_AUDIO_F32 = 1, NASR_AUDIO_MULAW = 2, NASR_AUDIO_ALAW = 3 };
typedef struct nasr_audio_format { int32_t sample_rate, encoding, channels, channel; } nasr_audio_format;  /* default {16000, S16, 1, 0} */
/* succeeds only on a stream that has taken no audio since create or reset; fails -- the previous format stays in force -- otherwise and
 * for an unsupported rate, encoding, channel count or channel index.  The format survives both reset modes. */
int nasr_stream_set_audio_format(nasr_stream *s, const nasr_audio_format *f);
/* nasr_engine_step for audio in each stream's own format: audio[b] holds n_frames[b] input frames (sample times, all channels), host
 * memory, or device memory with NASR_FLAG_PCM_DEVICE (then naturally aligned: 2 bytes for s16, 4 for f32; checked).  The converter writes the 16 kHz samples the frames complete (nasr_audio_out_ready)
 * and the call goes on exactly as nasr_engine_step does with them; a stream with the default format is passed through and gives
 * nasr_engine_step's bits.  A call that completes no sample for any stream is a nasr_engine_step of zero samples.  samples_in counts 16 kHz samples.
 * nasr_engine_step itself refuses a stream whose format is not the default.  nasr_engine_finalize first hands the front end the
 * converter's tail (nasr_audio_out_total - nasr_audio_out_ready samples, zeros as future input). */
int nasr_engine_step_audio(nasr_engine *e, nasr_stream *const *streams, int B, const void *const *audio,
                           const int32_t *n_frames, int32_t *const *tokens_out, const int32_t *tokens_cap,
                           int32_t *n_tokens, uint32_t flags);
/* one-shot, stateless: the same kernel over a whole buffer from a zero history, flushed: nasr_audio_out_total(f, n_frames) samples into
 * out (host memory; with NASR_FLAG_PCM_DEVICE audio AND out are device memory, naturally aligned).  Completes steps in flight, touches no stream.  Returns
 * the number of samples written or < 0 (also when cap is too small).  Feed the result to nasr_engine_transcribe / nasr_engine_align. */
int64_t nasr_engine_convert_audio(nasr_engine *e, const nasr_audio_format *f, const void *audio, int64_t n_frames,
                                  int16_t *out, int64_t cap, uint32_t flags);
/* host only, no GPU: 16 kHz samples available after n_frames_in input frames of a stream / in all once it has ended; < 0 for a bad format */
int64_t nasr_audio_out_ready(const nasr_audio_format *f, int64_t n_frames_in);
int64_t nasr_audio_out_total(const nasr_audio_format *f, int64_t n_frames_in);

/* debug/parity tap: same as nasr_engine_step but takes log-mel frames [n_frames][128] f32
 * (host memory) and skips stage a-1, i.e. enters at the mel_buffer append of :1162. */
int nasr_engine_step_mel(nasr_engine *e, nasr_stream *const *streams, int B,
                         const float *const *mel, const int32_t *n_frames,
                         int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens,
                         uint32_t flags);

/* tail flush: replaces nemo_stream_finalize (src/nemo-stream.cpp:1217-1293): if more than
 * 9 mel frames are buffered, n_valid = (frames-9)/8 outputs of one zero-padded step. */
int nasr_engine_finalize(nasr_engine *e, nasr_stream *const *streams, int B,
                         int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens);

/* ---- stream fork and tail preview (the reference has neither: a nemo_stream_context has one future) ----
 * nasr_stream_fork: *out = a new stream in the lowest free slot whose state is src's at this moment.  One device launch copies the live
 * part of src's slot (per layer the 70 K/V window rows and the conv cache, the buffered mel frames and samples, the decoder's per-slot
 * buffers: 8.6 MB of the 38 MB a slot of a 24-layer bf16 engine owns) into the free slot.
 *  - What the fork inherits.  Like nasr_stream_reset the call first completes the pipelined steps in flight.  The fork takes src's
 *    right_context, prompt, audio format and converter plan, boost / LM enable flags, every host-mirror counter (samples_in, chunks,
 *    cache_valid_len, ...) and the tokens decoded but not yet handed over (they come out of BOTH streams' next step / collect / finalize).
 *  - Identical twin.  Any sequence of calls made on both afterwards gives the same tokens, frames and read-outs (token frames, log-
 *    probabilities, alternatives, per-frame blank log-probabilities).  The read-outs are counted from src's create / reset: token index i
 *    and frame t mean the same on both.  (Stepped in one call of their own each they are equal bit for bit; two rows of one call may differ
 *    in the last bits of a log-probability, like any two rows.)
 *  - Isolation.  src is not changed in any bit, and the two streams are independent from then on: destroy, reset, set_boost, set_lm,
 *    set_prompt on one do not reach the other.
 *  - Failures.  Fails -- with a message, *out = NULL and the engine usable -- on a null stream, on a pointer that is no live stream (destroyed, or its engine destroyed: the library keeps the set of
 *    live streams and does not read the pointer) and on an exhausted pool
 *    ("stream pool exhausted (max_streams=%d)").
 *  - Options and graphs.  It allocates nothing on the device, captures no step graph and invalidates none (step graphs take the slot from
 *    their row descriptors).  Debug taps are not copied: a fork's taps (mel, PCM16, subsampled, layer and encoder outputs) are empty
 *    until its own first call.  The frame history (engine option "frame_history") is not copied either: a fork starts with an empty
 *    history at the frames src has decoded (nasr_stream_history_range gives (done, 0)) and keeps its own frames from there; src's history
 *    is untouched.  The copy plan is the same with the option on or off. */
int nasr_stream_fork(nasr_stream *src, nasr_stream **out);
/* nasr_engine_preview: the tokens nasr_engine_finalize would add for each stream if it were called now; the streams are not changed.
 *  - Mechanism.  Every stream is forked into a free slot, the forks take the nasr_engine_finalize path as ONE batch (the converter's tail
 *    of streams with an audio format of their own included), their new tokens are read and the slots are released.
 *  - Outputs.  n_tokens[b] (required) = the number of tail tokens; tokens the source produced before, delivered or still queued, are not
 *    among them.  The first min(n_tokens[b], tokens_cap[b]) are written to tokens_out[b]; the rest are dropped -- they are a preview, and
 *    nothing is queued anywhere.  frames_out (may be NULL, as may frames_out[b]) receives their absolute encoder frames.
 *  - Needs.  B free slots: fewer is an error that names how many are missing (max_streams is the caller's to size with headroom).  The
 *    rules of every batched call apply (one engine, one right_context, no stream twice).
 *  - Effects.  It completes steps in flight and runs eagerly, and synchronises.  Neither the sources nor their debug taps change (on a
 *    debug engine the per-call staging of NASR_TAP_MEL / NASR_TAP_PCM16 is set aside and put back; only NASR_TAP_ENCODER_OUT WITHOUT debug
 *    mode, which reads the engine's workspace and is valid "until the next chunk step of this engine", ends with a preview).  A stream with
 *    nothing to flush (at most 9 mel frames buffered) gives 0 tokens.
 * Engine counters "stream_forks" (fork launches: nasr_stream_fork calls and every fork of a preview) and "stream_previews". */
int nasr_engine_preview(nasr_engine *e, nasr_stream *const *streams, int B,
                        int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens,
                        int32_t *const *frames_out);

/* ---- stream snapshots in host memory: save, restore, move between engines (the reference has none) ----
 * nasr_stream_save: writes everything stream s is into buf as one self-describing blob (little-endian, format version 1:
 * csrc/nasr_snapshot.h) and its exact size into *bytes_out.  nasr_stream_restore: *out = a new stream in the lowest free slot of e that
 * continues exactly as the saved one would have.  nasr_engine_snapshot_bound: *bytes_out = the largest blob any stream of e can produce
 * under the decode options now in force (a buffer of that size always suffices).
 *  - What travels.  The live part of the slot -- what nasr_stream_fork copies: per layer the 70 K/V window rows and the conv cache, the
 *    buffered mel frames and samples, the converter's history, the decoder's per-slot buffers (8.55 MB at 24 layers bf16) -- gathered by one
 *    device launch and one device-to-host copy, and the host mirror: right_context, prompt, every counter (samples_in, chunks,
 *    cache_valid_len, ...), the boost / LM enable flags, the audio format, and the tokens decoded but not yet handed over.  Those tokens stay
 *    queued in s AND are in the blob: they come out of the restored stream's next step / collect / finalize.  Ring rows are stored in
 *    logical order with the ring positions in the mirror, so a blob does not depend on the slot it came from; it holds no pointer.
 *  - Identical twin.  The contract of nasr_stream_fork: any sequence of calls made on s and on the restored stream afterwards gives the
 *    same tokens, frames and read-outs, bit for bit when each is stepped in calls of its own; read-outs are counted from the original's
 *    create / reset.  e may be the engine that saved, another engine of the process, an engine on another device or of a later process, as
 *    long as it agrees with the blob: dtype, n_layers, kernel_size, the layout constants, the decode options (token_logprobs,
 *    token_alternatives, frame_blank_logprobs, phrase_boost, lm_fusion, token_entropy) and three fingerprints -- of the weight set (names, types, shapes
 *    and a bounded sample of every tensor's bytes, taken at nasr_engine_create), of the boost set in force and of the language model in
 *    force with its greedy weights (0 when none).  A caller who wants to restore under another boost set or model sets the same one
 *    first; there is no mode that resets the bias state.
 *  - Isolation.  nasr_stream_save completes the pipelined steps in flight, like nasr_stream_fork; s is not changed in any bit and goes on
 *    living.  The restored stream is independent of s and of the blob, which may be restored any number of times.
 *  - Failures.  Save: buf == NULL or cap too small is an error whose message names the size needed, and *bytes_out is still set (so a
 *    call with buf == NULL asks for the size); a null stream, a pointer that is no live stream.  Restore refuses, before any device work and
 *    with one message per cause: bad magic or version, a truncated blob or trailing bytes, a corrupted header / mirror checksum, every
 *    mismatch with the engine (the message names the field and both values), every mirror field out of its range, a device section whose
 *    size is not what the plan for this mirror says (no offset or length inside the blob is trusted), an exhausted pool
 *    ("stream pool exhausted (max_streams=%d)").  The device section's checksum is computed by the unpack launch itself and compared with the header
 *    afterwards; then the decoder fields a kernel uses as an index are range-checked.  On any failure *out = NULL, a message is set, no
 *    slot is held and the engine stays usable.  The format is integrity-checked, not authenticated: the checksums catch corruption in
 *    transit or on disk; a forged blob with matching checksums is outside the promise.
 *  - Options and graphs.  Neither call captures a step graph or invalidates one, and a step that never saves or restores launches what it
 *    always did.  The first save or restore allocates a device staging buffer of the size of the bound (grown when an option raises it,
 *    freed with the engine) and a pinned block.  Debug taps are empty until the restored stream's own first call, as after a fork.
 *    The frame history (engine option "frame_history") does not travel: the blob has the same bytes, size and header with the option on or
 *    off, the option is not among the ones that must agree, and a restored stream starts with an empty history at the frames the saved
 *    stream had decoded, as a fork does.
 * Engine counters "stream_saves" and "stream_restores". */
int nasr_engine_snapshot_bound(nasr_engine *e, int64_t *bytes_out);
int nasr_stream_save(nasr_stream *s, void *buf, int64_t cap, int64_t *bytes_out);
int nasr_stream_restore(nasr_engine *e, const void *buf, int64_t bytes, nasr_stream **out);

/* with NASR_FLAG_NO_SYNC: wait for outstanding work and fetch the tokens produced since the
 * last collect (replaces nemo_stream_get_tokens, src/nemo-stream.cpp:1301-1305, as a delta) */
int nasr_engine_collect(nasr_engine *e, nasr_stream *const *streams, int B,
                        int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens);

/* ---- parity taps (reference: append_dump_tensor, src/nemo-stream.cpp:982-1010) --------- */
enum {
    NASR_TAP_MEL         = 0, /* log-mel frames produced by the last step call  [n][128]       */
    NASR_TAP_SUBSAMPLED  = 1, /* conformer input of the last chunk (after drop-2) [T][1024]     */
    NASR_TAP_LAYER_OUT   = 2, /* output of layer `index` for the last chunk      [T][1024]     */
    NASR_TAP_ENCODER_OUT = 3, /* encoder output of the last chunk                [T][1024]     */
    NASR_TAP_K_CACHE     = 4, /* K cache of layer `index`, logical order         [70][1024]    */
    NASR_TAP_V_CACHE     = 5,
    NASR_TAP_CONV_CACHE  = 6, /*                                                 [ks-1][1024]  */
    NASR_TAP_DEC_STATE   = 7, /* h[2][640], c[2][640], then prev_token as float                */
    NASR_TAP_PCM16       = 8, /* the 16 kHz samples the last step / step_audio / finalize call handed to the front end
                                 for this stream, as floats holding the s16 values     [n]            */
};
/* engine options: "fused" (1: small-M fused layer kernels, default) / "graph" (1: hipGraph replay of the
 * steady-state step, default) / "multichunk" (1, default) are pure performance switches; results are unchanged.
 * "pipeline" (0, default; E = 1..4): launch sequences of consecutive steps run beside each other on their own HIP streams.
 * The encoder is cut into E pieces of L / E layers and a step's piece k + 1 runs one call after its piece k, beside piece k
 * of the next step; the decode follows one call after the last piece (layer l of a step needs from the previous step only
 * what its layer l left in the K/V ring and the conv cache).  E = 1: the decode graph of step s beside the encoder graph
 * of step s + 1.  The same tokens come out, E calls later: nasr_engine_step returns what has been decoded so far;
 * nasr_engine_finalize, nasr_engine_collect and every other entry point first complete the steps in flight.  Results are
 * bit-identical to synchronous stepping.  The engine runs at most as many pieces as it finds HIP streams that truly run side
 * by side (it measures which streams share a hardware queue at the first pipelined step: normally 4).  The decode graphs run on
 * the last of these streams: a queue of their own up to E = 3, right behind the fourth piece at E = 4 (worth 1-5 % at 16-64
 * streams, nothing at one stream); fewer pieces when the process leaves the engine fewer queues, and at most three pieces whatever E from 5 600 rows ("large_step_rows"; round 4: 3 584) per
 * step (400+ streams x R = 13: more lanes are more GEMM working sets in the same L2s; tokens then come back sooner; engine option "large_step_pieces",
 * 0 = no such limit).  Throughput option for callers that push back to back
 * (a server draining a backlog, a file); a live stream keeps the default.
 * "pipeline" = 8 (round 3, experimental): for calls of one or two rows per step (one stream x R = 0 or 1, two streams x R = 0) the 8 steps in flight
 * sit at 8 stages of 3 layers and every launch of the two chains carries the same kernel of FOUR steps (grouped launches); tokens 9 calls later;
 * other shapes fall back to four lanes.  Bit-identical as well; measured +2.7 % at batch 1 (profiles/r3_grouped_pipeline.md), so 4 stays the default.
 * "lanes" (1..4): keep at most this many encoder lanes and give the other lanes' streams back -- for a process with another GPU
 * client (the diarization side-car): a stream created after this call gets a hardware queue the engine no longer uses.  Not
 * reversible for the engine's lifetime.
 * "graph_cache" (>= 1, default 16): step shapes (streams in the call, lookahead, chunks per push, pieces) whose hipGraphs are kept;
 * beyond it the least recently used shape is dropped and re-captured when it comes back -- a server whose batch size changes from
 * call to call (reference: one stream per call, src/nemo-server.cpp:192-271) holds a bounded number of graph execs.
 * Kernel-selection switches for A/B runs and bit-identity tests (round 4: these were environment variables read inside the product path;
 * set them before the first step, results never depend on them): "gemm_cores" (-1 = the engine's rule, 0 / 1 = never / always the
 * large-M GEMM kernels of which two share a CU), "persistent_gemm" (1: GEMMs with several 128 x 128 tiles per CU on the persistent tile loop; default 0),
 * "wide_tiles" (default 1: 256- / 224-row tiles from 1 792 rows where their rounds fill the chip, in pipelined steps from 1 344 rows and 32 tiles ("wide_min_rows" / "wide_min_tiles"; rounds 4: 96);
 * 256: the 256-row form only; 3: without the pipelined steps' tile-count rule; 0: off), 
 * "t64_tiles" (default 64, per engine: the split-K GEMMs with N = 1024 take 128 x 64 tiles up to this many 128 x 128 tiles; round 3: 127),
 * "tile_bands" (-1 = the rule: above 4 row chunks the tiles of a launch are handed to the XCDs in bands of column groups, so that the panels an XCD reads stay in its L2;
 * 0 / 1 = never / always), "f32_mfma" (0: f32 GEMMs above
 * four rows on the FMA tile kernel instead of the f32 MFMA), "decode_graph_iterations" (decode iterations a pipelined step's decode graph carries before the eager
 * fallback.  N >= 1: max(the synchronous step graph's count, min(10 frames + 1, N)).  Default 0 = auto: as 12, except that a step of ONE
 * frame and up to four rows on a bf16 engine (one to four streams at R = 0) carries 3 -- a frame of two symbols and the closing blank; its
 * decode graph runs behind the fourth encoder piece on a lane the host waits for in every call, so idle iterations there cost step time.
 * A frame that emits three or more symbols is completed by the fallback: same tokens, one host round trip, counter "decode_fallbacks"),
 * "fused_cuts" (MEASUREMENT ONLY, results are valid: the launch indices at which a step of up to four rows is cut into its four lane
 * pieces, for a 24-layer model, 10 bits each, lowest first; 0 = built in (46 | 98 | 150 of 192).  REJECTED after the first pipelined step), "resid_epilogue" (0: every residual GEMM writes split-K partial
 * slabs and k_post adds them, as in rounds 1-4; default 1: the GEMM adds to the residual stream in its epilogue where one workgroup owns a tile's
 * whole K sum -- same bits), "gemm_prio" (default 0: round 5's GEMM loops -- k_gemm_wide2 / k_gemm_tiled3: the next chunk's fragments read under this chunk's
 * MFMAs, wave-private epilogues; 20: rounds 1-4's loops; same bits), "epilogue16" (default 1: the GEMM epilogues with 16-bit outputs store eight columns = 16 bytes
 * per thread; 0: four), "wide_min_tiles" / "wide_min_rows" (defaults 32 / 1 344: pipelined steps take the 224 x 256 tiles from this many tiles and rows), "split_tasks" (default 200: residual GEMMs take
 * one K slice from this many 128 x 128 tiles), "ablate" (MEASUREMENT ONLY -- results
 * are invalid: bit mask of launches left out of a step: 1 residual + LayerNorm, 2 attention, 4 depthwise conv, 8 decode iterations, 16 front end, 32 encoder
 * GEMMs; what each costs a pipelined step: profiles/r5_ablation.md), "decode_lane" (0: the decode graphs run behind the last encoder
 * piece instead of on a stream of their own; read when the lanes are picked, so it is REJECTED after the first pipelined step or
 * nasr_engine_lend_stream).
 * "audio_lds_table" (1 default / 0): nasr_engine_step_audio's kernel reads the coefficients of the 8 / 24 / 32 / 48 kHz tables from a copy in LDS
 * (0: from global memory like the larger tables; same bits; A/B switch, profiles/audio_input.md).
 * "fork_piece_kb" (0 default = 256; 1 .. 1024): KiB one workgroup of nasr_stream_fork's copy launch moves at most, i.e. its grid; the same
 * bytes are copied at every value (measurement only: A/B runs of profiles/stream_fork.md).
 * "token_logprobs" (0 default / 1): a capability, not a kernel A/B switch -- with 1 the device decode also keeps, for every emitted token,
 * the natural-log softmax probability of that token over the 1025 joint outputs (blank included) at the frame and decoder state where it
 * was emitted (nasr_stream_get_token_logprobs, nasr_engine_offline_token_logprobs).  Tokens, frames, iteration counts and decoder state
 * are bit-identical to 0.  It selects the decode kernels that are captured into the step graphs and allocates a ring per stream, so it is
 * REJECTED after the first step or offline call.
 * "phrase_boost" (0 default / N = 2 .. 4096): phrase boosting ("hotwords", "word boosting"; the reference has no such thing), a capability like
 * "token_logprobs".  N is the capacity of the phrase automaton in states: 2 fixed ones plus one per distinct non-empty prefix of the phrases
 * (about 100 phrases of 4 tokens: 400 states; 8 KB of tables per state, 34 MB at 4096).  With N > 0 the device decode takes
 * arg-max_v (logit[v] + bonus(v)) instead of arg-max_v logit[v], first maximum wins as before, where for a stream whose emitted non-blank
 * tokens since its last history reset are h, bonus(v) = the largest w_i over all phrases i and all k with p_i[0:k] a suffix of h and
 * p_i[k] == v, 0 if there is none; blank never gets a bonus and never enters h.  So the first token of every phrase is always boosted, and
 * token k only right after tokens 0 .. k-1 were emitted.  Every other rule of the decode is unchanged (10 symbols per frame, state commit on
 * emission, frame numbering).  The history persists across steps, chunks and pipelined calls and is reset by nasr_stream_create, both
 * reset modes, nasr_stream_set_boost and nasr_engine_set_boost_phrases; an offline utterance starts with an empty one.  With no phrases
 * set (the state after this option) tokens, frames, iteration counts and decoder state are bit-identical to 0.  It selects the decode kernels
 * that are captured into the step graphs and allocates the tables, so it is REJECTED after the first step or offline call; the phrases
 * themselves can be replaced at any time.
 * "token_alternatives" (0 default / K = 1 .. 8): a capability like "token_logprobs" and independent of it -- with K > 0 the device decode also
 * keeps, for every emitted token, the K largest of the 1025 joint outputs (blank included) at the frame and decoder state where it was
 * emitted, as (id, ln P) pairs in descending order of the raw logit, the lower id first among equal logit bits
 * (nasr_stream_get_token_alternatives, nasr_engine_offline_token_alternatives).  The ranking is the model's also under "phrase_boost": the
 * emitted token then need not be entry 0; without phrases it is.  The results for K are the first K columns of those for any larger K.
 * Tokens, frames, iteration counts and decoder state are bit-identical to 0.  It selects the decode kernels that are captured into the step
 * graphs and allocates two rings per stream, so it is REJECTED after the first step or offline call.
 * "frame_blank_logprobs" (0 default / 1): a capability like "token_logprobs" and independent of it -- with 1 the device decode also keeps, for
 * every encoder frame it has finished, the natural-log softmax probability of BLANK over the 1025 joint outputs at the last joint evaluation
 * it made on that frame (nasr_stream_get_frame_blank_logprobs, nasr_engine_offline_frame_blank_logprobs): the frame-level silence signal an
 * endpoint detector needs (csrc/nasr_endpoint.h).  Under "phrase_boost" the value stays the model's.  Tokens, frames, iteration counts, decoder
 * state and the values of "token_logprobs" / "token_alternatives" are bit-identical to 0.  It selects the decode kernels that are captured
 * into the step graphs (those of "token_logprobs" plus one small launch per iteration) and allocates a ring per stream, so it is REJECTED
 * after the first step or offline call.
 * "token_entropy" (0 default / round(1000 alpha): 1000 = Shannon, 333 = the usual 1/3; accepted are 1000, 50 .. 900 and 1100 .. 4000 -- closer
 * to 1 the order's 1 / (1 - alpha) outgrows the precision of the value -- anything else is refused): a capability like "token_logprobs" and
 * independent of it -- the device decode also keeps, for every emitted token, the entropy of order alpha of the joint's softmax over the 1025
 * outputs where it was emitted (nasr_stream_get_token_entropies, nasr_engine_offline_token_entropies): the input of entropy-based confidence
 * (host/token_confidence.h).  Under "phrase_boost" / "lm_fusion" the value stays the model's.  Tokens, frames, iteration counts, decoder state
 * and the values of the other read-outs are bit-identical to 0.  It selects the decode kernels that are captured into the step graphs and
 * allocates a ring per stream, so it is REJECTED after the first step or offline call.
 * "frame_history" (0 default; N = 64 .. 2048 in multiples of 64, other values are refused): a capability like "frame_blank_logprobs" -- with
 * N every live stream keeps the joint's encoder-projection rows ([640] f32, prompt fused in) of the last N encoder frames it decoded, in a
 * device ring filled by one more small launch at the head of every step's decode (csrc/nasr_history.h), so that the offline modes can run
 * over a window of them without audio and without an encoder run: nasr_stream_history_range, nasr_stream_get_history,
 * nasr_engine_history_transcribe / _beam / _align.  HBM: max_streams x N x 2 560 bytes -- 5.2 MB per slot at N = 2048, 2.7 GB at 512 streams.
 * Tokens, frames, decoder state and every other read-out are bit-identical to 0; with 0 no launch is added and nothing is allocated.  Cost
 * at 24 layers bf16 (profiles/frame_history.md): the headline shape (1 stream, "pipeline" = 4) and 64 streams x right_context 13 stay inside
 * their run-to-run spread; a synchronous one-stream step, one dependent chain, gains about 0.005 ms (0.8685 -> 0.873 .. 0.875 ms, 0.5 .. 0.75 %).  The
 * launch is captured into the step graphs and the rings are allocated by this call, so it is REJECTED after the first step or offline call;
 * until then another N replaces the rings and 0 frees them.  "history_append_rows" (MEASUREMENT ONLY; 0 default = 1, or 4): rows one
 * workgroup of the append launch moves, i.e. its grid; the same bytes (profiles/frame_history.md).  Before the first step. */
int nasr_engine_set_option(nasr_engine *e, const char *key, int value);
/* replaces the engine's boost set (engine option "phrase_boost" = N): phrase i = tokens[i][0 .. lens[i]), 1 .. 32 non-blank token ids
 * (0 .. 1023), with bonus[i], finite, 0 < bonus <= 1e4, in natural-log units (added to the joint's logits).  n_phrases = 0 clears the set.
 * Completes steps in flight, builds the automaton on the host, uploads it and resets EVERY stream's boost history; captured step graphs
 * stay valid.  Fails -- leaving the engine usable and the previous set in force -- when the option is off, a token id is blank or out of
 * range, a length is outside 1 .. 32, a bonus is not finite or not in (0, 1e4], or the set needs more than N states. */
int nasr_engine_set_boost_phrases(nasr_engine *e, int n_phrases, const int32_t *const *tokens, const int32_t *lens, const float *bonus);
/* diagnostics: "graph_execs" (hipGraphExec objects alive), "graph_shapes" (distinct cached step shapes), "graph_evictions",
 * "graph_replays" (calls served by a hipGraph, pipelined ones included), "eager_steps" (calls that were not graph-eligible: ragged
 * pushes, streams that complete different chunk counts), "pipelined_steps", "grouped_steps", "lanes" (HIP streams the engine found
 * to overlap; 0 before the first pipelined step), "boost_states" (automaton states of the current boost set, the two fixed ones included:
 * 2 with no phrases; 0 when engine option "phrase_boost" is off), "decode_fallbacks" / "decode_fallback_rounds" (graph steps whose
 * decode needed more iterations than their graph carries and was completed eagerly / the host round trips that took), "stream_forks" / "stream_previews" (nasr_stream_fork launches, a preview's included / nasr_engine_preview calls),
 * "stream_saves" / "stream_restores" (nasr_stream_save calls that wrote a blob / nasr_stream_restore calls that made a stream; refused calls are not counted),
 * "history_calls" / "history_frames" (nasr_engine_history_* calls that succeeded / the frames they gathered out of the streams' rings), "cut_drains" (pipelined calls that first completed the steps in flight because
 * they are cut into lane pieces differently: another piece count, or the other side of four rows per step on a bf16 engine).  Returns 0, or -1 for an unknown name.  Like every entry point that takes an
 * engine, call it from the thread that steps that engine: it reads the graph caches without a lock. */
int nasr_engine_get_counter(const nasr_engine *e, const char *name, int64_t *value);
/* enable recording of NASR_TAP_MEL / SUBSAMPLED / LAYER_OUT (costs extra copies) */
int nasr_engine_set_debug(nasr_engine *e, int enable);
/* returns the number of floats written (<= cap) or <0.  NASR_TAP_K_CACHE / V_CACHE return the LOGICAL cache: rows that are not
 * cached yet (the first 70 - cache_valid_len) read as the zeros the reference's tensors start with (src/nemo-stream.cpp:320-325). */
int64_t nasr_stream_get_tap(nasr_stream *s, int which, int index, float *out, int64_t cap);
/* test hook: overwrites every row of the stream's K/V rings (all layers) with +-value.  A stream start / reset does not clear the
 * rings -- rows behind cache_valid_len are masked with -1e9 and weigh exactly 0, as in the reference's own reset
 * (src/nemo-stream.cpp:95-115, :1037-1043) -- and this is how the tests prove that stale rows never reach a result. */
int nasr_stream_debug_fill_kv(nasr_stream *s, float value);

/* ---- measurement: per-kernel-class HIP-event timing on the engine's own
 * stream.  Replaces the std::chrono timers of src/nemo-stream.h:236-244. ---------------- */
int nasr_engine_profile(nasr_engine *e, int enable); /* enable also resets the counters */
int nasr_engine_profile_read(nasr_engine *e, nasr_kernel_stat *out, int cap); /* returns count */
/* raw hipStream_t of the engine (for external event timing) */
void *nasr_engine_hip_stream(nasr_engine *e);
/* Hands the last of the engine's side-by-side HIP streams -- and with it a hardware queue that no encoder lane will use -- to
 * another GPU client of the process (nasr_diar_set_stream).  The engine runs one encoder piece fewer at most and still owns the
 * stream.  Borrowers inside this library are counted: destroy them first.  If the engine goes first, nasr_engine_destroy says so
 * on stderr and in nasr_last_error(), and the stream stays alive until its last borrower lets go (nothing dangles in either
 * order).  *out receives a hipStream_t. */
int nasr_engine_lend_stream(nasr_engine *e, void **out);
/* device malloc/free/copy helpers so a host written without HIP can keep PCM resident */
int nasr_device_alloc(nasr_engine *e, void **out, int64_t bytes);
int nasr_device_free(nasr_engine *e, void *p);
int nasr_device_upload(nasr_engine *e, void *dst_device, const void *src_host, int64_t bytes);
int nasr_engine_synchronize(nasr_engine *e);

/* ---- offline full-context transcription: replaces nemo_transcribe_audio / nemo_encode (src/nemo-ggml.cpp:1600-1737, declared
 * src/nemo-ggml.h:359-375; the `transcribe` binary, src/transcribe.cpp) for B whole utterances at once.  mel[b]: n_frames[b] log-mel
 * frames [n][128] f32 (host memory) = the preprocessor run once over the whole utterance, no zero prefix.  Encoder frames
 * T = s(s(s(n_frames))), s(n) = n / 2 + 1 (ConvSubsampling without drop-2); every query attends to every key of its own utterance;
 * the depthwise conv starts from a zero history; prompt fusion uses prompt_index[b] (NULL = -1 for all); greedy decode with the
 * reference's rules, frames numbered from 0 within the utterance.  n_tokens[b] = tokens emitted for utterance b; the first
 * min(n_tokens[b], tokens_cap[b]) are written to tokens_out[b], their encoder-frame indices to frames_out[b] if frames_out != NULL.
 * An utterance with T > NASR_OFFLINE_MAX_FRAMES fails the call (the engine stays usable); n_frames[b] = 0 gives 0 tokens.  The call
 * first completes pipelined steps in flight and touches no stream state (K/V rings, conv caches, decoder states, mel buffers,
 * token rings, graph caches); it runs eagerly.  NASR_FLAG_NO_SYNC is rejected.  Utterances are packed densely and cut into
 * sub-batches of at most "offline_rows" encoder rows (engine option, default 16 384): results are bit-identical to one
 * utterance per call. */
#define NASR_OFFLINE_MAX_FRAMES 2048   /* encoder frames per utterance = the reference's max_pos_len (src/nemo-ggml.cpp:229-233) */
int nasr_engine_transcribe_mel(nasr_engine *e, int B, const float *const *mel, const int32_t *n_frames,
                               const int32_t *prompt_index, int32_t *const *tokens_out, const int32_t *tokens_cap,
                               int32_t *n_tokens, int32_t *const *frames_out, uint32_t flags);
/* the same from s16 PCM: pcm[b] holds n_samples[b] samples of a whole utterance (host memory, or device memory with
 * NASR_FLAG_PCM_DEVICE).  The log-mel is the reference preprocessor run once over the whole utterance (src/preprocessor.cpp,
 * no 9-frame zero prefix): 1 + (256 + n - 512) / 160 frames, none below 256 samples (such an utterance gives 0 tokens). */
int nasr_engine_transcribe(nasr_engine *e, int B, const int16_t *const *pcm, const int32_t *n_samples,
                           const int32_t *prompt_index, int32_t *const *tokens_out, const int32_t *tokens_cap,
                           int32_t *n_tokens, int32_t *const *frames_out, uint32_t flags);
/* after an offline call (either entry) made with nasr_engine_set_debug(e, 1): NASR_TAP_MEL [n][128] / NASR_TAP_SUBSAMPLED
 * [T][1024] / NASR_TAP_LAYER_OUT (index = layer) / NASR_TAP_ENCODER_OUT of utterance u of that call.  Every offline call forgets
 * the taps of the one before.  Returns the number of floats written (<= cap), with out == NULL the number available, or < 0. */
int64_t nasr_engine_offline_tap(nasr_engine *e, int which, int u, int index, float *out, int64_t cap);
/* ln P(token) of every token of utterance u of the LAST offline call (either entry; engine option "token_logprobs" = 1), in token order:
 * out[i] belongs to tokens_out[u][i]; in [-ln 1025, 0], or any finite value <= 0 with phrase boosting (the model's probability of a boosted
 * token, see nasr_stream_get_token_logprobs).  Returns the number written (<= cap), with out == NULL the number available, or < 0.  Every offline
 * call forgets the values of the one before. */
int nasr_engine_offline_token_logprobs(nasr_engine *e, int u, float *out, int32_t cap);
/* the entropy (engine option "token_entropy", see nasr_stream_get_token_entropies) at every token of utterance u of the LAST offline greedy
 * call (nasr_engine_transcribe / _transcribe_mel / nasr_engine_history_transcribe), in token order: out[i] belongs to tokens_out[u][i].
 * Returns the number written (<= cap), with out == NULL the number available, or < 0.  Every offline call forgets the values of the one before. */
int nasr_engine_offline_token_entropies(nasr_engine *e, int u, float *out, int32_t cap);
/* ln P(blank) at the last joint evaluation of every encoder frame of utterance u of the LAST offline call (either entry; engine option
 * "frame_blank_logprobs" = 1): out[t], t = 0 .. T - 1, see nasr_stream_get_frame_blank_logprobs.  Returns the number written (<= cap), with
 * out == NULL the number available (T), or < 0.  Every offline call forgets the values of the one before. */
int nasr_engine_offline_frame_blank_logprobs(nasr_engine *e, int u, float *out, int32_t cap);
/* the K alternatives (engine option "token_alternatives" = K) of every token of
 * utterance u of the LAST offline call; cap in tokens; ids_out == NULL: the number available.  [tokens][K] row-major, row i belongs to
 * tokens_out[u][i].  Returns the number of tokens written (<= cap) or < 0.  Every offline call forgets the values of the one before. */
int nasr_engine_offline_token_alternatives(nasr_engine *e, int u, int32_t *ids_out, float *logprobs_out, int32_t cap);

/* ---- forced alignment and transcript scoring (offline): given audio and a KNOWN transcript, when was each token spoken, and what is
 * ln P(transcript | audio) under the model.  The encoder is exactly that of nasr_engine_transcribe(_mel): the same frame-count rule and
 * NASR_OFFLINE_MAX_FRAMES failure, the same packing into sub-batches of "offline_rows", the same prompt fusion and the same contract (the call
 * completes steps in flight, touches no stream state, rejects NASR_FLAG_NO_SYNC, runs eagerly).  tokens[b] holds U = n_tokens[b] ids in
 * 0 .. 1023, 0 <= U <= NASR_ALIGN_MAX_TOKENS; a blank (1024), an id out of range or a longer transcript fails the whole call with a message
 * that names the utterance, and the engine stays usable.
 * Lattice of utterance b with T encoder frames: cell (t, u), 0 <= t < T, 0 <= u <= U, has the logits W_out . relu(encproj[t] + g[u]) + b_out --
 * the joint the greedy decode evaluates -- with g[u] = joint.pred(h1_u) + b_pred, h_u the LSTM state after blank, y_0 .. y_{u-1} from the zero
 * state (teacher forcing; u = 0 is the state a fresh decode starts in).  lb(t, u) = ln softmax at blank, ly(t, u) = ln softmax at y_u (u < U).
 * Phrase boosting never applies: these are the model's probabilities.  The recursions are those of the standard RNN-T lattice, in double:
 *   alpha(0, 0) = 0,  alpha(t, u) = logaddexp(alpha(t-1, u) + lb(t-1, u), alpha(t, u-1) + ly(t, u-1)),  loglik = alpha(T-1, U) + lb(T-1, U)
 * and Viterbi the same with max, where the token move (t, u-1) -> (t, u) is taken only when its score is STRICTLY greater than the blank
 * move's.  There is no cap of 10 symbols per frame here: that cap is a rule of the greedy loop, not of the model, so any number of tokens may
 * fall on one frame (U > T is fine).  loglik_out[b] = ln P(y | audio); best_out[b] = the score of the best path, its final blank included
 * (loglik >= best); frames_out[b][i] = the frame at which y_i is emitted on that path, non-decreasing, in 0 .. T-1;
 * token_logprobs_out[b][i] = ly(frames_out[b][i], i).  Any of the four output pointers, or a per-utterance row pointer, may be NULL.
 * T == 0 with U == 0: loglik = best = 0.  T == 0 with U > 0: loglik = best = -INFINITY, frames -1, log-probabilities -INFINITY, and the call
 * succeeds.  U == 0: loglik = best = the sum of the blanks of column 0.
 * Engine option "align_cells" (default 1 << 20, minimum 64): lattice cells one launch of the joint kernel covers; larger lattices and
 * sub-batches take several launches.  The lattice of a sub-batch itself is held whole for the recursions (9 bytes per cell).  Results are
 * bit-identical whatever its value and whatever else is in the batch. */
#define NASR_ALIGN_MAX_TOKENS 1024
int nasr_engine_align_mel(nasr_engine *e, int B, const float *const *mel, const int32_t *n_frames, const int32_t *prompt_index,
                          const int32_t *const *tokens, const int32_t *n_tokens, double *loglik_out, double *best_out,
                          int32_t *const *frames_out, float *const *token_logprobs_out, uint32_t flags);
/* the same from s16 PCM: pcm / n_samples and NASR_FLAG_PCM_DEVICE as for nasr_engine_transcribe */
int nasr_engine_align(nasr_engine *e, int B, const int16_t *const *pcm, const int32_t *n_samples, const int32_t *prompt_index,
                      const int32_t *const *tokens, const int32_t *n_tokens, double *loglik_out, double *best_out,
                      int32_t *const *frames_out, float *const *token_logprobs_out, uint32_t flags);
/* after an align call made with nasr_engine_set_debug(e, 1): lb and ly of utterance u of that call, each [T][U + 1] row-major f32 (column U
 * of lp_token reads -INFINITY); exp of them are the model's posteriors.  Returns the number of cells written (<= cap) to each non-NULL
 * pointer, with both NULL the number available, or < 0.  Every align call or offline call forgets the lattice of the call before. */
int64_t nasr_engine_align_lattice(nasr_engine *e, int u, float *lp_blank_out, float *lp_token_out, int64_t cap);

/* ---- frame-synchronous beam search (offline): the N best DISTINCT transcripts of each utterance with comparable scores.  The rules are
 * csrc/nasr_beam.h: per encoder frame up to max_symbols rounds; in a round every hypothesis of the active set A
 * arrives in the frame's set C with its score + ln P(blank), and A's successors are the `beam` best of the children (parent + token) over
 * each parent's largest non-blank joint outputs; C keeps its `beam` best and is the next frame's A.  Two arrivals with the same token
 * sequence are one hypothesis -- the higher score stays, with that path's frames -- so a score is always the score of ONE lattice path,
 * final blank of every frame included: a double sum of the f32 ln-softmax values nasr_engine_align_lattice exposes, never above `best`
 * of nasr_engine_align for that transcript.  Better = the higher score; among equal scores the earlier arrival wins.
 * beam = 1 is NOT the greedy decode of nasr_engine_transcribe: greedy emits the arg-max whenever it is not blank, the search may drop a
 * token whose continuation scores below the blank.  Phrase boosting ("phrase_boost") is NOT applied unless the call carries
 * NASR_FLAG_BEAM_BOOST (below); either way the scores are the model's probabilities, as in alignment.  An utterance with no encoder frame gives one hypothesis: empty, score 0.
 * The contract is that of nasr_engine_transcribe(_mel): the same encoder, frame-count rule and NASR_OFFLINE_MAX_FRAMES failure, the same
 * packing into sub-batches of "offline_rows", the call completes steps in flight, touches no stream state, runs eagerly and rejects
 * NASR_FLAG_NO_SYNC; results are bit-identical whatever else is in the batch.  nasr_engine_offline_tap works after a beam call made with
 * debug on.  Bad parameters fail the call with a message and leave the engine usable. */
typedef struct nasr_beam_params {
    int32_t beam;          /* W, 1 .. 8 */
    int32_t nbest;         /* N, 1 .. beam; 0 = beam */
    int32_t max_symbols;   /* S, 1 .. 10: tokens one frame may take; 0 = the default, 4 */
    int32_t reserved;      /* 0 */
} nasr_beam_params;
/* n_hyps[b] = hypotheses found for utterance b, 1 .. nbest (fewer than nbest only when the search kept fewer) */
int nasr_engine_transcribe_beam_mel(nasr_engine *e, int B, const float *const *mel, const int32_t *n_frames, const int32_t *prompt_index,
                                    const nasr_beam_params *params, int32_t *n_hyps, uint32_t flags);
/* the same from s16 PCM: pcm / n_samples and NASR_FLAG_PCM_DEVICE as for nasr_engine_transcribe */
int nasr_engine_transcribe_beam(nasr_engine *e, int B, const int16_t *const *pcm, const int32_t *n_samples, const int32_t *prompt_index,
                                const nasr_beam_params *params, int32_t *n_hyps, uint32_t flags);
/* hypothesis `rank` (0 = best) of utterance u of the LAST beam call: returns its token count and writes min(count, cap) tokens, encoder
 * frames and per-token ln P; *score_out = its score.  Any pointer may be NULL (cap 0: the count).  < 0 for a bad u or rank.  Every offline,
 * align or beam call forgets the hypotheses of the call before. */
int nasr_engine_beam_hypothesis(nasr_engine *e, int u, int rank, int32_t *tokens_out, int32_t *frames_out, float *token_logprobs_out,
                                int32_t cap, double *score_out);

/* ---- shallow fusion: a back-off n-gram language model in the beam search (csrc/nasr_lm.h, csrc/nasr_beam.h).
 * The model is over the transducer's own token ids (a sub-word LM; the engine has no word lexicon): tokens 0 .. 1023, NASR_LM_BOS only as
 * the first token of an n-gram, NASR_LM_EOS only as the last, never 1024 (blank).  Each n-gram has its tokens (oldest first), logprob
 * (natural log, finite, <= 0) and backoff (natural log, finite, any sign; NULL = all 0); unk_logprob (finite, <= 0) is the unigram value of
 * every token and of EOS without a unigram of its own.  Standard ARPA back-off semantics.  A duplicate n-gram, a length outside 1 .. order,
 * an id out of place, a non-finite value, an n-gram whose context (all tokens but the last) is not an n-gram of the set, or more than 2^24
 * n-grams fail the call with a message that names the n-gram.
 * While a model is attached EVERY beam call ranks by total = score + weight * lm + token_bonus * (tokens), lm = the sum of the tokens' LM
 * terms, everywhere the LM-free search compares scores; at the end lm gains the EOS term when some n-gram ends in EOS.  The LM re-scores the
 * candidates the transducer proposes (each hypothesis' `beam` largest non-blank outputs); it does not propose any.  score stays the model's
 * path score.  weight and token_bonus are finite in [0, 100]; with both 0 every result equals the LM-free call bit for bit.  The search
 * prunes only when token_bonus == 0 and no logprob or backoff is positive; otherwise it runs unpruned (same results, more work).
 * Without engine option "lm_fusion" (below) nasr_engine_transcribe, live streams and step graphs never see the model; alignment never does.
 * nasr_engine_set_lm completes steps in flight, builds
 * the tables on the host, uploads them and replaces the previous model; NULL detaches; a failure leaves the previous model in force and the
 * engine usable.  Counters: "lm_ngrams", "lm_states", "lm_max_probe" (0 when detached). */
#define NASR_LM_MAX_ORDER 5
#define NASR_LM_BOS 1025
#define NASR_LM_EOS 1026
typedef struct nasr_lm_desc {
    int32_t order, flags;            /* 1 .. 5; 0 */
    int64_t n_ngrams;
    const int32_t *lengths;          /* [n] */
    const int32_t *tokens;           /* concatenated, oldest first */
    const float *logprob;            /* [n] natural log */
    const float *backoff;            /* [n] or NULL = all 0 */
    float unk_logprob, weight, token_bonus, reserved;
} nasr_lm_desc;
int nasr_engine_set_lm(nasr_engine *e, const nasr_lm_desc *lm);              /* NULL detaches */
int nasr_engine_set_lm_weights(nasr_engine *e, float weight, float token_bonus);
/* the LM side of hypothesis `rank` of utterance u of the LAST beam call, which must have run with a model attached (else < 0; ranks are by
 * total): *lm_logprob_out = lm with the EOS term included when the model has one, *total_out = score + weight * that + token_bonus *
 * tokens, both as the device computed them; token_lm_logprobs_out gets min(count, cap) per-token LM terms (EOS not among them), recomputed
 * on the host by the same lookup.  Returns the token count.  Any pointer may be NULL.  A nasr_engine_set_lm after the beam call (another
 * model or NULL) ends this read-out: the call then fails; nasr_engine_set_lm_weights does not. */
int nasr_engine_beam_hypothesis_lm(nasr_engine *e, int u, int rank, double *lm_logprob_out, double *total_out,
                                   float *token_lm_logprobs_out, int32_t cap);

/* ---- shallow fusion in the greedy decode: live streams and nasr_engine_transcribe (csrc/nasr_lm.h).
 * Engine option "lm_fusion" (0 default / 1), a capability like "phrase_boost": it selects the decode launches that are captured into the step
 * graphs and allocates a state and a 1040-entry bias row per stream, so it is REJECTED after the first step or offline call.  With it the
 * model attached by nasr_engine_set_lm also biases the greedy device decode.  A stream carries an LM state s: the model's start (the state
 * after BOS, or the empty context) after nasr_stream_create, both reset modes, nasr_stream_set_lm, nasr_engine_set_lm and at the start of every
 * offline utterance; it runs on across steps, chunks, pipelined calls and endpoints.  With the greedy weights (weight, token_bonus):
 *     lmbias(v) = (float)((double)weight * ln P_lm(v | s) + (double)token_bonus)   for v in 0 .. 1023, product and sum rounded on their own
 *     lmbias(blank) = 0;  every entry 0 when no model is attached or the stream is switched off
 *     token = arg-max_v (logit[v] + (boostbonus(v) + lmbias(v))), all f32, first maximum wins; boostbonus is "phrase_boost"'s, 0 when that is off
 * On emission s becomes the state the lookup leads to; blank leaves it alone.  The model scores the whole vocabulary, so unlike in the beam
 * search it can propose a token; blank gets no LM term, which token_bonus is there to offset; there is no EOS term.  The 10-symbol cap,
 * state commit, frame numbering and the iteration statistic are unchanged, and the values of "token_logprobs", "token_alternatives" and
 * "frame_blank_logprobs" stay the model's (raw logits), as with boosting.  With weights 0 / 0 (the default) or no model every result is
 * bit-identical to "lm_fusion" = 0.  The beam search and alignment are untouched.
 * nasr_engine_set_greedy_lm_weights: finite in [0, 100] each, separate from the beam's weights (the useful values differ); completes steps in
 * flight, keeps every stream's state and takes effect at the next step -- captured graphs stay valid, as they do across nasr_engine_set_lm.
 * nasr_stream_set_lm: per-stream switch (default on); either way the stream's LM state restarts.
 * NASR_FLAG_NO_LM decodes one nasr_engine_transcribe / _transcribe_mel call unfused; the step, beam and align entries reject it.
 * Both setters fail without the option. */
int nasr_engine_set_greedy_lm_weights(nasr_engine *e, float weight, float token_bonus);
int nasr_stream_set_lm(nasr_stream *s, int enable);

/* ---- phrase boosting inside the beam search (csrc/nasr_beam.h, csrc/nasr_boost.h).  A beam call with
 * NASR_FLAG_BEAM_BOOST applies the engine's boost set (nasr_engine_set_boost_phrases; the bonus definition is that of the greedy decode).  The
 * flag needs engine option "phrase_boost" > 0 and excludes NASR_FLAG_NO_BOOST: otherwise the call fails with a message and the engine stays
 * usable.  Without the flag a beam call is what it was: same kernels, same bits.
 * A hypothesis carries boost_state, the automaton state after its tokens from the root (blank never moves it), and boost, the double sum of
 * bonus(state before y_i, y_i) over its tokens.
 * Proposal: a hypothesis in state s expands from its row's 8 largest keys of logit[v] + bonus(s, v) (the f32 sum of the greedy boosted
 * decode; descending, the lower id first among equal bits), blank dropped, the first `beam` of the rest kept -- so a boosted token outside the
 * row's largest raw outputs IS proposed, which the language model never does.  The per-token ln P stays the MODEL's, from the raw logit.
 * Ranking: everywhere the search compares keys the key is (score + weight * lm + token_bonus * tokens) + boost, or score + boost without a
 * model; boost is added last as one rounded double add.  score, the per-token ln P and the frames keep their meaning: one lattice path.
 * A boosted call with a non-empty set runs unpruned (a positive bonus breaks the prune's proof).  With the empty set every result equals the
 * unflagged call bit for bit, with or without a model.
 * Known limit: no retraction -- a partial match that later fails keeps the bonus it was paid, as in the greedy decode.
 * nasr_engine_beam_hypothesis_boost reads the boost side of hypothesis `rank` of utterance u of the LAST beam call, which must have been
 * boosted (else < 0): *boost_out = boost and *total_out = the ranking key, both as the device computed them (after a boosted call with a
 * model attached nasr_engine_beam_hypothesis_lm's total_out is this same key); token_bonus_out gets min(count, cap) per-token bonuses, fixed
 * when the call ended from the set it ran with -- a later nasr_engine_set_boost_phrases does not change them.  Returns the token count.  Any
 * pointer may be NULL. */
int nasr_engine_beam_hypothesis_boost(nasr_engine *e, int u, int rank, double *boost_out, double *total_out, float *token_bonus_out,
                                      int32_t cap);

/* ---- frame history of a live stream: second-pass greedy / beam / alignment over frames the stream has already encoded (engine option
 * "frame_history" = N; the reference has none: its offline entries take audio and run their own encoder).  With the option every step
 * appends the joint's encoder-projection rows of the frames it decodes to a ring of N rows in the stream's slot (csrc/nasr_history.h).
 * Frames are numbered from create / reset as by nasr_stream_get_token_frames; `done` = the frames decoded so far, what
 * nasr_stream_get_frame_blank_logprobs(s, 0, 0, NULL) returns.  A stream keeps frames [max(valid_from, done - N), done): valid_from is 0 after
 * nasr_stream_create and both reset modes, and `done` of the source after nasr_stream_fork / nasr_stream_restore (the history does not
 * travel).  The ring is never cleared and every read is checked against that range, so what a recycled slot or an earlier life of the stream
 * left in it is never visible.
 * nasr_stream_history_range: frames [*first_out, *first_out + *count_out) of s are kept.  Completes steps in flight.  Fails -- with a message,
 * the engine usable -- on a null argument and when the option is off. */
int nasr_stream_history_range(const nasr_stream *s, int64_t *first_out, int32_t *count_out);
/* parity read-out: the kept rows of frames [first, first + count) of s -> out [count][640] f32.  Returns the number of frames written
 * (= count), 0 for a range that is not wholly kept (and for count = 0), < 0 on error: a null stream, a null out with count > 0, a negative
 * range, the option off.  Completes steps in flight; changes nothing. */
int nasr_stream_get_history(const nasr_stream *s, int64_t first, int32_t count, float *out);
/* The three offline modes over window [first[b], first[b] + count[b]) of streams[b], b = 0 .. B - 1: nasr_engine_history_transcribe is
 * nasr_engine_transcribe, nasr_engine_history_beam is nasr_engine_transcribe_beam, nasr_engine_history_align is nasr_engine_align, each with
 * its twin's remaining arguments, outputs and failures -- but no front end and no encoder runs: a gather launch copies the windows' kept rows
 * into the packed rows the mode reads, then the mode runs unchanged (the same sub-batches under "offline_rows").
 *  - A fresh decode of the window.  The decoder starts from the zero state and blank, with an empty boost history and the LM's start state,
 *    exactly as an offline utterance starts: the window is meant to be an utterance between two endpoints, and the result is NOT the
 *    continuation of the stream's own decode at `first`.  Frames in every output are relative to first[b]; the caller adds it.  The prompt
 *    is the one the stream had when the frames were encoded (it is fused into the rows); there is no prompt_index.
 *  - Windows.  A window that is not wholly kept fails the call with a message that names the stream's index, the window and the kept range;
 *    so does count[b] > NASR_OFFLINE_MAX_FRAMES (never kept: N <= 2048).  count[b] = 0 gives what T = 0 gives in the offline entries.  The
 *    same stream may appear in several rows, and the streams need not share right_context.
 *  - Call contract.  The calls complete steps in flight, run eagerly and synchronise; they change no stream in any bit (K/V, caches,
 *    decoder state, token rings, the history itself), capture no graph and invalidate none.  They reject NASR_FLAG_NO_SYNC and accept the
 *    flags of their twins: NASR_FLAG_NO_BOOST and NASR_FLAG_NO_LM (transcribe), NASR_FLAG_BEAM_BOOST (beam).  Like every offline call each
 *    one forgets the read-outs of the call before; they fail with a message, the engine usable, when the option is off, on null streams /
 *    first / count and on a stream of another engine.
 *  - Results are read with the offline read-outs, which behave as after the twin: nasr_engine_beam_hypothesis, _lm and _boost,
 *    nasr_engine_offline_token_logprobs, _token_alternatives and _frame_blank_logprobs, nasr_engine_align_lattice.  The encoder taps of
 *    nasr_engine_offline_tap are empty after such a call.  Results of a window are bit-identical whatever else is in the batch.
 * Engine counters "history_calls" and "history_frames". */
int nasr_engine_history_transcribe(nasr_engine *e, nasr_stream *const *streams, int B, const int64_t *first, const int32_t *count,
                                   int32_t *const *tokens_out, const int32_t *tokens_cap, int32_t *n_tokens, int32_t *const *frames_out, uint32_t flags);
int nasr_engine_history_beam(nasr_engine *e, nasr_stream *const *streams, int B, const int64_t *first, const int32_t *count,
                             const nasr_beam_params *params, int32_t *n_hyps, uint32_t flags);
int nasr_engine_history_align(nasr_engine *e, nasr_stream *const *streams, int B, const int64_t *first, const int32_t *count,
                              const int32_t *const *tokens, const int32_t *n_tokens, double *loglik_out, double *best_out,
                              int32_t *const *frames_out, float *const *token_logprobs_out, uint32_t flags);

/* ---- diarization side-car (BASELINE config 5): MarbleNet VAD + TitaNet-L speaker embeddings ----------------------
 * Replaces the compute of vad_session / spk_session (src/diarize_vad.h:95-135, src/diarize_spk.h:95-120).  weights =
 * the tensors of diarize.gguf ("vad.*" and/or "spk.*", F32, layouts of scripts/convert_diarize_to_gguf.py:129-158),
 * same descriptor type as nasr_engine_create.  The onset/offset state machine, sub-segment cursor, NME-SC clustering and
 * RTTM output of src/diarize_pipeline.cpp / src/diarize_cluster.cpp are host control flow ABOVE this ABI:
 * nemotron-asr.cpp_amd/host/diarize_pipeline_amd.h, diarize_cluster_amd.h. */
typedef struct nasr_diar nasr_diar;
/* dtype: NASR_DTYPE_BF16 = TitaNet's pointwise convolutions on the bf16 MFMA (f32 accumulate), NASR_DTYPE_F32 = all f32;
 * MarbleNet is f32 (P(speech) within 2e-5 of the reference arithmetic) unless NASR_DIAR_VAD_BF16 is OR'ed in: then its pointwise
 * convolutions run on the bf16 MFMA with bf16 activation planes (3 workgroups per CU instead of 1; P(speech) within a few 1e-3).
 * max_windows / max_segments size the scratch (larger calls are tiled). */
#define NASR_DIAR_VAD_BF16 0x100
/* the same kernel with IEEE-half planes and weights on the f16 MFMA (same rate, 11 significand bits instead of 8: an eighth of the
 * bf16 planes' rounding -- logit error 0.006 against 0.04, P(speech) within 1e-4 of the f32 kernel on the synthetic network;
 * segment-level comparison in profiles/r4_vad_16bit_segments.md, tests/test_gpu_diar.py); values saturate at 65 504 */
#define NASR_DIAR_VAD_F16  0x200
int  nasr_diar_create(nasr_diar **out, int device_id, int dtype, const nasr_weight_desc *weights, int n_weights,
                      int max_windows, int max_segments);
void nasr_diar_destroy(nasr_diar *d);
/* the side-car's work goes onto a stream the caller owns (hipStream_t, e.g. from nasr_engine_lend_stream) until nasr_diar_destroy */
int  nasr_diar_set_stream(nasr_diar *d, void *hip_stream);
/* vad_session_run_batch (src/diarize_vad.cpp:490-503) for B buffers in one launch sequence: P(speech) of every 0.63 s
 * window (10 080 samples) of audio[b] at a 10 ms shift (the reference runs each window as its own graph,
 * src/diarize_pipeline.cpp:204-211).  audio: float samples in [-1, 1], or s16 PCM cast to the pointer type with
 * NASR_FLAG_AUDIO_S16; host memory, or device memory with NASR_FLAG_PCM_DEVICE;
 * n_windows[b] = 1 + (n_samples[b] - 10080) / 160, or 0. */
int  nasr_diar_vad(nasr_diar *d, int B, const float *const *audio, const int32_t *n_samples, float *const *probs_out,
                   const int32_t *probs_cap, int32_t *n_windows, uint32_t flags);
/* spk_session_run_chunk (src/diarize_spk.cpp:601-626) for S sub-segments at once: audio[s] holds 24 000 samples (zero
 * padded by the caller), lens_samples[s] of them real; emb_out = [S][192]. */
int  nasr_diar_embed(nasr_diar *d, int S, const float *const *audio, const int32_t *lens_samples, float *emb_out, uint32_t flags);

/* measurement: device time (ms) of the LAST nasr_diar_vad (which = 0) / nasr_diar_embed (which = 1) call's launch sequence, from HIP events on the
 * side-car's own stream around its kernels (staging copies and the read-back excluded) -- what bench.py prices configs[4]'s roofline with.  The
 * reference has no counterpart (it times whole sessions on the host, src/diarize_pipeline.cpp). */
int  nasr_diar_last_gpu_ms(nasr_diar *d, int which, float *ms_out);

/* parity tap: diarize_compute_logmel (src/diarize_audio.cpp:136-227) of one whole host buffer on the device front end,
 * which = 0: the 'vad.*' filterbank, 1: 'spk.*'.  mel_out = [80][t_padded] row-major like the reference's output
 * (t_padded = t_valid rounded up to 16, t_valid = n_samples / 160); this is what tests/test_diarize_preproc.cpp checks
 * against the NeMo fixture (threshold 1e-3). */
int  nasr_diar_logmel(nasr_diar *d, int which, const float *audio, int32_t n_samples, int per_feature_normalize,
                      float *mel_out, int64_t cap, int32_t *t_valid_out);

#ifdef __cplusplus
}
#endif
#endif /* NEMOTRON_ASR_AMD_H */
