// nemo_amd.h -- host-side mirror of the reference's streaming interface on top of the C ABI
// (include/nemotron_asr_amd.h).  Same names, argument meaning and error behaviour as
// reference src/nemo-stream.h:271-326 and src/nemo-ggml.h (nullptr / false / "" + a line on stderr),
// so a caller written against the reference (src/transcribe_stream.cpp, src/nemo-server.cpp)
// compiles against this header unchanged.  The GGUF file is read with host/gguf_reader (no ggml).
#pragma once
#include <cmath>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "nasr_endpoint.h"          // csrc/: the endpoint detector, pure host code

struct nasr_engine;
struct nasr_stream;

struct nemo_hparams {               // reference src/nemo-ggml.h:37-55
    int32_t n_mels = 128, d_model = 1024, n_heads = 8, d_head = 128, d_ff = 4096, n_layers = 24;
    int32_t vocab_size = 1025, decoder_dim = 640, joint_dim = 640, subsampling_factor = 8;
    int32_t att_left_context = 70, kernel_size = 9, num_prompts = 0;
    int32_t blank_token() const { return vocab_size - 1; }
};

struct nemo_context {               // reference: nemo_context / nemo_model (src/nemo-ggml.h:240-252)
    nemo_hparams hparams;
    std::vector<std::string> vocab;
    std::map<std::string, int> prompt_dict;
    int prompt_index = -1;          // default language prompt (101 = "auto") for multilingual models
    nasr_engine *engine = nullptr;
    int max_streams = 0;
    int token_alternatives = 0;      // K of nemo_set_token_alternatives (0: off)
    bool token_logprobs = false;     // nemo_set_token_logprobs
    int token_entropy_milli = 0;     // round(1000 alpha) of nemo_set_token_entropy (0: off)
    bool lm_attached = false;        // nemo_load_lm_arpa succeeded and nemo_clear_lm has not been called
    bool beam_boost = false;         // nemo_set_beam_boost: nemo_transcribe_beam applies the boost phrases inside the search
    int workspace_rows = 0;          // rows one engine call may carry (streams x chunks x (1 + right_context)); nasr_engine_create_ex
};

enum class nemo_latency_mode { PURE_CAUSAL = 0, ULTRA_LOW = 1, LOW = 6, DEFAULT = 13 };   // src/nemo-stream.h:15-20

struct nemo_cache_config {          // the caller-visible part of reference src/nemo-stream.h:23-128
    int32_t att_left_context = 70, att_right_context = 0;
    int32_t subsampling_factor = 8, n_mels = 128, sample_rate = 16000, hop_length = 160;
    int32_t pre_encode_cache_size = 9, drop_extra_pre_encoded = 2;
    size_t get_chunk_mel_frames() const { return (size_t)(pre_encode_cache_size + subsampling_factor * (1 + att_right_context)); }
    size_t get_shift_mel_frames() const { return (size_t)(subsampling_factor * (1 + att_right_context)); }
    int32_t get_chunk_samples() const { return (int32_t)get_chunk_mel_frames() * hop_length; }
    int32_t get_latency_ms() const { return (int32_t)get_chunk_mel_frames() * hop_length * 1000 / sample_rate; }
    int32_t get_valid_out_len() const { return 1 + att_right_context; }
    static nemo_cache_config with_latency(nemo_latency_mode m) { nemo_cache_config c; c.att_right_context = (int32_t)m; return c; }
    static nemo_cache_config default_config() { return with_latency(nemo_latency_mode::PURE_CAUSAL); }
};

struct nemo_stream_context {        // reference src/nemo-stream.h:177-262 (host-visible members)
    nemo_context *nctx = nullptr;
    nemo_cache_config config;
    nasr_stream *stream = nullptr;
    int prompt_index = -1;
    int audio_rate = 16000, audio_encoding = 0, audio_channels = 1, audio_channel = 0;      // nemo_stream_set_audio_format (default: s16 16 kHz mono)
    std::vector<int> tokens;
    // nemo_stream_set_endpointing / nemo_stream_get_endpoints: the detector's state, the frames and device tokens it has consumed, the events so far
    bool ep_on = false;
    nasr_endpoint::Config ep_cfg;
    nasr_endpoint::State ep_state;
    int64_t ep_frames = 0, ep_tokens = 0;
    std::vector<nasr_endpoint::Event> ep_events;
    std::string transcript;
    double total_audio_seconds = 0, total_compute_seconds = 0;
    int total_chunks_processed = 0;
    double rtf() const { return total_audio_seconds > 0 ? total_compute_seconds / total_audio_seconds : 0; }
};

// ---- model (reference src/nemo-ggml.cpp:444-540) ------------------------------------------------
// dtype: 0 = f32, 1 = bf16 (NASR_DTYPE_*).  Returns nullptr on failure (message on stderr).
nemo_context *nemo_init_with_device(const char *model_path, int device, int dtype, int max_streams);
// ... with room for several chunks of every stream in one engine call (a server's backlog): workspace_rows >= max_streams x 14, 0 = default
nemo_context *nemo_init_with_rows(const char *model_path, int device, int dtype, int max_streams, int workspace_rows);
nemo_context *nemo_init(const char *model_path);              // device 0, bf16, 64 streams
void nemo_free(nemo_context *ctx);
bool nemo_set_language(nemo_context *ctx, const char *lang);  // default prompt for new streams
// MI355X extension: pipelined steps (nasr_engine_set_option "pipeline"): the decode of one call runs beside the encoder of the
// next; nemo_stream_process_incremental then returns each text delta one call later, nemo_stream_finalize returns the rest
// MI355X extension: per-token log-probabilities (nasr_engine_set_option "token_logprobs"); before the first stream processes audio
bool nemo_set_token_logprobs(nemo_context *ctx, bool on);
// MI355X extension: per-frame blank log-probabilities (nasr_engine_set_option "frame_blank_logprobs"), the input of the endpoint detector; before
// the first stream processes audio
bool nemo_set_frame_blank_logprobs(nemo_context *ctx, bool on);
// MI355X extension: per-token entropies of order alpha (nasr_engine_set_option "token_entropy" = round(1000 alpha): 1 = Shannon, 0.333 = the
// usual 1/3, 0 = off; accepted 0.05 .. 0.9, 1 and 1.1 .. 4), the input of entropy-based confidence (token_confidence.h); before the first
// stream processes audio
bool nemo_set_token_entropy(nemo_context *ctx, float alpha);
// MI355X extension: the K = 1 .. 8 most probable joint outputs at every emission (nasr_engine_set_option "token_alternatives"; 0 = off); before
// the first stream processes audio
bool nemo_set_token_alternatives(nemo_context *ctx, int k);
// MI355X extension: phrase boosting ("hotwords"; nasr_engine_set_option "phrase_boost" + nasr_engine_set_boost_phrases).
// nemo_set_phrase_boost: before the first stream processes audio; max_states = capacity of the phrase automaton, 2 .. 4096 (one state per
// distinct phrase prefix + 2), 0 = off.  nemo_set_boost_phrases: any time afterwards; phrases as text (boost_phrases.h: each word segmented by
// greedy longest match against the vocabulary, or `ids:12,55,9`), bonus[i] in natural-log units (a shorter list: default_bonus).  Phrases that
// cannot be converted are reported on stderr and skipped; returns false if the engine refuses the set (the previous one then stays).  Every
// stream's boost history restarts.  nemo_load_boost_file: the same from a file, one `phrase<TAB>bonus` per line (bonus optional).
bool nemo_set_phrase_boost(nemo_context *ctx, int max_states);
bool nemo_set_boost_phrases(nemo_context *ctx, const std::vector<std::string> &phrases, const std::vector<float> &bonus, float default_bonus = 4.0f);
bool nemo_load_boost_file(nemo_context *ctx, const char *path, float default_bonus = 4.0f);
bool nemo_set_pipeline(nemo_context *ctx, int depth);   // 0 off, 1 decode beside the next encoder, 2 / 3 / 4: the encoder in that many pieces of consecutive steps side by side

// MI355X extension: forced alignment / transcript scoring of one whole utterance (nasr_engine_align): tokens = ids 0 .. 1023 of a KNOWN
// transcript (at most 1024).  loglik = ln P(tokens | audio), best = the best path's score, frames[i] = the encoder frame (80 ms each) at which
// token i is emitted on that path, logprobs[i] = ln P of token i there.  The context's language prompt applies.  ok = false on failure
// (the reason on stderr)
struct nemo_alignment {
    bool ok = false;
    double loglik = 0.0, best = 0.0;
    std::vector<int32_t> frames;
    std::vector<float> logprobs;
};
nemo_alignment nemo_align_audio(nemo_context *ctx, const int16_t *audio, int n_samples, const std::vector<int32_t> &tokens);

// MI355X extension: offline transcription of one whole utterance with the frame-synchronous beam search (nasr_engine_transcribe_beam): the
// nbest distinct transcripts, best first, each with its score (the ln P of its best-scoring lattice path), the encoder frame of every token
// and its ln P.  beam 1 .. 8, nbest 0 = beam, max_symbols 0 = the default; beam = 0 is the greedy offline transcription
// (nasr_engine_transcribe: one hypothesis, score NAN; logprobs is filled after nemo_set_token_logprobs and entropies after
// nemo_set_token_entropy, both empty otherwise, and a read-out that fails fails the call; it is boosted whenever phrase boosting is on).  In beam calls
// phrase boosting is applied only after nemo_set_beam_boost(ctx, true).  Empty on failure (the reason on stderr)
struct nemo_hypothesis {
    double score = 0.0;
    std::vector<int32_t> tokens, frames;
    std::vector<float> logprobs;
    std::vector<float> entropies;    // beam = 0 only, after nemo_set_token_entropy: the entropy at every token (beam = 0 also fills logprobs after nemo_set_token_logprobs)
    bool has_lm = false;             // a language model was attached (nemo_load_lm_arpa): ranks are by `total`
    double lm_logprob = 0.0, total = 0.0;      // ln P_LM of the transcript (EOS term included when the model has one); score + weight * lm + bonus * tokens
    bool has_boost = false;          // the search was boosted (nemo_set_beam_boost): ranks are by `total`, which then also includes `boost`
    double boost = 0.0;              // the sum of the tokens' phrase bonuses
    std::vector<float> token_bonuses;
};
std::vector<nemo_hypothesis> nemo_transcribe_beam(nemo_context *ctx, const int16_t *audio, int n_samples, int beam, int nbest = 0, int max_symbols = 0);
// the line both command-line tools print for hypothesis `rank` of a beam call: rank score [lm] [boost] [total] text
std::string beam_hypothesis_line(size_t rank, const nemo_hypothesis &h, const std::vector<std::string> &vocab);

// MI355X extension: shallow fusion of a back-off n-gram language model in nemo_transcribe_beam (nasr_engine_set_lm).
// The ARPA file is over the vocabulary's pieces (lm_arpa.h: one piece or `ids:N` per word, <s>, </s>, <unk>; log10 values).  weight and
// token_bonus in [0, 100]; unk_logprob (natural log, <= 0) is needed only when the file has no <unk> unigram (NAN = take the file's).  The model
// re-scores the candidates the transducer proposes; greedy transcription and streams see it only after nemo_set_lm_fusion.  false on failure (the reason on stderr;
// the previous model stays).  nemo_clear_lm detaches it.
bool nemo_load_lm_arpa(nemo_context *ctx, const char *path, float weight, float token_bonus = 0.0f, float unk_logprob = NAN);
bool nemo_clear_lm(nemo_context *ctx);

// MI355X extension: shallow fusion in the GREEDY decode -- live streams and nemo_transcribe_beam with beam = 0 (engine option "lm_fusion";
// DESIGN.md section 17).  nemo_set_lm_fusion(true) right after the context is made, before any stream processes audio; the model is the one of
// nemo_load_lm_arpa, and the greedy decode has weights of its own (both in [0, 100], default 0 / 0 = unfused): arg-max over
// logit + weight * ln P_lm(token | the stream's emitted tokens) + token_bonus for every non-blank token, blank unbiased.  Unlike in the beam
// search the model scores the whole vocabulary, so it can propose a token.  false on failure (the reason on stderr)
bool nemo_set_lm_fusion(nemo_context *ctx, bool enable);
bool nemo_set_greedy_lm_weights(nemo_context *ctx, float weight, float token_bonus = 0.0f);

// MI355X extension: phrase boosting inside nemo_transcribe_beam (NASR_FLAG_BEAM_BOOST), with or without a language
// model.  It needs nemo_set_phrase_boost and a boost set (nemo_set_boost_phrases / nemo_load_boost_file); unlike the language model the
// boost also PROPOSES: a boosted token outside a hypothesis' largest outputs enters its expansion list.  Off by default; false when phrase
// boosting is off
bool nemo_set_beam_boost(nemo_context *ctx, bool enable);

// ---- streaming (reference src/nemo-stream.h:271-326) -------------------------------------------------
nemo_stream_context *nemo_stream_init(nemo_context *ctx, const nemo_cache_config *config = nullptr);
bool nemo_stream_set_language(nemo_stream_context *sctx, const char *lang);
std::string nemo_stream_process_incremental(nemo_stream_context *sctx, const int16_t *audio, int n_samples);
// MI355X extension: audio in another format, converted on the device (nasr_stream_set_audio_format / nasr_engine_step_audio): sample_rate 8000,
// 11025, 16000, 22050, 24000, 32000, 44100 or 48000; encoding NASR_AUDIO_S16 / F32 / MULAW / ALAW; channels 1 .. 8 interleaved; channel = an
// index, or -1 for the mean.  Set it before the stream's first audio (or right after a reset); then push with nemo_stream_process_audio, whose
// n_frames counts sample times with all channels.  nemo_stream_finalize flushes the converter's tail.
bool nemo_stream_set_audio_format(nemo_stream_context *sctx, int sample_rate, int encoding, int channels, int channel);
std::string nemo_stream_process_audio(nemo_stream_context *sctx, const void *audio, int n_frames);
std::string nemo_stream_finalize(nemo_stream_context *sctx);
// MI355X extension: a second stream that continues from where sctx is now (nasr_stream_fork: one device launch into a free slot of the
// engine); the mirror's own transcript, tokens and endpoint detector state are copied too, and the two are independent from then on.
// nullptr on failure (no free slot; the reason on stderr).  Free it with nemo_stream_free
nemo_stream_context *nemo_stream_fork(nemo_stream_context *sctx);
// MI355X extension: the stream as bytes in host memory, and a stream made from such bytes (nasr_stream_save / nasr_stream_restore: the live
// part of the slot and the engine's mirror, checksummed) -- to park an idle stream and give its slot away, to move it to another context or
// device, to resume it in a later process.  Around the engine's blob goes what nemo_stream_fork carries beside the engine stream:
// transcript, tokens, language prompt, audio format, endpoint detector state and events (stream_envelope.h).  save leaves sctx as it is;
// restore needs a context with the same model, dtype and decode options (boost set and language model included) and a free slot, and
// returns nullptr on failure (the reason on stderr).  Free the result with nemo_stream_free
bool nemo_stream_save(nemo_stream_context *sctx, std::vector<uint8_t> &out);
nemo_stream_context *nemo_stream_restore(nemo_context *ctx, const uint8_t *data, size_t size);
// MI355X extension: the text nemo_stream_finalize would add if it were called now -- the tentative tail of a caption at a long right
// context -- without ending or changing the stream (nasr_engine_preview; it needs one free slot).  "" when nothing is buffered or on failure
std::string nemo_stream_preview(nemo_stream_context *sctx);
// MI355X extension: a second pass over frames the stream has already encoded (engine option "frame_history"): the
// beam search of nemo_transcribe_beam, or the alignment of nemo_align_audio, over encoder frames [first, first + count) of the stream --
// e.g. an utterance of nemo_stream_get_endpoints: first = utt_start, count = frame + 1 - utt_start -- with no audio and no encoder run.
// nemo_set_frame_history(ctx, frames) before the first stream processes audio: frames kept per stream, 64 .. 2048 in multiples of 64 (0 =
// off); nemo_stream_history_range: the frames the stream keeps now.  A second pass is a fresh decode of the window (zero decoder state, the
// LM's start state, an empty boost history); frames in its results count from `first`.  The language model of nemo_load_lm_arpa and
// nemo_set_beam_boost apply as in nemo_transcribe_beam.  The stream, its transcript and its tokens are not changed.  Empty / ok = false on
// failure (a window that is not wholly kept, the option off: the reason on stderr)
bool nemo_set_frame_history(nemo_context *ctx, int frames);
bool nemo_stream_history_range(nemo_stream_context *sctx, int64_t *first, int *count);
std::vector<nemo_hypothesis> nemo_stream_second_pass_beam(nemo_stream_context *sctx, int64_t first, int count, int beam, int nbest = 0, int max_symbols = 0);
nemo_alignment nemo_stream_second_pass_align(nemo_stream_context *sctx, int64_t first, int count, const std::vector<int32_t> &tokens);
std::string nemo_stream_get_transcript(nemo_stream_context *sctx);
const std::vector<int> &nemo_stream_get_tokens(nemo_stream_context *sctx);
void nemo_stream_reset(nemo_stream_context *sctx);
// MI355X extension: phrase boosting on / off for this stream (default on; nasr_stream_set_boost); its boost history restarts either way
bool nemo_stream_set_boost(nemo_stream_context *sctx, bool enable);
void nemo_stream_free(nemo_stream_context *sctx);

// MI355X extension: one launch sequence for B streams that share right_context.  out[b] receives the
// text delta of stream b.  This is what a multi-stream server's worker calls instead of looping.
bool nemo_stream_process_batch(nemo_stream_context *const *sctx, int B, const int16_t *const *audio,
                               const int *n_samples, std::string *out);
// MI355X extension: with pipelined steps, complete the steps in flight of B streams (one engine) and return their text --
// what a batch former calls when its queue runs empty (nasr_engine_collect)
bool nemo_stream_collect_batch(nemo_stream_context *const *sctx, int B, std::string *out);

// MI355X extension: nemo_stream_finalize for B streams of one engine in ONE tail-flush launch sequence (a server ends many
// sessions at once); out[b] += the text the flush (and, with pipelined steps, what was still in flight) produced
bool nemo_stream_finalize_batch(nemo_stream_context *const *sctx, int B, std::string *out);

// token ids -> text: U+2581 starts a word (reference src/nemo-ggml.cpp:1556-1583); ids outside the vocab are skipped
std::string tokens_to_text(const std::vector<int> &tokens, const std::vector<std::string> &vocab);

// reference src/nemo-ggml.h:383-395: a token with the encoder frame it was emitted on (80 ms per frame)
struct timed_token {
    int token_id;
    int64_t frame_idx;
    timed_token(int id = 0, int64_t frame = 0) : token_id(id), frame_idx(frame) {}
    float to_seconds(int frame_samples = 1280, int sample_rate = 16000) const { return (float)frame_idx * frame_samples / sample_rate; }
};
// every token of the stream since init/reset with its frame (the engine keeps the frames of the last 4096 tokens)
std::vector<timed_token> nemo_stream_get_timed_tokens(nemo_stream_context *sctx);
// ln P(token) of every token of the stream since init/reset (needs nemo_set_token_logprobs; NaN for tokens that have left the
// engine's 4096-token ring, as their frame is -1); word confidences from them: word_confidence.h
std::vector<float> nemo_stream_get_token_logprobs(nemo_stream_context *sctx);
// the entropy of order alpha at every token of the stream since init/reset (needs nemo_set_token_entropy; NaN for tokens that have left the
// engine's 4096-token ring); token and word confidences from them: token_confidence.h
std::vector<float> nemo_stream_get_token_entropies(nemo_stream_context *sctx);
// ln P(blank) at the last joint evaluation of every encoder frame of the stream since init/reset (needs nemo_set_frame_blank_logprobs; NaN for
// frames that have left the engine's 4096-frame ring).  Completes steps in flight
std::vector<float> nemo_stream_get_frame_blank_logprobs(nemo_stream_context *sctx);
// endpointing (csrc/nasr_endpoint.h; needs nemo_set_frame_blank_logprobs): nemo_stream_set_endpointing turns it on with the given rules (nullptr:
// the defaults) and restarts the detector at the stream's next frame.  nemo_stream_get_endpoints completes steps in flight, runs the detector
// over the frames decoded since the last call -- their blank log-probabilities and the frames of the device's tokens (timed_token.frame_idx) --
// and returns every event since set_endpointing / reset: utterance = frames [utt_start, frame], `tokens` tokens; the utterances' tokens follow one
// another in the stream's token order, so utterance i starts at token sum(tokens of events before i).  Call it at least every 4096 frames
// (5.5 minutes): frames that have left the engine's ring count as not silent
bool nemo_stream_set_endpointing(nemo_stream_context *sctx, const nasr_endpoint::Config *cfg);
const std::vector<nasr_endpoint::Event> &nemo_stream_get_endpoints(nemo_stream_context *sctx);
// the K alternatives of every token of the stream since init/reset (needs nemo_set_token_alternatives): row i of ids / logprobs [n_tokens][k]
// belongs to token i, descending probability, ids 0 .. 1024 (1024 = blank), logprobs = ln P; tokens that have left the engine's
// 4096-token ring get ids -1 and NaN.  k = 0 and empty when the option is off
struct nemo_token_alternatives {
    int k = 0;
    size_t n_tokens = 0;
    std::vector<int32_t> ids;
    std::vector<float> logprobs;
};
nemo_token_alternatives nemo_stream_get_token_alternatives(nemo_stream_context *sctx);
// reference src/nemo-ggml.cpp:1556-1583: "{12.34}" in front of every word when timestamp_words is set
std::string tokens_to_text(const std::vector<timed_token> &tokens, const std::vector<std::string> &vocab, bool timestamp_words);
