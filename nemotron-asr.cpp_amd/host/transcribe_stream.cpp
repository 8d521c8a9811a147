// nemotron-asr-amd -- streaming transcription CLI with the argv / stdout contract of the reference's
// `nemotron-asr.cpp` binary (reference src/transcribe_stream.cpp:33-297): positional
// `model.gguf audio.pcm [chunk_ms] [right_context]`, s16le 16 kHz mono from a file or stdin ("-"),
// text deltas on stdout as they are produced, configuration and the RTF summary on stderr.
// --input-rate / --input-encoding / --input-channels / --input-channel: audio in another format, converted on the device; a file that
// starts with RIFF....WAVE sets them from its header (wav_header.h).
// --diarize <diarize.gguf> [--rttm F] [--speaker-text F] [--json F] [--num-speakers K] [--sub-shift SEC] run the
// diarization pipeline beside the ASR stream like the reference's CLI (:146-170, :243-290).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <cmath>

#include "diarize_pipeline_amd.h"
#include "nemo_amd.h"
#include "nemotron_asr_amd.h"
#include "wav_header.h"
#include "word_confidence.h"
#include "token_confidence.h"

static void usage(const char *prog) {
    fprintf(stderr,
            "Usage: %s <model.gguf> <audio.pcm | -> [chunk_ms] [right_context] [--lang CODE] [--f32] [--device N] [--print-tokens] [--read-chunks N] [--timestamps] [--confidence] [--confidence-method M] [--confidence-alpha A] [--confidence-norm N] [--confidence-agg G] [--alternatives K] [--endpoints] [--preview] [--save-state FILE] [--load-state FILE] [--boost-file FILE] [--boost-bonus X] [--lm FILE.arpa] [--lm-weight X] [--token-bonus Y] [--pipeline [E]] [--input-rate N] [--input-encoding s16|f32|mulaw|alaw] [--input-channels C] [--input-channel I|mix]\n"
            "  audio: raw s16le, 16 kHz, mono, unless the --input-* flags or a WAV header say otherwise.  right_context in {0, 1, 6, 13} (80 ms .. 1.12 s lookahead)\n"
            "  --input-rate N:  sample rate of the audio: 8000, 11025, 16000, 22050, 24000, 32000, 44100 or 48000 (converted to 16 kHz on the GPU)\n"
            "  --input-encoding E: s16 (default), f32, mulaw or alaw (G.711).  --input-channels C: 1 .. 8 interleaved channels\n"
            "  --input-channel I|mix: the channel to transcribe, or the mean of all (default: mix when there are several).  A file that starts with\n"
            "                   RIFF....WAVE (PCM 16-bit, IEEE float 32-bit, mu-law, A-law) sets rate, encoding and channels from its header\n"
            "  --read-chunks N: read N chunks of audio per call (default 1 = the reference's read size); a file is\n"
            "                   transcribed fastest with N = 256 and --pipeline 4: same transcript, the chunks of a read share one\n"
            "                   launch sequence and consecutive reads run side by side\n"
            "  --timestamps:    print the final transcript again with {seconds} in front of every word\n"
            "  --confidence:    print the final transcript again with [0.93] behind every word: exp of the smallest log-probability among\n"
            "                   the word's tokens under the joint's softmax (with --timestamps: one line, {seconds} in front and [p] behind)\n"
            "  --confidence-method max_prob|entropy|tsallis [--confidence-alpha A] [--confidence-norm lin|exp] [--confidence-agg min|mean|prod]:\n"
            "                   the bracketed number becomes the chosen measure (any of these implies --confidence).  max_prob: P(token); entropy / tsallis:\n"
            "                   the entropy of order A (default 0.333; 1 = Shannon; 0.05 .. 0.9, 1, 1.1 .. 4) of the joint's whole output distribution where\n"
            "                   the token was emitted, mapped to [0, 1] linearly or exponentially (default exp).  A word's number is the min (default),\n"
            "                   the mean or the product of its tokens'.  --confidence-alpha and --confidence-norm go with entropy or tsallis\n"
            "  --alternatives K: after the transcript (and the --timestamps / --confidence line) one line per emitted token, `alt <i> <id>:<p> <id>:<p> ...`\n"
            "                   with K = 1 .. 8 pairs: i = the token's index from 0, then the K most probable joint outputs at that emission (id 1024 =\n"
            "                   blank: the model nearly emitted nothing) with p = their softmax probability as %%.4f, in descending order; without\n"
            "                   --boost-file the first id is the token.  The first line and the --print-tokens line stay as they are\n"
            "  --endpoints:     after the transcript one line per utterance, `endpoint <start s> <end s> rule <r> tokens <n>:<text>`: the stream cut where the\n"
            "                   decoder says the speaker stopped.  rule 1: silence with nothing decoded, 2: silence after speech, 3: maximum length, 0: the\n"
            "                   open utterance at the end of the audio (only if it has tokens).  A frame (80 ms) is silent if it emitted no token and\n"
            "                   P(blank) >= --endpoint-blank-prob P (default 0: every token-less frame).  --endpoint-silence S (rule 2, default 1.2 s),\n"
            "                   --endpoint-idle S (rule 1, default 2.4 s), --endpoint-max S (rule 3, default 20 s); 0 disables a rule\n"
            "  --preview:       after every read one extra line, `~ ` followed by the tentative text of the tail: what the audio still waiting for its right\n"
            "                   context (up to 1.12 s at right_context 13) would add if the stream ended now (a flush on a fork of the stream; the stream goes\n"
            "                   on untouched).  NOTE: the committed transcript is held back and printed when the audio ends, so that every line which does\n"
            "                   not start with `~ ` is the output without the flag; until then only the `~ ` lines appear.  A live caption shows\n"
            "                   committed text + tail: nemo_stream_get_transcript() + nemo_stream_preview() of host/nemo_amd.h\n"
            "  --save-state F:  at the end of the audio do NOT flush the stream: write it to F as a snapshot (nemo_stream_save: the engine's state and the\n"
            "                   transcript so far) and print what has been transcribed so far.  --load-state F: start from such a snapshot instead of a fresh\n"
            "                   stream, with the same model, --f32 or not, and the same --confidence / --alternatives / --endpoints / --boost-file / --lm\n"
            "                   flags; right_context and the input format come from the snapshot.  Two runs over the two halves of a file, the first cut at a\n"
            "                   multiple of the read size, print what one run over the whole file prints, by this rule: the FIRST line of run 1 without its\n"
            "                   newline, followed by the first line of run 2, is the first line of the whole run; every later line of run 2 (--print-tokens,\n"
            "                   --timestamps, --confidence, --alternatives, --endpoints) covers the whole stream and is the whole run's; run 1's later lines do not count\n"
            "  --boost-file F:  phrase boosting: one phrase per line, `phrase<TAB>bonus` (bonus optional, natural-log units added to the logits of the\n"
            "                   phrase's next token).  Words are cut into vocabulary pieces by greedy longest match; `ids:12,55,9` gives token ids literally\n"
            "  --boost-bonus X: the bonus of lines that give none (default 4.0)\n"
            "  --lm FILE.arpa:  shallow fusion of a back-off n-gram model over the vocabulary's pieces (one piece or ids:N per ARPA word, <s>, </s>, <unk>;\n"
            "                   up to 5-grams) in the greedy decode: arg-max over logit + X * ln P_lm(token | tokens so far) + Y for every non-blank token,\n"
            "                   blank unbiased.  --lm-weight X (default 0.5), --token-bonus Y (default 0; it offsets the deletions an unbiased blank causes); 0 .. 100\n"
            "  --second-pass W [--nbest N] [--max-symbols S] [--history-frames F]: a beam search (width W = 1 .. 8) over the encoder frames the stream\n"
            "                   itself has produced (engine option frame_history = F, default 2048; no second encoder run): at the end of the input -- with\n"
            "                   --endpoints at every endpoint, and at the end for an utterance still open -- the N best transcripts of the utterance's frames,\n"
            "                   one line per hypothesis as nemotron-transcribe-amd --beam prints them: rank score [lm] [boost total] text.  The transcript's own\n"
            "                   line is held until the end, as with --preview.  --lm and --boost-file then also act inside the search, as that tool's --beam\n"
            "                   does (the model's --lm-weight / --token-bonus; hypotheses rank by total).  An utterance longer than F frames gets a notice and\n"
            "                   its greedy text instead\n"
            "  --pipeline E:    consecutive reads overlap on the GPU, E = 0..4 (same transcript; each delta appears E reads later).\n"
            "                   1: decode of one read beside the encoder of the next; 2..4: the encoder in E pieces on E hardware queues\n"
            "                   (4 = the fastest way through a file).  --pipeline without a number = 1; --pipeline2 / --pipeline3 still work\n"
            "  --cpu | --cuda | --metal: the reference's backend selectors are accepted and ignored (this build has one backend: MI355X)\n"
            "  --diarize <diarize.gguf> [--rttm <file>] [--speaker-text <file>] [--json <file>] [--num-speakers K] [--sub-shift SEC] [--vad-onset P] [--vad-offset P]\n"
            "                   speaker diarization beside the transcript (speaker-tagged transcript on stdout at EOF)\n", prog);
}

int main(int argc, char **argv) {
    if (argc < 3) { usage(argv[0]); return 1; }
    const char *model_path = argv[1], *audio_path = argv[2];
    int chunk_ms = 80, right_context = 0, device = 0, dtype = 1, positional = 0;
    const char *lang = nullptr;
    bool print_tokens = false, timestamps = false, confidence = false;
    bool conf_entropy_opts = false;
    bool conf_opts = false, conf_max_prob = true;      // --confidence-*: the bracketed number becomes the chosen measure (token_confidence.h)
    token_conf::Method conf_method = token_conf::METHOD_ENTROPY;
    token_conf::Norm conf_norm = token_conf::NORM_EXP;
    token_conf::Agg conf_agg = token_conf::AGG_MIN;
    float conf_alpha = 0.333f;
    const char *boost_file = nullptr, *save_state = nullptr, *load_state = nullptr;
    int alternatives = 0;
    bool endpoints = false, preview = false;
    int second_pass = 0, sp_nbest = 0, sp_symbols = 0, history_frames = 2048;
    nasr_endpoint::Config ep_cfg;
    float boost_bonus = 4.0f;
    const char *lm_path = nullptr;
    float lm_weight = 0.5f, token_bonus = 0.0f;
    bool lm_opts = false;
    int pipeline = 0;
    int read_chunks = 1, num_speakers = -1;
    float sub_shift_sec = 0.75f, vad_onset = -1.0f, vad_offset = -1.0f;
    int in_rate = 16000, in_enc = NASR_AUDIO_S16, in_channels = 1, in_channel = -2;      // -2: not given (one channel: 0, several: the mean)
    std::string diarize_gguf, rttm_path, speaker_text_path, json_path;
    const bool from_stdin = strcmp(audio_path, "-") == 0 || strcmp(audio_path, "--stdin") == 0;
    for (int i = 3; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--lang" && i + 1 < argc) lang = argv[++i];
        else if (a == "--device" && i + 1 < argc) device = atoi(argv[++i]);
        else if (a == "--f32") dtype = 0;
        else if (a == "--print-tokens") print_tokens = true;
        else if (a == "--timestamps") timestamps = true;
        else if (a == "--confidence") confidence = true;
        else if (a == "--confidence-method" && i + 1 < argc) {
            if (!token_conf::parse_method(argv[++i], &conf_max_prob, &conf_method)) { fprintf(stderr, "--confidence-method must be max_prob, entropy or tsallis (got %s)\n", argv[i]); return 1; }
            confidence = conf_opts = true;
        }
        else if (a == "--confidence-alpha" && i + 1 < argc) { conf_alpha = strtof(argv[++i], nullptr); confidence = conf_opts = conf_entropy_opts = true; }
        else if (a == "--confidence-norm" && i + 1 < argc) {
            if (!token_conf::parse_norm(argv[++i], &conf_norm)) { fprintf(stderr, "--confidence-norm must be lin or exp (got %s)\n", argv[i]); return 1; }
            confidence = conf_opts = conf_entropy_opts = true;
        }
        else if (a == "--confidence-agg" && i + 1 < argc) {
            if (!token_conf::parse_agg(argv[++i], &conf_agg)) { fprintf(stderr, "--confidence-agg must be min, mean or prod (got %s)\n", argv[i]); return 1; }
            confidence = conf_opts = true;
        }
        else if (a == "--alternatives" && i + 1 < argc) alternatives = atoi(argv[++i]);
        else if (a == "--endpoints") endpoints = true;
        else if (a == "--preview") preview = true;
        else if (a == "--second-pass" && i + 1 < argc) second_pass = atoi(argv[++i]);
        else if (a == "--nbest" && i + 1 < argc) sp_nbest = atoi(argv[++i]);
        else if (a == "--max-symbols" && i + 1 < argc) sp_symbols = atoi(argv[++i]);
        else if (a == "--history-frames" && i + 1 < argc) history_frames = atoi(argv[++i]);
        else if (a == "--save-state" && i + 1 < argc) save_state = argv[++i];
        else if (a == "--load-state" && i + 1 < argc) load_state = argv[++i];
        else if (a == "--endpoint-silence" && i + 1 < argc) ep_cfg.silence_frames_after_speech = (int)std::lround(atof(argv[++i]) / 0.08);
        else if (a == "--endpoint-idle" && i + 1 < argc) ep_cfg.silence_frames_idle = (int)std::lround(atof(argv[++i]) / 0.08);
        else if (a == "--endpoint-max" && i + 1 < argc) ep_cfg.max_utterance_frames = (int)std::lround(atof(argv[++i]) / 0.08);
        else if (a == "--endpoint-blank-prob" && i + 1 < argc) { const double pb = atof(argv[++i]); ep_cfg.min_blank_logprob = pb > 0.0 ? (float)std::log(pb) : -INFINITY; }
        else if (a == "--boost-file" && i + 1 < argc) boost_file = argv[++i];
        else if (a == "--boost-bonus" && i + 1 < argc) boost_bonus = (float)atof(argv[++i]);
        else if (a == "--lm" && i + 1 < argc) lm_path = argv[++i];
        else if (a == "--lm-weight" && i + 1 < argc) { lm_weight = strtof(argv[++i], nullptr); lm_opts = true; }
        else if (a == "--token-bonus" && i + 1 < argc) { token_bonus = strtof(argv[++i], nullptr); lm_opts = true; }
        else if (a == "--cpu" || a == "--cuda" || a == "--metal")      // reference src/transcribe_stream.cpp:86-88
            fprintf(stderr, "note: %s ignored -- this build runs on the MI355X HIP engine only\n", a.c_str());
        else if (a == "--pipeline") {
            pipeline = 1;
            if (i + 1 < argc && strlen(argv[i + 1]) == 1 && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '4') pipeline = argv[++i][0] - '0';
        }
        else if (a == "--pipeline2") pipeline = 2;
        else if (a == "--pipeline3") pipeline = 3;
        else if (a == "--pipeline4") pipeline = 4;
        else if (a == "--read-chunks" && i + 1 < argc) read_chunks = atoi(argv[++i]);
        else if (a == "--input-rate" && i + 1 < argc) in_rate = atoi(argv[++i]);
        else if (a == "--input-encoding" && i + 1 < argc) {
            const std::string v = argv[++i];
            in_enc = v == "s16" ? NASR_AUDIO_S16 : v == "f32" ? NASR_AUDIO_F32 : v == "mulaw" ? NASR_AUDIO_MULAW : v == "alaw" ? NASR_AUDIO_ALAW : -1;
            if (in_enc < 0) { fprintf(stderr, "--input-encoding must be s16, f32, mulaw or alaw (got %s)\n", v.c_str()); return 1; }
        }
        else if (a == "--input-channels" && i + 1 < argc) in_channels = atoi(argv[++i]);
        else if (a == "--input-channel" && i + 1 < argc) in_channel = strcmp(argv[i + 1], "mix") == 0 ? (++i, -1) : atoi(argv[++i]);
        else if (a == "--diarize" && i + 1 < argc) diarize_gguf = argv[++i];
        else if (a == "--rttm" && i + 1 < argc) rttm_path = argv[++i];
        else if (a == "--speaker-text" && i + 1 < argc) speaker_text_path = argv[++i];
        else if (a == "--json" && i + 1 < argc) json_path = argv[++i];
        else if (a == "--num-speakers" && i + 1 < argc) num_speakers = atoi(argv[++i]);
        else if (a == "--sub-shift" && i + 1 < argc) sub_shift_sec = (float)atof(argv[++i]);
        else if (a == "--vad-onset" && i + 1 < argc) vad_onset = (float)atof(argv[++i]);      // default 0.9 / 0.5 (diar_infer_meeting)
        else if (a == "--vad-offset" && i + 1 < argc) vad_offset = (float)atof(argv[++i]);
        else if (!a.empty() && a[0] == '-') { fprintf(stderr, "Unknown flag: %s\n", a.c_str()); return 1; }
        else if (positional == 0) { chunk_ms = atoi(argv[i]); positional++; }
        else if (positional == 1) { right_context = atoi(argv[i]); positional++; }
    }
    if (read_chunks < 1 || read_chunks > 4096) { fprintf(stderr, "--read-chunks must be in 1..4096 (got %d)\n", read_chunks); return 1; }
    if (lm_opts && !lm_path) { fprintf(stderr, "--lm-weight and --token-bonus go with --lm\n"); return 1; }
    if (conf_entropy_opts && conf_max_prob) { fprintf(stderr, "--confidence-alpha and --confidence-norm go with --confidence-method entropy or tsallis\n"); return 1; }
    if (second_pass < 0 || second_pass > 8) { fprintf(stderr, "--second-pass must be 1 .. 8 (got %d)\n", second_pass); return 1; }
    if (!second_pass && (sp_nbest || sp_symbols || history_frames != 2048)) { fprintf(stderr, "--nbest, --max-symbols and --history-frames go with --second-pass\n"); return 1; }
    if (chunk_ms < 10) { fprintf(stderr, "chunk_ms must be >= 10 (got %d)\n", chunk_ms); return 1; }
    fprintf(stderr, "Configuration:\n  Model:          %s\n  Audio:          %s\n  Chunk size:     %d ms\n  Right context:  %d\n\n",
            model_path, from_stdin ? "stdin" : audio_path, chunk_ms, right_context);

    if (second_pass && !diarize_gguf.empty()) { fprintf(stderr, "--second-pass does not go with --diarize\n"); return 1; }
    if (second_pass && (save_state || load_state)) { fprintf(stderr, "--second-pass does not go with --save-state / --load-state (the frame history does not travel)\n"); return 1; }
    if (preview && !diarize_gguf.empty()) { fprintf(stderr, "--preview does not go with --diarize\n"); return 1; }
    if ((save_state || load_state) && !diarize_gguf.empty()) { fprintf(stderr, "--save-state / --load-state do not go with --diarize\n"); return 1; }
    nemo_context *ctx = nemo_init_with_device(model_path, device, dtype, preview ? 2 : 1);      // a preview flushes a fork of the stream: one slot of headroom
    if (!ctx) { fprintf(stderr, "Failed to load ASR model\n"); return 1; }
    if (confidence && conf_max_prob && !nemo_set_token_logprobs(ctx, true)) { fprintf(stderr, "Failed to enable token log-probabilities\n"); nemo_free(ctx); return 1; }
    if (confidence && !conf_max_prob && !nemo_set_token_entropy(ctx, conf_alpha)) { fprintf(stderr, "Failed to enable token entropies (--confidence-alpha 0.05 .. 0.9, 1 or 1.1 .. 4)\n"); nemo_free(ctx); return 1; }
    if (alternatives && !nemo_set_token_alternatives(ctx, alternatives)) { fprintf(stderr, "Failed to enable %d token alternatives (K = 1 .. 8)\n", alternatives); nemo_free(ctx); return 1; }
    if (second_pass && !nemo_set_frame_history(ctx, history_frames)) { fprintf(stderr, "Failed to enable the frame history (--history-frames 64 .. 2048 in multiples of 64)\n"); nemo_free(ctx); return 1; }
    if (endpoints && !nemo_set_frame_blank_logprobs(ctx, true)) { fprintf(stderr, "Failed to enable per-frame blank log-probabilities\n"); nemo_free(ctx); return 1; }
    if (boost_file && !(nemo_set_phrase_boost(ctx, 4096) && nemo_load_boost_file(ctx, boost_file, boost_bonus) && (!second_pass || nemo_set_beam_boost(ctx, true)))) { fprintf(stderr, "Failed to load boost phrases from '%s'\n", boost_file); nemo_free(ctx); return 1; }
    if (lm_path && !(nemo_set_lm_fusion(ctx, true) && nemo_load_lm_arpa(ctx, lm_path, second_pass ? lm_weight : 0.0f, second_pass ? token_bonus : 0.0f) && nemo_set_greedy_lm_weights(ctx, lm_weight, token_bonus))) {
        fprintf(stderr, "Failed to load the language model from '%s'\n", lm_path);
        nemo_free(ctx);
        return 1;
    }
    if (pipeline && !nemo_set_pipeline(ctx, pipeline)) { fprintf(stderr, "Failed to enable pipelined steps\n"); nemo_free(ctx); return 1; }
    if (lang && !nemo_set_language(ctx, lang)) { fprintf(stderr, "Failed to set language '%s'\n", lang); nemo_free(ctx); return 1; }
    nemo_cache_config cfg = nemo_cache_config::default_config();
    cfg.att_right_context = right_context;
    nemo_stream_context *sctx = nullptr;
    if (load_state) {                                  // the stream of an earlier run: its right_context, format and endpoint detector come with it
        std::vector<uint8_t> blob;
        FILE *sf = fopen(load_state, "rb");
        if (!sf) { fprintf(stderr, "Failed to open the snapshot: %s\n", load_state); nemo_free(ctx); return 1; }
        uint8_t part[65536];
        for (size_t k; (k = fread(part, 1, sizeof(part), sf)) > 0;) blob.insert(blob.end(), part, part + k);
        fclose(sf);
        sctx = nemo_stream_restore(ctx, blob.data(), blob.size());
        if (!sctx) { fprintf(stderr, "Failed to restore the stream from '%s'\n", load_state); nemo_free(ctx); return 1; }
        if (positional >= 2 && right_context != sctx->config.att_right_context) fprintf(stderr, "note: right_context %d comes from the snapshot\n", sctx->config.att_right_context);
        right_context = sctx->config.att_right_context;
        cfg.att_right_context = right_context;
    } else sctx = nemo_stream_init(ctx, &cfg);
    if (!sctx) { fprintf(stderr, "Failed to create streaming context\n"); nemo_free(ctx); return 1; }

    if (endpoints && !load_state && !nemo_stream_set_endpointing(sctx, &ep_cfg)) { fprintf(stderr, "Failed to enable endpointing\n"); nemo_stream_free(sctx); nemo_free(ctx); return 1; }

    diarize_pipeline *dp = nullptr;
    if (!diarize_gguf.empty()) {                       // reference :146-170
        diarize_pipeline_cfg dcfg = diarize_pipeline_default_cfg();
        dcfg.diarize_gguf_path = diarize_gguf;
        dcfg.device = device;
        dcfg.dtype = dtype;
        dcfg.sub_shift_sec = sub_shift_sec;
        if (vad_onset >= 0.0f) dcfg.vad_post.onset = vad_onset;
        if (vad_offset >= 0.0f) dcfg.vad_post.offset = vad_offset;
        dcfg.cluster.oracle_num_speakers = num_speakers;
        dcfg.cluster.min_samples_for_nmesc = 4;
        dcfg.rttm_path = rttm_path;
        dcfg.speaker_text_path = speaker_text_path.empty() ? "-" : speaker_text_path;
        dp = diarize_pipeline_init(dcfg);
        if (!dp) { fprintf(stderr, "Failed to init diarization pipeline\n"); nemo_stream_free(sctx); nemo_free(ctx); return 1; }
    }
    FILE *json_file = json_path.empty() || json_path == "-" ? nullptr : fopen(json_path.c_str(), "w");
    std::string held;
    auto handle_text = [&](const std::string &text, size_t samples_so_far) {     // reference :196-224
        if (!text.empty() && (preview || second_pass)) held += text;       // --preview: the `~ ` lines come first, the transcript's line stays whole
        else if (!text.empty()) { fputs(text.c_str(), stdout); fflush(stdout); }
        if (!dp || text.empty()) return;
        diarize_pipeline_push_text(dp, text, (double)samples_so_far / 16000.0);
        if (!json_path.empty()) {
            const std::string j = diarize_pipeline_drain_json(dp);
            if (!j.empty()) fputs(j.c_str(), json_file ? json_file : stdout);
        }
    };
    // --second-pass: the N best of one utterance, frames [start, end) of the stream holding tokens [tok0, tok0 + n_tok) of its greedy decode
    size_t sp_events = 0, sp_tok0 = 0;
    auto second_pass_utterance = [&](int64_t start, int64_t end, size_t n_tok) {
        const std::vector<int> &all = nemo_stream_get_tokens(sctx);
        const size_t a = std::min(sp_tok0, all.size()), b = std::min(sp_tok0 + n_tok, all.size());
        sp_tok0 += n_tok;
        fprintf(stderr, "second pass: utterance %.2f .. %.2f s\n", (double)start * 0.08, (double)end * 0.08);
        int64_t kept_first = 0;
        int kept = 0;
        const bool have = nemo_stream_history_range(sctx, &kept_first, &kept);
        if (end - start > history_frames || !have || start < kept_first || end > kept_first + kept) {
            printf("second pass: the utterance's %lld frames are not all among the %d kept; greedy:%s\n", (long long)(end - start), history_frames,
                   tokens_to_text(std::vector<int>(all.begin() + (long)a, all.begin() + (long)b), ctx->vocab).c_str());
            fflush(stdout);
            return;
        }
        const std::vector<nemo_hypothesis> hyps = nemo_stream_second_pass_beam(sctx, start, (int)(end - start), second_pass, sp_nbest, sp_symbols);
        for (size_t r = 0; r < hyps.size(); r++) printf("%s\n", beam_hypothesis_line(r, hyps[r], ctx->vocab).c_str());
        fflush(stdout);
    };
    auto second_pass_new_endpoints = [&]() {
        const std::vector<nasr_endpoint::Event> &evs = nemo_stream_get_endpoints(sctx);
        for (; sp_events < evs.size(); sp_events++) second_pass_utterance(evs[sp_events].utt_start, evs[sp_events].frame + 1, (size_t)evs[sp_events].tokens);
    };
    std::vector<float> f32;
    FILE *in = from_stdin ? stdin : fopen(audio_path, "rb");
    if (!in) { fprintf(stderr, "Failed to open audio file: %s\n", audio_path); nemo_stream_free(sctx); nemo_free(ctx); return 1; }
    // a WAVE header names the format and is skipped; whatever was read past it is the first audio
    // (12 bytes tell: a live stream of raw audio is not made to wait for more than that before its first chunk)
    std::vector<uint8_t> pending(12);
    pending.resize(fread(pending.data(), 1, pending.size(), in));
    if (pending.size() == 12 && !memcmp(pending.data(), "RIFF", 4) && !memcmp(pending.data() + 8, "WAVE", 4)) {
        pending.resize(4096);
        pending.resize(12 + fread(pending.data() + 12, 1, pending.size() - 12, in));
    }
    size_t data_left = SIZE_MAX;                     // bytes of the data chunk still to come (raw audio: to the end of the file)
    for (;;) {
        wav_header::Info wi;
        char err[160];
        const int rc = wav_header::parse(pending.data(), pending.size(), &wi, err, sizeof(err));
        if (rc == wav_header::NOT_WAV) break;
        if (rc == wav_header::OK) {
            in_rate = wi.sample_rate; in_enc = wi.encoding; in_channels = wi.channels;
            if (wi.data_bytes != 0 && wi.data_bytes != 0xFFFFFFFFu) data_left = wi.data_bytes;
            pending.erase(pending.begin(), pending.begin() + (long)wi.data_offset);
            fprintf(stderr, "  WAV header:     %d Hz, %d channel(s), format tag %d at %d bits\n\n", wi.sample_rate, wi.channels, wi.format_tag, wi.bits);
            break;
        }
        // the data chunk may lie behind chunks longer than what has been read: read on (up to 1 MiB), unless the file has ended
        const size_t have = pending.size();
        if ((rc == wav_header::ERR_NO_DATA || rc == wav_header::ERR_NO_FMT || rc == wav_header::ERR_TRUNCATED) && have < (1u << 20)) {
            pending.resize(2 * have);
            pending.resize(have + fread(pending.data() + have, 1, have, in));
            if (pending.size() > have) continue;
        }
        fprintf(stderr, "%s\n", err);
        nemo_stream_free(sctx); nemo_free(ctx);
        return 1;
    }
    if (in_channel == -2) in_channel = in_channels > 1 ? -1 : 0;
    const bool own_format = !(in_rate == 16000 && in_enc == NASR_AUDIO_S16 && in_channels == 1 && in_channel == 0);
    if (load_state) {
        if (in_rate != sctx->audio_rate || in_enc != sctx->audio_encoding || in_channels != sctx->audio_channels || in_channel != sctx->audio_channel) {
            fprintf(stderr, "The snapshot's stream takes %d Hz, encoding %d, %d channel(s), channel %d: give the same --input-* flags\n", sctx->audio_rate, sctx->audio_encoding, sctx->audio_channels, sctx->audio_channel);
            nemo_stream_free(sctx); nemo_free(ctx);
            return 1;
        }
    } else if (own_format) {
        if (dp) { fprintf(stderr, "--diarize takes s16le 16 kHz mono audio\n"); nemo_stream_free(sctx); nemo_free(ctx); return 1; }
        if (!nemo_stream_set_audio_format(sctx, in_rate, in_enc, in_channels, in_channel)) { fprintf(stderr, "Unsupported input format\n"); nemo_stream_free(sctx); nemo_free(ctx); return 1; }
        fprintf(stderr, "  Input:          %d Hz, encoding %d, %d channel(s), channel %d (converted on the GPU)\n\n", in_rate, in_enc, in_channels, in_channel);
    }
    // like the reference, the read size is the model's chunk (chunk_ms is validated and printed only); in another format, the input frames of as much time
    const size_t frame_bytes = (size_t)in_channels * (in_enc == NASR_AUDIO_S16 ? 2 : in_enc == NASR_AUDIO_F32 ? 4 : 1);
    const size_t read_samples = (size_t)cfg.get_chunk_samples() + (size_t)(read_chunks - 1) * 1280u * (size_t)(1 + right_context);
    const size_t read_frames = (read_samples * (size_t)in_rate + 15999) / 16000;
    std::vector<uint8_t> raw(read_frames * frame_bytes + 8);
    uint8_t *buf = raw.data() + (8 - (uintptr_t)raw.data() % 8) % 8;            // aligned for s16 / f32 reads
    size_t total = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const size_t want = std::min(read_frames * frame_bytes, data_left);
        size_t have = std::min(want, pending.size());
        memcpy(buf, pending.data(), have);
        pending.erase(pending.begin(), pending.begin() + (long)have);
        if (have < want) have += fread(buf + have, 1, want - have, in);
        if (data_left != SIZE_MAX) data_left -= have;
        const size_t got = have / frame_bytes;                                   // a cut last frame is dropped
        if (got == 0) break;
        total += got;
        // handle_text's sample count feeds the diarization pipeline only, which runs on the default format: there frames are 16 kHz samples
        handle_text(own_format ? nemo_stream_process_audio(sctx, buf, (int)got) : nemo_stream_process_incremental(sctx, (const int16_t *)buf, (int)got), total);
        if (preview) { printf("~ %s\n", nemo_stream_preview(sctx).c_str()); fflush(stdout); }
        if (second_pass && endpoints) second_pass_new_endpoints();
        if (dp) {
            f32.resize(got);
            for (size_t k = 0; k < got; k++) f32[k] = (float)((const int16_t *)buf)[k] / 32768.0f;
            diarize_pipeline_push_audio(dp, f32.data(), got);
        }
        if (have < want || data_left == 0) break;
    }
    if (save_state) {                                  // no flush: the stream goes on in a later run
        std::vector<uint8_t> blob;
        FILE *sf = nemo_stream_save(sctx, blob) ? fopen(save_state, "wb") : nullptr;
        if (!sf || fwrite(blob.data(), 1, blob.size(), sf) != blob.size() || fclose(sf) != 0) {
            fprintf(stderr, "Failed to write the snapshot: %s\n", save_state);
            nemo_stream_free(sctx); nemo_free(ctx);
            return 1;
        }
        fprintf(stderr, "Wrote snapshot: %s (%zu bytes)\n", save_state, blob.size());
    } else handle_text(nemo_stream_finalize(sctx), total);
    if (second_pass && endpoints) {                    // the endpoints the tail produced, then the utterance still open
        second_pass_new_endpoints();
        if (sctx->ep_state.tokens > 0) second_pass_utterance(sctx->ep_state.utt_start, sctx->ep_frames, (size_t)sctx->ep_state.tokens);
    } else if (second_pass) {                          // without endpointing the whole stream is one utterance
        int64_t kept_first = 0;
        int kept = 0;
        if (nemo_stream_history_range(sctx, &kept_first, &kept)) second_pass_utterance(0, kept_first + kept, nemo_stream_get_tokens(sctx).size());
    }
    fputs(held.c_str(), stdout);
    printf("\n");
    if (!from_stdin) fclose(in);
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const double audio_s = (double)total / (double)in_rate;
    fprintf(stderr, "\nAudio duration:   %.2f s\nProcessing time:  %.3f s\nReal-time factor: %.4f (%.1fx real time)\nChunks: %d\n",
            audio_s, wall, audio_s > 0 ? wall / audio_s : 0.0, wall > 0 ? audio_s / wall : 0.0, sctx->total_chunks_processed);
    if (timestamps && !confidence) printf("%s\n", tokens_to_text(nemo_stream_get_timed_tokens(sctx), ctx->vocab, true).c_str());
    if (confidence) {
        // --confidence alone: exp(min ln P) as ever.  With a --confidence-* flag: the per-token confidences of the chosen measure, aggregated per word
        const std::vector<word_conf::Word> ws =
            !conf_opts ? word_conf::words(nemo_stream_get_tokens(sctx), nemo_stream_get_token_logprobs(sctx), ctx->vocab)
                       : token_conf::words(nemo_stream_get_tokens(sctx),
                                           conf_max_prob ? token_conf::max_prob_confidences(nemo_stream_get_token_logprobs(sctx))
                                                         : token_conf::confidences(nemo_stream_get_token_entropies(sctx), (double)ctx->token_entropy_milli / 1000.0, conf_method, conf_norm),
                                           ctx->vocab, conf_agg);
        std::vector<std::string> stamps;
        if (timestamps) {
            const std::vector<timed_token> tt = nemo_stream_get_timed_tokens(sctx);
            for (const word_conf::Word &w : ws) {
                char stamp[32];
                snprintf(stamp, sizeof(stamp), "{%.2f}", (size_t)w.first_token < tt.size() ? tt[(size_t)w.first_token].to_seconds() : -1.0f);
                stamps.push_back(stamp);
            }
        }
        printf("%s\n", word_conf::annotate(ws, timestamps ? &stamps : nullptr).c_str());
    }
    if (alternatives) {
        const nemo_token_alternatives alt = nemo_stream_get_token_alternatives(sctx);
        for (size_t i = 0; i < alt.n_tokens; i++) {
            printf("alt %zu", i);
            for (int j = 0; j < alt.k; j++) printf(" %d:%.4f", alt.ids[i * alt.k + j], std::exp((double)alt.logprobs[i * alt.k + j]));
            printf("\n");
        }
    }
    if (endpoints) {
        const std::vector<nasr_endpoint::Event> evs = nemo_stream_get_endpoints(sctx);
        const std::vector<int> &all = nemo_stream_get_tokens(sctx);
        size_t t0i = 0;
        auto line = [&](int64_t start, int64_t end, int rule, size_t n_tok) {
            const size_t a = std::min(t0i, all.size()), b = std::min(t0i + n_tok, all.size());
            printf("endpoint %.2f %.2f rule %d tokens %zu:%s\n", (double)start * 0.08, (double)end * 0.08, rule, n_tok,
                   tokens_to_text(std::vector<int>(all.begin() + (long)a, all.begin() + (long)b), ctx->vocab).c_str());
            t0i += n_tok;
        };
        for (const nasr_endpoint::Event &ev : evs) line(ev.utt_start, ev.frame + 1, ev.rule, (size_t)ev.tokens);
        if (sctx->ep_state.tokens > 0) line(sctx->ep_state.utt_start, sctx->ep_frames, 0, (size_t)sctx->ep_state.tokens);
    }
    if (print_tokens) {
        printf("TOKENS:");
        for (int t : nemo_stream_get_tokens(sctx)) printf(" %d", t);
        printf("\n");
    }
    if (dp) {                                          // reference :268-292
        fprintf(stderr, "\nFinalizing diarization (%zu sub-segments, %zu words)...\n", diarize_pipeline_n_embeddings(dp), diarize_pipeline_n_words(dp));
        const std::string spk_text = diarize_pipeline_finalize(dp);
        if (!json_path.empty()) {
            const std::string j = diarize_pipeline_drain_json(dp);
            if (!j.empty()) fputs(j.c_str(), json_file ? json_file : stdout);
        }
        if (speaker_text_path.empty() || speaker_text_path == "-") {
            fprintf(stderr, "\n=== Speaker-tagged transcript ===\n");
            fputs(spk_text.c_str(), stdout);
        }
        if (!rttm_path.empty()) fprintf(stderr, "Wrote RTTM: %s\n", rttm_path.c_str());
        diarize_pipeline_free(dp);
    }
    if (json_file) fclose(json_file);
    nemo_stream_free(sctx);
    nemo_free(ctx);
    return 0;
}
