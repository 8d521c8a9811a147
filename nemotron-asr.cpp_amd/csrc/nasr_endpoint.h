// nasr_endpoint.h -- the endpoint detector over the per-frame blank log-probabilities (engine option "frame_blank_logprobs"), pure code without
// HIP so that the CPU suite compiles it with g++ under sanitizers (tests/test_endpoint_math.py), like nasr_boost.h.  It is stated once, here;
// host/nemo_amd.cpp and the CLI run it over the values the engine hands out.
//
// Frames are fed in order, one call per encoder frame (80 ms): its absolute number, ln P(blank) at the last joint evaluation on it and the
// number of tokens the decode emitted on it.  A frame is SILENT iff it emitted no token and lp_blank >= min_blank_logprob.  advance():
//   1. trailing = silent ? trailing + 1 : 0
//   2. tokens  += tokens_on_frame
//   3. rule 2 (end of speech)     fires if tokens > 0 and trailing >= silence_frames_after_speech
//   4. else rule 1 (idle)         fires if tokens == 0 and trailing >= silence_frames_idle
//   5. else rule 3 (too long)     fires if frame - utt_start + 1 >= max_utterance_frames
//   6. a limit <= 0 disables its rule
//   7. on firing: *out is filled, utt_start = frame + 1, tokens = trailing = 0, and advance returns true
// The defaults follow the convention of the Kaldi / sherpa-onnx endpoint rules at this model's 80 ms frames: every frame without a token counts
// as silence (threshold -inf), 2.4 s of silence with nothing decoded, 1.2 s of silence after something decoded, 20 s at the most.  They are
// user parameters.
#pragma once
#include <math.h>
#include <stdint.h>

namespace nasr_endpoint {

constexpr int RULE_IDLE = 1, RULE_AFTER_SPEECH = 2, RULE_MAX_LENGTH = 3;

struct Config {
    float min_blank_logprob = -INFINITY;       // a token-less frame is silent from this ln P(blank) upwards
    int silence_frames_idle = 30;              // rule 1: 2.4 s
    int silence_frames_after_speech = 15;      // rule 2: 1.2 s
    int max_utterance_frames = 250;            // rule 3: 20 s
};
struct State {
    int64_t utt_start = 0;                     // first frame of the utterance in progress
    int32_t tokens = 0, trailing = 0;          // tokens of the utterance so far; silent frames at its end
};
struct Event {
    int64_t frame = 0, utt_start = 0;          // the utterance is frames [utt_start, frame]
    int32_t rule = 0, tokens = 0;
};

inline bool advance(State &st, const Config &cfg, int64_t frame, float lp_blank, int tokens_on_frame, Event *out) {
    const bool silent = tokens_on_frame == 0 && lp_blank >= cfg.min_blank_logprob;
    st.trailing = silent ? st.trailing + 1 : 0;
    st.tokens += tokens_on_frame;
    int rule = 0;
    if (cfg.silence_frames_after_speech > 0 && st.tokens > 0 && st.trailing >= cfg.silence_frames_after_speech) rule = RULE_AFTER_SPEECH;
    else if (cfg.silence_frames_idle > 0 && st.tokens == 0 && st.trailing >= cfg.silence_frames_idle) rule = RULE_IDLE;
    else if (cfg.max_utterance_frames > 0 && frame - st.utt_start + 1 >= cfg.max_utterance_frames) rule = RULE_MAX_LENGTH;
    if (!rule) return false;
    if (out) { out->frame = frame; out->utt_start = st.utt_start; out->rule = rule; out->tokens = st.tokens; }
    st.utt_start = frame + 1;
    st.tokens = 0;
    st.trailing = 0;
    return true;
}

}  // namespace nasr_endpoint
