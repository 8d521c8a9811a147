// nasr_offline_plan.h -- the plan of one offline call (nasr_engine_transcribe_mel), pure host code without HIP so that it can be
// compiled and tested on a CPU under sanitizers (tests/test_offline_abi.py), like server_protocol.h: pick_call.
//   mel frames of an utterance of n samples: 1 + (256 + n - 512) / 160 (none below 256 samples)
//   encoder frames of an utterance: T = s(s(s(n_mel))), s(n) = n / 2 + 1 -- ConvSubsampling over the whole mel, three stride-2
//   3x3 convs padded 2 before / 1 after (reference src/nemo-ggml.cpp:905-913, :969-994); n_mel = 0 gives T = 0 (nothing runs)
//   limit: T <= 2048 = max_pos_len (src/nemo-ggml.cpp:229-233)
//   sub-batches: consecutive utterances, at most `row_budget` encoder rows and `max_utts` utterances each; an utterance whose T
//   alone exceeds the budget is a sub-batch of its own
#pragma once
#include <stdint.h>
#include <vector>
#include "nasr_step_plan.h"

namespace nasr_plan {

constexpr int OFFLINE_MAX_FRAMES = 2048;
constexpr int OFFLINE_MAX_UTTS = 256;      // utterances per sub-batch (decoder slots of the offline path)

inline int sub_len(int n) { return n / 2 + 1; }
// log-mel frames of a whole utterance of n samples = what the reference preprocessor returns for it (src/preprocessor.cpp:320-328:
// 256 zero samples in front, 512-sample frames every 160 samples)
inline int mel_frames(int64_t n_samples) { return nasr_step::push_frames(256, n_samples > 0 ? n_samples : 0); }
// most samples whose encoder frames stay within the limit
inline int64_t max_samples() { return (int64_t)(16377 - 1) * 160 + 512 - 256 + 159; }
inline int enc_frames(int n_mel) { return n_mel <= 0 ? 0 : sub_len(sub_len(sub_len(n_mel))); }
// rows of the two intermediate images of the subsampling (conv0 output is never stored): H1, H2
inline int sub_h1(int n_mel) { return n_mel <= 0 ? 0 : sub_len(n_mel); }
inline int sub_h2(int n_mel) { return n_mel <= 0 ? 0 : sub_len(sub_len(n_mel)); }

struct Batch { int first, count, rows; };

// Returns 0, or -1 with *bad = the first utterance over the limit (or with a negative frame count).  T[b] and the sub-batches
// are filled on success.
// frames_given: n_mel[b] is already the encoder frame count of utterance b (a window of a stream's frame history), not its mel frames
inline int plan_offline(const int32_t *n_mel, int B, int row_budget, int max_utts, std::vector<int> &T, std::vector<Batch> &batches, int *bad,
                        bool frames_given = false) {
    T.assign(B > 0 ? B : 0, 0);
    batches.clear();
    if (bad) *bad = -1;
    if (B < 0 || row_budget < 1 || max_utts < 1) return -1;
    for (int b = 0; b < B; b++) {
        if (n_mel[b] < 0) { if (bad) *bad = b; return -1; }
        T[b] = frames_given ? n_mel[b] : enc_frames(n_mel[b]);
        if (T[b] > OFFLINE_MAX_FRAMES) { if (bad) *bad = b; return -1; }
    }
    int b = 0;
    while (b < B) {
        Batch bt{b, 0, 0};
        while (b < B && bt.count < max_utts && (bt.count == 0 || bt.rows + T[b] <= row_budget)) {
            bt.rows += T[b];
            bt.count++;
            b++;
            if (bt.rows > row_budget) break;          // a lone utterance longer than the budget
        }
        batches.push_back(bt);
    }
    return 0;
}

}  // namespace nasr_plan
