// nasr_constants.h -- the model constants and the per-step descriptors, without HIP: what the pure host headers (nasr_step_plan.h) share
// with the engine.  nasr_internal.h includes it.
#pragma once
#include <stdint.h>

namespace nasr {

// ---- model constants this build is specialised for (nemotron-speech-streaming-0.6B and
// its multilingual sibling: reference src/nemo-ggml.h:37-55). n_layers / kernel_size /
// num_prompts stay runtime. -----------------------------------------------------------
constexpr int D      = 1024;
constexpr int NH     = 8;
constexpr int DH     = 128;
constexpr int FF     = 4096;
constexpr int NMEL   = 128;
constexpr int NBINS  = 257;
constexpr int NFFT   = 512;
constexpr int HOP    = 160;
constexpr int WIN    = 400;
constexpr int LCTX   = 70;    // att_left_context
constexpr int TMAX   = 14;    // 1 + max right context (13)
constexpr int MAXNEW = 256;   // encoder frames one stream may complete in ONE launch sequence (multi-chunk steps)
constexpr int KVC    = LCTX + MAXNEW;   // K/V ring capacity: the 70-row window + the rows a launch appends
constexpr int SUBC   = 256;   // subsampling channels
constexpr int SUBF   = 17;    // subsampled freq bins
constexpr int SUBFLAT = SUBC * SUBF;  // 4352
constexpr int VOCAB  = 1025;
constexpr int BLANK  = 1024;
constexpr int HID    = 640;
constexpr int JNT    = 640;
constexpr int PRE_CACHE = 9;
constexpr int DROP_EXTRA = 2;
constexpr int MAX_SYMBOLS = 10;
constexpr int MEL_RING = 4096;        // mel ring frames per stream (power of two, > 9 + 8 * MAXNEW + one chunk)
constexpr int MAX_PUSH = 1280 * MAXNEW;   // samples per internal sub-push (MAXNEW encoder frames)
constexpr int ABUF_CAP = MAX_PUSH + NFFT + 64;
constexpr int MAX_KS   = 32;          // max depthwise kernel size supported
constexpr int FUSE_MAX_M = 2;         // rows up to which attention / depthwise conv are fused into the following GEMM's prologue
constexpr int TOK_CAP  = 4096;        // per-stream device token ring between collects
constexpr int FRAME_CAP = 4096;       // per-stream device ring of per-frame blank log-probabilities (engine option "frame_blank_logprobs"): 5.5 minutes of 80 ms frames

// ---- per-step descriptors (uploaded by the host for every launch sequence) -----------
struct RowDesc {          // one per batch row (= stream taking part in this chunk step)
    int slot;             // state-pool slot
    int valid_len;        // cache_valid_len BEFORE this chunk (src/nemo-stream.cpp:1037)
    int kv_head;          // ring index of logical key 0
    int mel_start;        // mel-ring index of the first frame of the chunk
    int cc_par;           // conv-cache buffer to read (the other one is written)
    int n_dec;            // encoder frames to decode (T, or n_valid on the tail flush)
    int prompt;           // language prompt index (multilingual) or -1
    int pad;
};

struct PcmDesc {          // one per stream receiving samples in a sub-push
    const int16_t *pcm;   // device pointer to the samples of this sub-push
    int slot;
    int n;                // samples in this sub-push
    int cnt;              // samples already in the audio buffer
    int par;              // audio buffer parity holding them
    int n_frames;         // frames this sub-push completes
    int mel_wpos;         // mel-ring write index of the first new frame
    int consumed;         // samples consumed = n_frames * HOP
    int pad;
};

}  // namespace nasr
