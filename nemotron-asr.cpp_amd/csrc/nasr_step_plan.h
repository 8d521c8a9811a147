// nasr_step_plan.h -- the host arithmetic of a push: frames, chunks, graph-step eligibility, the cut of a long push and the counting fields of
// a PcmDesc.  Pure host code without HIP (only nasr_constants.h), compiled and tested on a CPU under sanitizers (tests/test_step_plan.py),
// like nasr_gemm_plan.h and nasr_offline_plan.h.
#pragma once
#include "nasr_constants.h"

namespace nasr_step {
using namespace nasr;

// log-mel frames a push of n samples completes when cnt samples wait in the audio buffer (a fresh stream: 256 zeros): 512-sample frames
// every 160 samples (src/preprocessor.cpp:320-328)
inline int push_frames(int64_t cnt, int64_t n) {
    const int64_t avail = cnt + n;
    return avail < NFFT ? 0 : (int)((avail - NFFT + HOP) / HOP);
}
inline int max_frames_per_push(int TS) { return 8 * TS + 16; }  // TS = frames of encoder output the push completes (+ what a first push leaves over)

// chunks of T encoder frames that mel_count buffered mel frames complete
inline int chunks_completed(int mel_count, int T) {
    const int chunk_mel = PRE_CACHE + 8 * T;
    return mel_count < chunk_mel ? 0 : (mel_count - chunk_mel) / (8 * T) + 1;
}

// The G of a graph step: the chunks the push of n[b] samples completes on EVERY stream b, or 0 for "take the eager path" (a push of no or
// too many samples, a stream that completes no chunk or another number than the others, more frames than the captured front end takes).
// G consecutive chunks of a stream are one launch sequence (same results: a chunk's layer-l inputs do not depend on the previous chunk's
// layer-l outputs, only on its K/V and conv state); that needs the option and the new rows to fit in the K/V ring next to the 70-row window.
inline int graph_step_chunks(const int *abuf_cnt, const int *mel_count, const int32_t *n, int B, int T, int w_rows, bool multichunk) {
    int G = -1;
    for (int b = 0; b < B; b++) {
        if (n[b] <= 0 || n[b] > MAX_PUSH) return 0;
        const int nf = push_frames(abuf_cnt[b], n[b]);
        const int g = chunks_completed(mel_count[b] + nf, T);
        if (g == 0) return 0;
        if (G < 0) G = g;
        if (g != G) return 0;
        if (nf > max_frames_per_push(T * G)) return 0;
    }
    if (G > 1 && (!multichunk || B * G * T > w_rows || G * T > MAXNEW)) return 0;
    return G < 0 ? 0 : G;
}

// A push longer than one launch sequence can take (MAXNEW encoder frames per stream, w_rows rows in all) is cut into pieces of whole
// chunks: the samples of one piece
inline int64_t piece_samples(int T, int B, int w_rows) {
    int gcap = MAXNEW / T < w_rows / (B * T) ? MAXNEW / T : w_rows / (B * T);
    if (gcap < 1) gcap = 1;
    return (int64_t)gcap * 8 * T * HOP;
}

// the counting fields of d for a push of n samples onto a stream whose audio buffer holds cnt samples in parity par and whose mel ring
// window is (mel_start, mel_count); pcm and slot are the caller's
inline void fill_pcm_counts(PcmDesc &d, int n, int cnt, int par, int mel_start, int mel_count) {
    d.n = n; d.cnt = cnt; d.par = par;
    d.n_frames = push_frames(cnt, n);
    d.mel_wpos = (mel_start + mel_count) & (MEL_RING - 1);
    d.consumed = d.n_frames * HOP;
}
// ... and the stream's counts once that push has been queued
inline void apply_pcm_counts(const PcmDesc &d, int &abuf_cnt, int &abuf_par, int &mel_count) {
    abuf_cnt = d.cnt + d.n - d.consumed;
    if (d.n_frames > 0) abuf_par ^= 1;
    mel_count += d.n_frames;
}

// ---- the fused family, its decode-graph budget and its lane cut ---------------------------------------------------------------------------
// Steps of up to FUSED_ROWS rows on a bf16 engine run the 8-launch fused layer (run_layers_fused), every other step the unfused layers
// (enqueue_layers).  The two forms cut a pipelined step into lane pieces differently, so the family is part of a step's cut identity.
constexpr int FUSED_ROWS = 4;
inline bool fused_family(bool bf16, bool opt_fused, bool debug, long rows) { return bf16 && opt_fused && !debug && rows >= 1 && rows <= FUSED_ROWS; }

// iterations enqueued before the host looks at n_active: (symbols of the busiest stream) + 1 are needed; a shortfall
// costs one host round trip and a further round of iterations
inline int blind_iterations(int frames) {
    if (frames <= 1) return 2;                  // one emission + the closing blank; a spare iteration would cost 1 % of the step
    return frames / 2 + 4 < 16 ? frames / 2 + 4 : 16;   // an idle iteration (~10 us) is far cheaper than a host round trip
}

// Decode iterations the decode graph of a pipelined step carries.  rows: the rows of a fused-family step (B T G), 0 for a step of any other
// form; cap: engine option "decode_graph_iterations", 0 = auto.  An explicit cap gives one frame up to its worst case (MAX_SYMBOLS + the
// closing blank), never less than the synchronous step graph carries.  Auto is a cap of 12, except for the one-frame step of the fused
// family: its decode graph runs behind the last encoder piece on a lane the host waits for in every call, where five launches per idle
// iteration are a dependent chain, so it carries 3 (a frame of two symbols + the closing blank; more symbols: finish_step_decode's fallback).
constexpr int DECODE_GRAPH_CAP = 12, SMALL_STEP_DECODE_ITERS = 3;
inline int pipe_decode_iterations(int rows, int frames, int cap) {
    if (cap <= 0 && frames == 1 && rows >= 1 && rows <= FUSED_ROWS) return SMALL_STEP_DECODE_ITERS;
    if (cap <= 0) cap = DECODE_GRAPH_CAP;
    const int worst = frames * MAX_SYMBOLS + 1, blind = blind_iterations(frames);
    const int want = worst < cap ? worst : cap;
    return blind > want ? blind : want;
}

// Launch index (of the 8 L launches of the L fused layers) at which lane piece k of E begins; piece E - 1 ends at 8 L.  The first piece also
// carries the front end (about 8 launches' worth of time), the last one the tail and the decode graph.  cut4: the three indices of the
// four-piece cut of a 24-layer model (engine option "fused_cuts"), nullptr = FUSED_CUT4; other depths scale them.
// Four pieces, batch 1, R = 0, 3-iteration decode graph, ms per step (median of 5 regions of 200 steps, spread 0.1-0.3 %; two machines, the
// parent commit on the same machine 0.4247 / 0.4222; profiles/small_step_decode.md):
//   48 | 104 | 162  0.4121 (the cut before: within two launches of the unfused path's layer bounds)     48 | 104 | 164  0.4131
//   46 |  98 | 150  0.4065 / 0.4039     46 | 96 | 150  - / 0.4024     46 | 98 | 154  - / 0.4036     44 | 98 | 150  - / 0.4045
//   46 | 102 | 154  - / 0.4048     46 | 100 | 150  - / 0.4059     46 | 98 | 152  - / 0.4060     46 | 100 | 152  - / 0.4061     46 | 100 | 154  0.4078 / -
//   48 |  98 | 150  - / 0.4135     48 | 100 | 150  - / 0.4133     48 | 100 | 148  0.4147 / -     48 | 100 | 152  0.4153 / -     46 | 96 | 148  0.4154 / -
//   44 |  96 | 148  0.4160 / -     48 | 102 | 156  0.4169 / -     46 | 98 | 148  - / 0.4179     50 | 104 | 156  0.4230 / -     46 | 98 | 146  0.4281 / -
//   44 |  94 | 146  0.4282 / -
// A plateau of 0.402-0.406 around 46 + 52 + 52 + 42 (a first piece of 48 or a last one of 44 and more leave it); with the decode
// iterations taken out altogether ("ablate" = 8) the same cut measures 0.4044: the decode no longer binds the step.
constexpr int FUSED_CUT4[3] = {46, 98, 150};
inline int fused_cut(int L, int E, int k, const int *cut4 = nullptr) {
    if (k <= 0) return 0;
    if (k >= E) return 8 * L;
    if (E == 4 && L >= 8) return (cut4 ? cut4 : FUSED_CUT4)[k - 1] * L / 24;
    if (E == 3 && L >= 6) return (k == 1 ? 57 : 126) * L / 24;
    if (E == 2 && L >= 8) return 8 * (L / 2 - 1);
    return 8 * L * k / E;
}
// "fused_cuts" packs the three indices in 10 bits each (lowest first); valid when they cut 8 L launches into four non-empty pieces
inline void unpack_cut4(int packed, int *cut4) { for (int k = 0; k < 3; k++) cut4[k] = (packed >> (10 * k)) & 1023; }
inline bool valid_cut4(const int *cut4, int L) {
    int prev = 0;
    for (int k = 0; k < 3; k++) {
        const int b = cut4[k] * L / 24;
        if (b <= prev) return false;
        prev = b;
    }
    return prev < 8 * L;
}

// ---- the read-out rings (token frames, log-probabilities, alternatives, per-frame blank): item i of the `have` the device has produced
// lives at i & (cap - 1), so the last `cap` are there.  Of the items first .. first + count - 1 (first, count >= 0: the getters refuse
// negatives) the caller gets those that exist: their number, or RING_TOO_OLD when there are some but the first of them has been overwritten
constexpr int RING_TOO_OLD = -1;
inline int ring_window(int64_t first, int count, int64_t have, int cap) {
    if (first >= have || count <= 0) return 0;
    if (count > have - first) count = (int)(have - first);
    return have - first > cap ? RING_TOO_OLD : count;
}

}  // namespace nasr_step
