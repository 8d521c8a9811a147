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

}  // namespace nasr_step
