// nasr_history.h -- the per-stream ring of encoder-projection rows (engine option "frame_history" = N) and its arithmetic: which
// frames a stream keeps, whether a window of frames is kept, and where a window lies in the ring.  The ring is [slot][N][640] f32; row f % N
// of a slot holds absolute encoder frame f, counted from create / reset (the numbering of nasr_stream_get_token_frames).  It is never
// cleared: every read goes through window_kept, so what a recycled slot or an earlier life of the stream left in it is never visible.
// Pure host + device code without HIP calls, compiled and tested on a CPU under sanitizers (tests/test_history_math.py) like
// nasr_fork_plan.h and nasr_offline_plan.h; the engine's read-outs and k_history_gather (kernels_history.hip) both use these functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NASR_HIST_HD __host__ __device__ inline
#else
#define NASR_HIST_HD inline
#endif

namespace nasr_hist {

constexpr int ROW_FLOATS = 640;                    // one row of the joint's encoder projection (nasr::JNT)
constexpr int ROW_BYTES = ROW_FLOATS * 4;          // 2 560: what a kept frame costs
constexpr int ROW_VECS = ROW_BYTES / 16;           // 160 vectors of 16 bytes: how both kernels move a row
constexpr int MIN_FRAMES = 64, MAX_FRAMES = 2048;  // N of the option; 2048 = the longest window an offline mode takes (NASR_OFFLINE_MAX_FRAMES)

// the option's values: 0 (off), or 64 .. 2048 in multiples of 64
NASR_HIST_HD bool valid_frames(int n) { return n == 0 || (n >= MIN_FRAMES && n <= MAX_FRAMES && n % MIN_FRAMES == 0); }

// bytes of the rings of an engine: max_streams x N x 2 560 (5.2 MB per slot at N = 2048)
NASR_HIST_HD int64_t ring_bytes(int max_streams, int N) { return (int64_t)max_streams * N * ROW_BYTES; }

// frames [first, first + count) of a stream
struct Range { int64_t first; int32_t count; };

// THE retained range: a stream that has decoded `done` frames since create / reset and whose history starts at valid_from (0 after create
// and both reset modes, `done` of the source after a fork or a restore) keeps [max(valid_from, done - N), done)
NASR_HIST_HD Range retained(int64_t valid_from, int64_t done, int N) {
    int64_t first = done - N;
    if (first < valid_from) first = valid_from;
    if (first > done) first = done;                // a valid_from beyond done (never produced by the engine) keeps nothing
    return Range{first, (int32_t)(done - first)};
}

// THE window check: every frame of [first, first + count) is kept.  A window without a frame names no row and is kept wherever it starts
NASR_HIST_HD bool window_kept(Range kept, int64_t first, int32_t count) {
    if (first < 0 || count < 0) return false;
    if (count == 0) return true;
    return first >= kept.first && first + count <= kept.first + kept.count;
}

// THE ring position of a window of at most N frames: rows [row0, row0 + n0) hold its first n0 frames, rows [0, n1) the rest (n1 = 0 unless
// the window crosses the wrap)
struct Runs { int32_t row0, n0, n1; };
NASR_HIST_HD Runs ring_runs(int64_t first, int32_t count, int N) {
    const int32_t row0 = (int32_t)(first % N);
    const int32_t n0 = count < N - row0 ? count : N - row0;
    return Runs{row0, n0, count - n0};
}
// ... and of its frame j (0 <= j < n0 + n1)
NASR_HIST_HD int32_t run_row(Runs r, int32_t j) { return j < r.n0 ? r.row0 + j : j - r.n0; }

// where the append puts absolute frame f
NASR_HIST_HD int32_t ring_row(int64_t frame, int N) { return (int32_t)(frame % N); }

}  // namespace nasr_hist
