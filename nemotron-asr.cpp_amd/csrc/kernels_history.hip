// kernels_history.hip -- engine option "frame_history" (nasr_history.h): the append of a step's encoder-projection rows into their
// slots' rings, and the gather of frame windows out of the rings into the packed rows of an offline call.  Both are plain copies of 2 560-byte
// rows as 160 vectors of 16 bytes.  The append moves one row per workgroup: measured against four rows per workgroup (HistAppendParams::wg_rows
// = 4; engine option "history_append_rows", measurement only) it takes 6.4 against 7.2 us at 896 rows and the same 6.2 us at one row
// (profiles/frame_history.md).  A workgroup of the gather moves HIST_WG_ROWS rows (640 vectors on 256 threads).
#include "nasr_internal.h"

namespace nasr {

constexpr int HIST_WG_ROWS = 4;
constexpr int HIST_WG_VECS = HIST_WG_ROWS * nasr_hist::ROW_VECS;

// Row (b, t) of the step -- batch row b, frame t of p.T, the layout the joint reads (encproj[(b * T + t)]) -- goes to row (frame0 + t) % N of
// its slot's ring.  frame0 is what k_dec_begin has just put in force for this step, n_dec the frames the step decodes (n_valid on the
// finalize tail): the rows past it are padding and are not appended
template <int WG_ROWS>
__global__ __launch_bounds__(256) void k_history_append(HistAppendParams p) {
    const int rows = p.B * p.T;
    for (int v = threadIdx.x; v < WG_ROWS * nasr_hist::ROW_VECS; v += 256) {
        const int m = blockIdx.x * WG_ROWS + v / nasr_hist::ROW_VECS, c = v % nasr_hist::ROW_VECS;
        if (m >= rows) break;
        const int b = m / p.T, t = m % p.T;
        const RowDesc rd = p.rows[b];
        if (t >= rd.n_dec || rd.slot < 0 || rd.slot >= p.slots) continue;
        const int64_t frame = (int64_t)p.ctrl[rd.slot].frame0 + t;
        if (frame < 0) continue;
        const float4 *src = (const float4 *)(p.encproj + (size_t)m * nasr_hist::ROW_FLOATS);
        float4 *dst = (float4 *)(p.ring + ((size_t)rd.slot * p.N + nasr_hist::ring_row(frame, p.N)) * nasr_hist::ROW_FLOATS);
        dst[c] = src[c];
    }
}
void launch_history_append(const HistAppendParams &p, hipStream_t st) {
    const int rows = p.B * p.T;
    if (rows <= 0) return;
    if (p.wg_rows == 4) hipLaunchKernelGGL(k_history_append<4>, dim3((rows + 3) / 4), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_history_append<1>, dim3(rows), dim3(256), 0, st, p);
}

// Window w (blockIdx.y): frame j of it, ring row run_row(runs, j) of its slot, becomes packed row out_row + j of out.  The host has checked the
// window against the stream's retained range (nasr_hist::window_kept) and the slot against the pool
__global__ __launch_bounds__(256) void k_history_gather(const HistWindow *win, const float *ring, int N, float *out) {
    const HistWindow w = win[blockIdx.y];
    const nasr_hist::Runs runs = nasr_hist::ring_runs(w.first, w.count, N);
    for (int v = threadIdx.x; v < HIST_WG_VECS; v += 256) {
        const int j = blockIdx.x * HIST_WG_ROWS + v / nasr_hist::ROW_VECS, c = v % nasr_hist::ROW_VECS;
        if (j >= w.count) break;
        const float4 *src = (const float4 *)(ring + ((size_t)w.slot * N + nasr_hist::run_row(runs, j)) * nasr_hist::ROW_FLOATS);
        float4 *dst = (float4 *)(out + ((size_t)w.out_row + j) * nasr_hist::ROW_FLOATS);
        dst[c] = src[c];
    }
}
void launch_history_gather(const HistWindow *win, int n, int max_count, const float *ring, int N, float *out, hipStream_t st) {
    if (n > 0 && max_count > 0) hipLaunchKernelGGL(k_history_gather, dim3((max_count + HIST_WG_ROWS - 1) / HIST_WG_ROWS, n), dim3(256), 0, st, win, ring, N, out);
}

}  // namespace nasr
