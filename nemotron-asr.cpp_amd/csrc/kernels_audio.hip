// kernels_audio.hip -- device-side audio input conversion: any supported rate / encoding / channel layout -> the 16 kHz s16 mono that
// k_preemph (kernels_front.hip) reads.  The arithmetic is nasr_resample.h's, shared with the host: the same functions, the same order,
// __fmul_rn / __fadd_rn (this file is also compiled without FMA contraction), so a launch gives the bits of nasr_rs::HostStream.
//
// ONE launch for all streams of a call: grid = (blocks of 256 outputs + 1, streams).  A workgroup decodes (and down-mixes) the input
// frames its 256 outputs read into LDS -- at most nasr_rs::SPAN_CAP floats: frames from before the push come from the stream's history,
// frames before the stream's start or past its end are zeros -- and runs the tap loop, one output per thread.  The coefficient table of
// the L <= 2 rates (8 / 24 / 32 / 48 kHz: <= 193 floats) is copied into LDS by every workgroup; the larger tables stay in global memory:
// at one loop trip the lanes of a wave read within one window of L floats (nasr_resample.h: the linear table is the [tap][phase] layout),
// and all workgroups of all streams at a rate share it (113 KB at 44.1 kHz: L2-resident).  LDS holds 4 KB of input + 1 KB of table, so
// occupancy is bounded by waves, not by LDS.
// The last block column writes every stream's next history (the last hist decoded input frames) into the OTHER parity of its history
// buffer, as k_abuf_shift does for the audio buffer: nothing in this launch reads what it writes.
#include "nasr_internal.h"

namespace nasr {

__global__ __launch_bounds__(nasr_rs::BLOCK) void k_audio_convert(const AudioDesc *descs) {
    const AudioDesc d = descs[blockIdx.y];
    __shared__ float xs[nasr_rs::SPAN_CAP];
    nasr_rs::Plan pl;
    pl.fin = 0; pl.L = d.L; pl.M = d.M; pl.half = d.half; pl.hist = 2 * d.half / d.L + 1;
    nasr_rs::Source src;
    src.in = d.in; src.hist = d.hist ? d.hist + d.par * nasr_rs::HIST_MAX : nullptr;
    src.n_before = d.n_before; src.n_push = d.n_push; src.enc = d.enc; src.channels = d.channels; src.channel = d.channel; src.hist_len = pl.hist;
    if (blockIdx.x == gridDim.x - 1) {           // the history the next launch finds
        if (!d.hist || d.n_push <= 0) return;
        float *next = d.hist + (d.par ^ 1) * nasr_rs::HIST_MAX;
        for (int i = threadIdx.x; i < pl.hist && i < nasr_rs::HIST_MAX; i += nasr_rs::BLOCK) next[i] = src.hist_next(i);
        return;
    }
    const long long o0 = (long long)blockIdx.x * nasr_rs::BLOCK;
    if (o0 >= d.n_out) return;
    const int cnt = (int)(d.n_out - o0 < nasr_rs::BLOCK ? d.n_out - o0 : nasr_rs::BLOCK);
    const long long n0 = d.out_first + o0;
    const long long k_lo = nasr_rs::k_first(pl, n0), span = nasr_rs::k_last(pl, n0 + cnt - 1) - k_lo + 1;
    if (span > nasr_rs::SPAN_CAP) return;        // never for a plan of nasr_rs::make_plan (the host checks block_span); keeps LDS in bounds
    for (int i = threadIdx.x; i < (int)span; i += nasr_rs::BLOCK) xs[i] = src.at(k_lo + i);
    __syncthreads();
    auto x_at = [&](long long k0, int i) { return xs[(int)(k0 - k_lo) + i]; };
    if (d.lds_table) {                           // engine option "audio_lds_table" (default on; same bits): the tables of L <= 2 (<= 193 floats) from LDS
        __shared__ float cs[LDS_TABLE_MAX];
        for (int i = threadIdx.x; i < 2 * d.half + 1; i += nasr_rs::BLOCK) cs[i] = d.table[i];
        __syncthreads();
        if ((int)threadIdx.x < cnt) d.out[o0 + threadIdx.x] = nasr_rs::quantize(nasr_rs::accumulate(pl, cs, n0 + threadIdx.x, x_at));
        return;
    }
    if ((int)threadIdx.x < cnt) d.out[o0 + threadIdx.x] = nasr_rs::quantize(nasr_rs::accumulate(pl, d.table, n0 + threadIdx.x, x_at));
}

void launch_audio_convert(const AudioDesc *descs, int B, long long max_out, hipStream_t st) {
    if (B <= 0) return;
    const unsigned nblk = (unsigned)((max_out + nasr_rs::BLOCK - 1) / nasr_rs::BLOCK);
    hipLaunchKernelGGL(k_audio_convert, dim3(nblk + 1, B), dim3(nasr_rs::BLOCK), 0, st, descs);
}

}  // namespace nasr
