// nasr_diar_set.h -- the working set of a TitaNet-L embedding call (nasr_diar.hip): every activation and scratch buffer its launches
// touch (SpkSet), each buffer's size and the engine that needs it (spk_set_layout), and the allocation of what is missing (spk_set_ensure).
// The f32 engine runs the network layer by layer (spk_embed_layers_f32), the bf16 engine on segment tiles (spk_embed_segment_tiles): each
// gets its own buffers and not the other's.  Pure host code (tests/test_diar_set.py compiles it with the host compiler); include it after
// nasr_internal.h.
#pragma once
#include <cstddef>

namespace nasr {

// [seg]: one entry per sub-segment of a call (S = max_segments); [row]: one per frame row, M = S x 160.  Nothing is freed or moved while
// the engine lives: captured graphs hold the addresses
struct SpkSet {
    // both engines
    float *s_mel = nullptr;                  // [row][96] log-mel, 80 channels zero padded
    float *Y = nullptr;                      // [row][3072] a block's pointwise output (f32 engine: also the attention logits)
    float *se_z = nullptr, *se_h = nullptr;  // [2][seg][3072] SE gate pre-activation ; masked mean, [seg][384] hidden layer
    float *att_c = nullptr, *att_g = nullptr;    // [seg][128] mean / std thirds of the attention conv, [row][128] its x third
    float *pool = nullptr, *emb = nullptr;   // [seg][6144] attentive statistics, [seg][192] embeddings
    int *s_lens = nullptr; long long *s_off = nullptr;       // [seg] valid frames, sample offset in the staged audio
    // f32 engine: block outputs ping-pong, residual branch, masked statistics, GEMM A operand (up to 3072 channels)
    float *X0 = nullptr, *X1 = nullptr, *R = nullptr, *st_mean = nullptr, *st_std = nullptr, *A32 = nullptr;
    // bf16 engine (kernels_spk.hip): A operands ping-pong [row][1024], block outputs [row][1024] x 2, encoder output [row][3072]
    bf16_t *sA[2] = {nullptr, nullptr}, *sX[2] = {nullptr, nullptr}, *sX4 = nullptr;
    float *st_ms = nullptr, *fc_part = nullptr;      // [seg][2 C] masked mean ; std, split-K scratch of launch_spk_fc
    bf16_t *A16 = nullptr;                   // [row][128] operand of the second attention conv (the only thing k_spk_att_post writes, SG_ASP reads)
};

// THE layout: buf(name, pointer, needed, elements) once for every buffer of the set, for S segments
template <class Visit>
inline void spk_set_layout(SpkSet &d, bool bf16, int max_segments, Visit &&buf) {
    const size_t S = (size_t)max_segments, M = S * SPK_T, C = SPK_C;
    //  buffer                      needed by   elements
    buf("s_mel",    d.s_mel,        true,       M * 96);
    buf("Y",        d.Y,            true,       M * C);
    buf("se_z",     d.se_z,         true,       2 * S * C);
    buf("se_h",     d.se_h,         true,       S * (C / 8));
    buf("att_c",    d.att_c,        true,       S * SPK_ATT);
    buf("att_g",    d.att_g,        true,       M * SPK_ATT);
    buf("pool",     d.pool,         true,       S * 2 * C);
    buf("emb",      d.emb,          true,       S * SPK_EMB);
    buf("s_lens",   d.s_lens,       true,       S);
    buf("s_off",    d.s_off,        true,       S);
    buf("X0",       d.X0,           !bf16,      M * C);
    buf("X1",       d.X1,           !bf16,      M * C);
    buf("R",        d.R,            !bf16,      M * 1024);
    buf("st_mean",  d.st_mean,      !bf16,      S * C);
    buf("st_std",   d.st_std,       !bf16,      S * C);
    buf("A",        d.A32,          !bf16,      M * C);
    buf("sA0",      d.sA[0],        bf16,       M * 1024);
    buf("sA1",      d.sA[1],        bf16,       M * 1024);
    buf("sX0",      d.sX[0],        bf16,       M * 1024);
    buf("sX1",      d.sX[1],        bf16,       M * 1024);
    buf("sX4",      d.sX4,          bf16,       M * C);
    buf("st_ms",    d.st_ms,        bf16,       S * 2 * C);
    buf("fc_part",  d.fc_part,      bf16,       16 * S * 512);
    buf("A",        d.A16,          bf16,       M * SPK_ATT);
}

// Allocates every buffer the engine needs and the set does not have yet; never frees or moves one.  alloc(name, &pointer, bytes) returns
// 0 or reports its own failure.  0, or not 0
template <class Alloc>
inline int spk_set_ensure(SpkSet &d, bool bf16, int max_segments, Alloc &&alloc) {
    int rc = 0;
    spk_set_layout(d, bf16, max_segments, [&](const char *name, auto *&p, bool needed, size_t n) {
        if (needed && !p && !rc) rc = alloc(name, (void **)&p, n * sizeof(*p));
    });
    return rc;
}

}  // namespace nasr
