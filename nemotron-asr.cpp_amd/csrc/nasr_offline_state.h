// nasr_offline_state.h -- what the translation units of the offline path share: its state and device buffers, the description of a
// sub-batch and the driver of an offline call.  nasr_offline.hip = encoder, PCM-to-mel stage, driver, greedy mode, taps; nasr_offline_align.hip = the
// align mode and its read-out; nasr_offline_beam.hip = the beam mode and its read-outs.
#pragma once
#include "nasr_engine_priv.h"
#include "nasr_offline.h"

#include <memory>

// a device buffer of the offline path: grown on demand (nasr_eng::grow), never shrunk, owned by OfflineState::bufs
struct OffBuf {
    void *p = nullptr; size_t cap = 0;
    template <class T> T *as() const { return (T *)p; }
};

struct OfflineState {
    std::vector<void *> bufs;                    // everything below, freed with the engine (or when a buffer grows)
    int rows_cap = 0;
    OffBuf x, glu, hfuse, encproj, a, hbuf, qkv, ctx, cbuf, tpos, items, prow;     // the row buffers (ensure_rows): f32 x / glu / hfuse / encproj, act dtype a .. cbuf
    OffBuf part, sub_a, sub_b, mel;              // split-K slab, front-end images (f32 sized), packed log-mel
    float *zero_bias = nullptr;
    // PCM entry: the streaming front end's buffers for a group of utterances (one preprocessor state each) and the log-mel it produces
    float *abuf = nullptr, *last_sample = nullptr, *mel_ring = nullptr; PcmDesc *pdesc = nullptr;
    OffBuf pmel, pcm;
    OffSubDesc *sdesc = nullptr;
    std::vector<void *> pos;                     // per layer [4095][1024] act dtype
    // greedy decode: one slot per utterance of a sub-batch, OFF_DEC_WIN rows per slot (nasr_decode_set.h; allocated with the row buffers for the
    // engine's decode options, which the first offline call freezes); win = the encoder projection of the window being decoded
    DecodeSet dec;
    float *win = nullptr; RowDesc *drows = nullptr; int4 *dwin = nullptr;
    bool no_boost = false, no_lm = false;                          // NASR_FLAG_NO_BOOST, NASR_FLAG_NO_LM of the call in progress
    std::vector<std::vector<int32_t>> alt_ids; std::vector<std::vector<float>> alt_lps;             // "token_alternatives" of the last call, by utterance: [tokens][K] each
    std::vector<std::vector<float>> frame_blank_lps;               // "frame_blank_logprobs" of the last call, by utterance: [T] (nasr_engine_offline_frame_blank_logprobs)
    std::vector<std::vector<float>> entropies;                     // "token_entropy" of the last call, by utterance (nasr_engine_offline_token_entropies)
    std::vector<std::vector<float>> logprobs;                      // "token_logprobs" of the last call, by utterance (nasr_engine_offline_token_logprobs)
    // forced alignment (nasr_engine_align*): the prediction-network rows g, the lattice of the sub-batch in flight (two values and one
    // back-pointer byte per cell), its descriptors and its results
    OffBuf al_g, al_lpb, al_lpt, al_tlp, al_bp, al_tiles, al_tok, al_frames;
    nasr_align::Utt *al_utt = nullptr; double *al_scores = nullptr;
    bool lat_valid = false;                                        // the last call was an align call with debug on
    std::vector<std::vector<float>> lat_b, lat_t;                  // ... its lattices by utterance: lp_blank, lp_token [T][U + 1]
    // beam search (nasr_engine_transcribe_beam*): its own decoder slots (3 W per utterance), batch rows (W per utterance), the joint's LP + ALT
    // scratch whatever the engine options are, the search state and trie of the sub-batch in flight, and the results of the last call
    OffBuf bm_utt, bm_beam, bm_nodes, bm_enc, bm_rows, bm_ctrl, bm_h, bm_c, bm_predg, bm_key, bm_part, bm_alt, bm_cnt, bm_dlist, bm_rowmap, bm_out_lm, bm_bstate, bm_raw, bm_out_boost,
           bm_out_n, bm_out_len, bm_out_score, bm_out_tok, bm_out_frame, bm_out_lp;
    struct BeamHyp { double score; std::vector<int32_t> tokens, frames; std::vector<float> lps; double lm_final = 0.0, total = 0.0;
                     double boost = 0.0; std::vector<float> bonuses; };     // a boosted call: the sum and the per-token bonuses by the set in force during it
    long long beam_lm_generation = 0;                              // the engine's lm_generation at that call
    bool beam_valid = false, beam_lm = false;                      // beam_lm: the last beam call ran with a language model (nasr_engine_set_lm)
    bool beam_boost = false;                                       // the last beam call was boosted (NASR_FLAG_BEAM_BOOST)
    std::vector<std::vector<BeamHyp>> beam_res;                    // by utterance, best first
    float *t_sub = nullptr, *t_lay = nullptr, *t_enc = nullptr;   // debug taps of the sub-batch in flight
    // debug taps of the last call, by utterance
    std::vector<std::vector<float>> tap_mel, tap_sub, tap_enc;
    std::vector<std::vector<std::vector<float>>> tap_lay;
};

namespace nasr_eng {

int off_alloc(OfflineState *o, void **p, size_t bytes);         // at least 16 bytes, recorded in o->bufs
int grow(nasr_engine *e, OfflineState *o, OffBuf &b, size_t bytes);   // room for `bytes`; a larger buffer replaces b behind everything queued on the stream

// a sub-batch whose encoder has been enqueued: utterances [first, first + n) of the call, utterance first + k in packed rows
// [off[k], off[k] + T[k]) of o->encproj (and of the debug taps)
struct OffBatch { int first = 0, n = 0, M = 0, maxT = 0; std::vector<int> off, T; };

// the input of an offline call: the log-mel of every utterance in host memory, or its 16 kHz s16 samples (host, or device with NASR_FLAG_PCM_DEVICE)
// ... or, engine option "frame_history", windows of live streams' kept encoder-projection rows: frames [first[b], first[b] + n[b]) of streams[b].
// Such a call runs no front end and no encoder: o->encproj is filled by the gather (k_history_gather), then the mode's batch step runs unchanged
struct OffInput { bool is_pcm; const float *const *mel; const int16_t *const *pcm; const int32_t *n;
                  bool is_history = false; nasr_stream *const *streams = nullptr; const int64_t *first = nullptr; };
inline OffInput mel_input(const float *const *mel, const int32_t *n_frames) { return {false, mel, nullptr, n_frames}; }
inline OffInput pcm_input(const int16_t *const *pcm, const int32_t *n_samples) { return {true, nullptr, pcm, n_samples}; }
inline OffInput history_input(nasr_stream *const *streams, const int64_t *first, const int32_t *count) { return {false, nullptr, nullptr, count, true, streams, first}; }

// What a mode (greedy, align, beam) supplies to offline_call, in the order it is called.  early and check may be empty
struct OffMode {
    const char *who = "";                                          // the entry's name, for begin_call's messages
    const int32_t *counts = nullptr;                               // the entry's per-utterance count array: begin_call refuses a null one
    bool greedy = false;                                           // the greedy mode: the only one that takes NASR_FLAG_NO_LM
    bool streaming_hint = false;                                   // the over-limit message points at the streaming path
    std::function<int()> early;                                    // checks that hold for B == 0 too, before any other argument is looked at
    std::function<int(int B)> check;                               // checks whose failure has already forgotten the call before
    std::function<int(OfflineState *, int B)> setup;               // room for the results of B utterances
    std::function<int(OfflineState *, const OffBatch &)> batch;    // the sub-batch whose encoder projection is in o->encproj (also with ob.M == 0)
    std::function<void(OfflineState *)> failed;                    // setup, an encoder, a batch step or a tap fetch failed (may be empty)
    std::function<int(OfflineState *, int B)> finish;              // results to the caller
};
int offline_call(nasr_engine *e, int B, const OffInput &in, const int32_t *prompt_index, uint32_t flags, const OffMode &m);

// the tail of a read-out: the count on a size query (out == nullptr), else the first min(count, cap) values copied and their number
template <class T>
inline int64_t read_out(const std::vector<T> &src, T *out, int64_t cap) {
    if (!out) return (int64_t)src.size();
    const int64_t n = std::min<int64_t>((int64_t)src.size(), std::max<int64_t>(cap, 0));
    memcpy(out, src.data(), (size_t)n * sizeof(T));
    return n;
}

}  // namespace nasr_eng
