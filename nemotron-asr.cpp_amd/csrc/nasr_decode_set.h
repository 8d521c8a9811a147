// nasr_decode_set.h -- the working set of the device greedy decode: the options in force (DecFeatures), every per-slot and per-row buffer
// its launches touch (DecodeSet), each buffer's size and the option that needs it (dec_set_layout; dec_set_slot_layout: what one slot owns of them), the allocation of what is missing
// (dec_set_ensure) and the DecParams of a launch sequence (dec_set_bind).  The live engine holds one set, the offline path another; a new
// decode option is added here.  Pure host code (tests/test_decode_set.py compiles it with the host compiler); include it after
// nasr_internal.h.  The beam search has a working set of its own (OfflineState::bm_*, BeamParams).
#pragma once
#include <cstring>

namespace nasr {

// the decode options in force: they pick the decode launches that get captured into step graphs, so they are fixed from the first decode on
struct DecFeatures {
    bool token_logprobs = false;     // option "token_logprobs"
    int alt_k = 0;                   // option "token_alternatives" = K (0: off)
    bool frame_blank = false;        // option "frame_blank_logprobs"
    bool phrase_boost = false;       // option "phrase_boost" (the capacity of its tables is the engine's)
    bool lm_fusion = false;          // option "lm_fusion"
    int lm_fold = 1, lm_relook = 0;  // measurement switches "lm_refresh_fold", "lm_commit_lookup"
    int entropy_milli = 0;           // option "token_entropy" = round(1000 alpha) (0: off), nasr_entropy.h
    bool lp_kernels() const { return token_logprobs || alt_k != 0 || frame_blank || entropy_milli != 0; }      // the kernels that leave the softmax parts
    bool winner_raw() const { return phrase_boost || lm_fusion; }                        // the biased forms read the winner's raw logit
};

// [slot]: one entry per decoder slot (a live stream / an utterance of an offline sub-batch); [row]: one per row of a decode iteration (the
// engine's workspace rows / the offline decode windows).  Nothing is freed or moved while the engine lives: captured graphs hold the addresses
struct DecodeSet {
    int slots = 0, rows = 0, alt_k = 0;      // what the buffers were sized for; K the alt_* buffers were allocated for (0: none yet)
    DecCtrl *ctrl = nullptr;                 // [slot]
    float *h = nullptr, *c = nullptr;        // [slot][2 versions][2 layers][640] LSTM state
    float *predg = nullptr;                  // [slot][640] cached joint.pred output of the LSTM candidate
    unsigned long long *key = nullptr;       // [row] packed argmax keys
    int *n_active = nullptr;                 // [4] = n_active, n_dirty, n_rows, ChainParams::error (zeroed by the owner)
    int *dlist = nullptr;                    // [slot] batch rows whose LSTM candidate must be recomputed
    unsigned *rowmap = nullptr;              // [row] (frame << 16 | batch row) of every frame still to decode
    int *tok_ring = nullptr, *tok_frame = nullptr;       // [slot][TOK_CAP] each: the tokens and their absolute encoder frames
    // the LP kernels ("token_logprobs", "token_alternatives", "frame_blank_logprobs")
    nasr_lp::Part *lp_part = nullptr;        // [max(64 x 65, rows x 17)] softmax parts of the rows of a decode iteration (nasr_logprob.h)
    float *tok_logprob = nullptr;            // [slot][TOK_CAP] beside tok_ring / tok_frame
    // "phrase_boost" (the automaton tables [capacity][1040] are the engine's), nasr_boost.h
    int *boost_state = nullptr;              // [slot] automaton state of every slot's emitted history
    float *boost_raw = nullptr;              // scratch beside lp_part: raw logit of every part's winner ("phrase_boost" or "lm_fusion"; read only with the LP kernels)
    // "token_alternatives" = K, nasr_topk.h
    unsigned long long *alt_key = nullptr;   // scratch beside lp_part: [row][slice][K] largest keys of every vocab slice
    int32_t *alt_id = nullptr; float *alt_lp = nullptr;        // [slot][TOK_CAP][K] each, beside tok_ring / tok_frame / tok_logprob
    // "frame_blank_logprobs": the ring is indexed by the absolute frame number since create / reset and is never cleared: the live read-out
    // clips to the frames decoded since then (DecCtrl::frame0 + t, which k_stream_reset zeroes), so what an earlier stream or an earlier
    // life of this one left in a slot's ring is never visible; an offline utterance (T <= 2048 < FRAME_CAP) starts at frame 0
    float *fb_row = nullptr;                 // scratch beside key: [row] ln P(blank) of the rows of a decode iteration
    float *frame_blank = nullptr;            // [slot][FRAME_CAP]
    // "lm_fusion" (the block with the model's view and the greedy weights is the engine's), nasr_lm.h / DESIGN 17
    int32_t *lm_state = nullptr;             // [slot] LM state of the slot's emitted history
    float *lm_row = nullptr; int32_t *lm_next = nullptr;       // [slot][1040] each: the bias row (phrase bonus + lmbias), the next-state row beside it
    // "token_entropy" = round(1000 alpha), nasr_entropy.h
    float *ent_part = nullptr;               // scratch beside lp_part: the entropy term of every part (sum exp(alpha (x - m)), or sum exp(x - m) (x - m) at alpha = 1)
    float *tok_entropy = nullptr;            // [slot][TOK_CAP] beside tok_ring / tok_frame / tok_logprob
};

// THE layout: buf(name, pointer, needed, elements) once for every buffer of the set, for `slots` slots and `rows` rows under features f
template <class Visit>
inline void dec_set_layout(DecodeSet &d, const DecFeatures &f, int slots, int rows, Visit &&buf) {
    const size_t S = (size_t)slots, M = (size_t)rows, K = (size_t)f.alt_k, parts = nasr_lp::scratch_parts(rows);
    const bool lp = f.lp_kernels(), alt = f.alt_k != 0;
    //  buffer                          needed by               elements
    buf("ctrl",        d.ctrl,          true,                   S);
    buf("h",           d.h,             true,                   S * 4 * HID);
    buf("c",           d.c,             true,                   S * 4 * HID);
    buf("predg",       d.predg,         true,                   S * JNT);
    buf("key",         d.key,           true,                   M);
    buf("n_active",    d.n_active,      true,                   (size_t)4);
    buf("dlist",       d.dlist,         true,                   S);
    buf("rowmap",      d.rowmap,        true,                   M);
    buf("tok_ring",    d.tok_ring,      true,                   S * TOK_CAP);
    buf("tok_frame",   d.tok_frame,     true,                   S * TOK_CAP);
    buf("lp_part",     d.lp_part,       lp,                     parts);
    buf("tok_logprob", d.tok_logprob,   lp,                     S * TOK_CAP);
    buf("boost_state", d.boost_state,   f.phrase_boost,         S);
    buf("boost_raw",   d.boost_raw,     f.winner_raw(),         parts);
    buf("alt_key",     d.alt_key,       alt,                    nasr_topk::scratch_keys(rows, f.alt_k));
    buf("alt_id",      d.alt_id,        alt,                    S * TOK_CAP * K);
    buf("alt_lp",      d.alt_lp,        alt,                    S * TOK_CAP * K);
    buf("fb_row",      d.fb_row,        f.frame_blank,          M);
    buf("frame_blank", d.frame_blank,   f.frame_blank,          S * FRAME_CAP);
    buf("lm_state",    d.lm_state,      f.lm_fusion,            S);
    buf("lm_row",      d.lm_row,        f.lm_fusion,            S * nasr_lm::ROW_COLS);
    buf("lm_next",     d.lm_next,       f.lm_fusion,            S * nasr_lm::ROW_COLS);
    buf("ent_part",    d.ent_part,      f.entropy_milli != 0,   parts);
    buf("tok_entropy", d.tok_entropy,   f.entropy_milli != 0,   S * TOK_CAP);
}

// The per-slot part of THE layout: buf(name, pointer, needed, elements_per_slot) once for every buffer whose size grows with the slots and
// whose option is in force under f -- what one slot owns of the set (a stream fork copies it, nasr_fork_plan.h).  Read off dec_set_layout
// itself (its sizes at two slots against one), so a buffer added there is here without being named again; [row] buffers are not listed
template <class Visit>
inline void dec_set_slot_layout(DecodeSet &d, const DecFeatures &f, Visit &&buf) {
    size_t one[64];
    int n = 0, i = 0;
    dec_set_layout(d, f, 1, 1, [&](const char *, auto *&, bool, size_t elems) { if (n < 64) one[n++] = elems; });
    dec_set_layout(d, f, 2, 1, [&](const char *name, auto *&p, bool needed, size_t elems) {
        const size_t per_slot = i < n ? elems - one[i] : 0;
        i++;
        if (needed && per_slot) buf(name, p, needed, per_slot);
    });
}

// Allocates every buffer that f needs and the set does not have yet; never frees or moves one.  alloc(name, &pointer, bytes) returns 0 or
// reports its own failure; a refusal goes through refuse(format, value) (the engine's fail), whose result is returned.  0, or not 0
template <class Alloc, class Refuse>
inline int dec_set_ensure(DecodeSet &d, const DecFeatures &f, int slots, int rows, Alloc &&alloc, Refuse &&refuse) {
    if (f.alt_k && d.alt_k && f.alt_k != d.alt_k) return refuse("token_alternatives: the rings already hold %d entries per token", d.alt_k);
    int rc = 0;
    dec_set_layout(d, f, slots, rows, [&](const char *name, auto *&p, bool needed, size_t n) {
        if (needed && !p && !rc) rc = alloc(name, (void **)&p, n * sizeof(*p));
    });
    d.slots = slots; d.rows = rows;
    if (f.alt_k && !rc) d.alt_k = f.alt_k;
    return rc;
}

// the engine-wide tables the decode reads beside its set (the decoder's weights go in through bind_dec_weights)
struct DecTables { const float *boost_bonus; const int32_t *boost_next; const nasr_lm::Greedy *lm_blk; };

// dp = zeros + the set's pointers: the base part always, an optional part only where its option is in force (a buffer that exists but
// whose option is off stays null: the launches are then the ones without it).  rows, B, T, encproj and the weights are the caller's
inline void dec_set_bind(const DecodeSet &d, const DecFeatures &f, const DecTables &t, DecParams &dp) {
    memset(&dp, 0, sizeof(dp));
    dp.ctrl = d.ctrl; dp.h = d.h; dp.c = d.c; dp.predg = d.predg; dp.key = d.key; dp.dlist = d.dlist; dp.rowmap = d.rowmap;
    dp.n_active = d.n_active; dp.n_dirty = d.n_active + 1; dp.n_rows = d.n_active + 2; dp.tok_ring = d.tok_ring; dp.tok_frame = d.tok_frame;
    if (f.lp_kernels()) { dp.lp_part = d.lp_part; dp.tok_logprob = d.tok_logprob; }
    if (f.frame_blank) { dp.fb_row = d.fb_row; dp.frame_blank = d.frame_blank; }
    if (f.alt_k) { dp.alt_key = d.alt_key; dp.alt_id = d.alt_id; dp.alt_lp = d.alt_lp; dp.alt_k = f.alt_k; }
    if (f.phrase_boost) { dp.boost_bonus = t.boost_bonus; dp.boost_next = t.boost_next; dp.boost_state = d.boost_state; }
    if (f.winner_raw()) dp.boost_raw = d.boost_raw;
    if (f.lm_fusion) { dp.lm_blk = t.lm_blk; dp.lm_state = d.lm_state; dp.lm_row = d.lm_row; dp.lm_next = d.lm_next; dp.lm_fold = f.lm_fold; dp.lm_relook = f.lm_relook; }
    if (f.entropy_milli) { dp.ent_part = d.ent_part; dp.tok_entropy = d.tok_entropy; dp.ent_alpha = nasr_ent::alpha_of(f.entropy_milli); }
}

}  // namespace nasr
