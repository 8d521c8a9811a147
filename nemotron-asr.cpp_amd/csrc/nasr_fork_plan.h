// nasr_fork_plan.h -- the copy plan of a stream fork: the segments that make slot B the twin of slot A, and their cut into the pieces
// k_stream_fork's workgroups move (kernels_front.hip).  Only the LIVE part of a slot is copied: the 70 K/V window rows a key can name, the
// buffered mel frames, the waiting samples -- not the rings around them.  Pure host code without HIP, compiled and tested on a CPU under
// sanitizers (tests/test_fork_plan.py), like nasr_step_plan.h and nasr_offline_plan.h; include it after nasr_internal.h and nasr_decode_set.h.
#pragma once
#include <cstring>
#include <vector>

namespace nasr_fork {
using namespace nasr;

// whose base address an offset counts from: the engine's pools (KV and CC: the pool of Seg::layer), or a buffer of the DecodeSet (Seg::base)
enum Buf { BUF_KV = 0, BUF_CC, BUF_MEL, BUF_ABUF, BUF_LAST_SAMPLE, BUF_AUD_HIST, BUF_DEC };

// the source stream's host mirror, as far as it says what is live (nasr_stream)
struct Source { int kv_head, mel_start, mel_count, abuf_cnt, abuf_par; };

// bytes [src, src + bytes) -> [dst, dst + bytes) of one buffer, offsets from the buffer's base; slot_bytes: what one slot owns of it.
// blob: the segment's offset in the device section of a snapshot (nasr_snapshot.h; a fork leaves it 0)
struct Seg { int buf, layer; const char *name; char *base; int64_t src, dst, bytes, slot_bytes, blob = 0; };

// Segments move as 16-byte vectors; the buffers below hold one 4-byte value per slot, or (aud_hist: 2 x 193 floats) slots that are no multiple
// of 16 bytes, and move as 4-byte words
inline bool word_item(const char *name) {
    return !strcmp(name, "last_sample") || !strcmp(name, "aud_hist") || !strcmp(name, "boost_state") || !strcmp(name, "lm_state");
}
// sized by the slots but indexed by a decode iteration's list position, not by slot: scratch, like the [row] buffers
inline bool positional_scratch(const char *name) { return !strcmp(name, "dlist"); }

// rows first .. first + count - 1 (mod ring) of a ring of `ring` rows that starts at byte `at` of both slots' parts: two segments where they wrap
inline void ring_rows(std::vector<Seg> &out, Seg s, int64_t at, int first, int count, int ring, int64_t row_bytes) {
    if (count > ring) count = ring;
    const int64_t src0 = s.src, dst0 = s.dst;
    const int n1 = count < ring - first ? count : ring - first;
    if (n1 > 0) { s.src = src0 + at + first * row_bytes; s.dst = dst0 + at + first * row_bytes; s.bytes = n1 * row_bytes; out.push_back(s); }
    if (count > n1) { s.src = src0 + at; s.dst = dst0 + at; s.bytes = (count - n1) * row_bytes; out.push_back(s); }
}

// THE plan: what slot `dst_slot` must receive to continue exactly as slot `src_slot` would.  esz: bytes per K/V element; the decoder's
// buffers are the per-slot part of the set under the features in force (dec_set_slot_layout)
inline std::vector<Seg> fork_plan(const Source &m, int src_slot, int dst_slot, int esz, int n_layers, int kernel_size, DecodeSet &d, const DecFeatures &f) {
    std::vector<Seg> out;
    const auto slot_seg = [&](int buf, int layer, const char *name, char *base, int64_t slot_bytes) {
        return Seg{buf, layer, name, base, src_slot * slot_bytes, dst_slot * slot_bytes, slot_bytes, slot_bytes};
    };
    const int64_t row = (int64_t)D * esz, plane = KVC * row, cc = 2 * (int64_t)(kernel_size - 1) * D * 4;
    for (int l = 0; l < n_layers; l++) {
        // logical keys 0 .. LCTX-1 = ring rows (kv_head + j) % KVC of K (plane 0) and V (plane 1): the rows k_stream_reset zeroes
        for (int p = 0; p < 2; p++) ring_rows(out, slot_seg(BUF_KV, l, "kv", nullptr, 2 * plane), p * plane, m.kv_head % KVC, LCTX, KVC, row);
        out.push_back(slot_seg(BUF_CC, l, "cc", nullptr, cc));                       // conv cache, both parities
    }
    ring_rows(out, slot_seg(BUF_MEL, -1, "mel", nullptr, (int64_t)MEL_RING * NMEL * 4), 0, m.mel_start & (MEL_RING - 1), m.mel_count, MEL_RING, NMEL * 4);
    {   // the waiting samples of the live parity, rounded up to 16 bytes (ABUF_CAP has the slack)
        Seg s = slot_seg(BUF_ABUF, -1, "abuf", nullptr, 2 * (int64_t)ABUF_CAP * 4);
        const int64_t at = (int64_t)(m.abuf_par & 1) * ABUF_CAP * 4, cap = (int64_t)ABUF_CAP * 4;
        s.src += at; s.dst += at;
        s.bytes = ((int64_t)m.abuf_cnt * 4 + 15) & ~(int64_t)15;
        if (s.bytes > cap) s.bytes = cap;
        if (s.bytes > 0) out.push_back(s);
    }
    out.push_back(slot_seg(BUF_LAST_SAMPLE, -1, "last_sample", nullptr, 4));
    out.push_back(slot_seg(BUF_AUD_HIST, -1, "aud_hist", nullptr, 2 * (int64_t)nasr_rs::HIST_MAX * 4));      // audio converter, both parities
    dec_set_slot_layout(d, f, [&](const char *name, auto *&p, bool, size_t per_slot) {
        if (!positional_scratch(name)) out.push_back(slot_seg(BUF_DEC, -1, name, (char *)p, (int64_t)(per_slot * sizeof(*p))));
    });
    return out;
}

inline int64_t plan_bytes(const std::vector<Seg> &segs) {
    int64_t n = 0;
    for (const Seg &s : segs) n += s.bytes;
    return n;
}

// What the engine checks before it launches: every segment lies inside its own slot's part of its buffer on both sides, and is made of
// 16-byte vectors unless it is a word item (then of 4-byte words).  nullptr, or what is wrong
// one side of one segment: [at, at + bytes) inside slot's part of the buffer, in whole vectors (words)
inline const char *seg_fault(const Seg &s, int64_t at, int slot, const char *leaves) {
    if (s.bytes <= 0 || s.slot_bytes <= 0) return "empty segment";
    if (at < slot * s.slot_bytes || at + s.bytes > (slot + 1) * s.slot_bytes) return leaves;
    if ((at | s.bytes) & (word_item(s.name) ? 3 : 15)) return "misaligned segment";
    return nullptr;
}
inline const char *plan_fault(const std::vector<Seg> &segs, int src_slot, int dst_slot) {
    if (src_slot == dst_slot || src_slot < 0 || dst_slot < 0) return "source and destination slot must differ";
    for (const Seg &s : segs) {
        if (const char *what = seg_fault(s, s.src, src_slot, "source range leaves its slot")) return what;
        if (const char *what = seg_fault(s, s.dst, dst_slot, "destination range leaves its slot")) return what;
    }
    return nullptr;
}

// one workgroup of k_stream_fork moves one piece (nasr_internal.h)
using Piece = StreamForkPiece;

// cuts seg (its buffer at `base`) into pieces of at most piece_bytes (a multiple of 16)
inline void cut_pieces(std::vector<Piece> &out, const Seg &s, char *base, int64_t piece_bytes) {
    for (int64_t at = 0; at < s.bytes; at += piece_bytes) {
        const int64_t n = s.bytes - at < piece_bytes ? s.bytes - at : piece_bytes;
        out.push_back(Piece{base + s.src + at, base + s.dst + at, (uint32_t)n, 0});
    }
}

// Bytes a workgroup moves at most.  At bf16 and 24 layers a fork moves 8.5 MB, 6.9 MB of it K/V window rows in runs of at most 143 KB: at
// 256 KiB every segment is one piece, 82 workgroups (3.4 per layer).  Measured between the engine's own events (profiles/stream_fork.md;
// engine option "fork_piece_kb" for A/B runs): 17.4 us, against 19.3 us at 128 KiB (130 workgroups), 18.9 us at 64 KiB (178) and 20 us at 16
// and 4 KiB (540, 2 093)
constexpr int PIECE_BYTES = 256 * 1024;

}  // namespace nasr_fork
