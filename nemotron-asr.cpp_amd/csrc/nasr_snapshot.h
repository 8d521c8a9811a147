// nasr_snapshot.h -- a stream snapshot in host memory: the blob nasr_stream_save writes and nasr_stream_restore reads.  Pure host
// code without HIP, compiled and tested on a CPU under sanitizers (tests/test_snapshot_format.py), like nasr_fork_plan.h, whose plan it
// extends: include it after nasr_internal.h, nasr_decode_set.h and nasr_fork_plan.h.  Only word_term is shared with the device
// (k_stream_pack / k_stream_unpack, kernels_front.hip).
//
// Format, version 1, every value little-endian:
//   header  144 bytes   magic "NASS", version, total size; what restore must agree on (dtype and element size, n_layers, kernel_size, KVC,
//                       LCTX, MEL_RING, NMEL, ABUF_CAP, the converter's HIST_MAX, TOK_CAP, the five DecFeatures values); the fingerprints
//                       of the weight set, the boost set and the LM in force; the sizes of the two sections; the checksum of the device
//                       section; 4 reserved bytes (zero) and, in the word behind them (offset 132), the sixth DecFeatures value, option
//                       "token_entropy" (0 = off: a blob saved with it off is byte for byte what it was before the option existed);
//                       the checksum of header and mirror
//   mirror              the record of what the stream is (struct Mirror: nasr_stream derives from it, so the stream IS the record and nothing
//                       copies it field by field), its fixed fields in wire order (visit_fields), then the queued tokens, zero-padded to 16 bytes
//   device              the segments of the fork plan for this mirror (nasr_fork::fork_plan) in plan order, each zero-padded to 16 bytes.
//                       Ring rows come in logical order (ring_rows), so the bytes do not depend on the slot; they do name the ring
//                       positions (kv_head, mel_start), which restore keeps
// No offset or length inside the blob is trusted: restore recomputes the plan from the parsed mirror and its own engine's configuration
// and requires the section sizes to be what the plan says.
//
// The format is INTEGRITY-CHECKED, NOT AUTHENTICATED: the two checksums catch corruption in transit or on disk.  A forged blob with
// matching checksums is outside the promise (what a kernel uses as an index is range-checked all the same: device_fault).
#pragma once
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define NASR_SNAP_HD __host__ __device__ inline
#else
#define NASR_SNAP_HD inline
#endif

namespace nasr_snap {
using namespace nasr;
using nasr_fork::Seg;

constexpr uint32_t MAGIC = 0x5353414Eu;        // "NASS"
constexpr uint32_t VERSION = 1;
constexpr int64_t HEADER_BYTES = 144, HEAD_SUM_AT = 136, MIRROR_FIXED = 100;

// ---- THE checksum of the device section (host and kernels): word w at word index i of the section adds fmix32(w ^ i * 0x9E3779B1) to a sum
// mod 2^64 -- order-free (any cut into pieces gives the same value), position-sensitive, integer (host and device agree exactly).  fmix32
// (murmur3's finaliser) is a bijection, so a change of one word always changes its term, and with it the sum
NASR_SNAP_HD uint32_t fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu;
    h ^= h >> 13; h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}
NASR_SNAP_HD uint64_t word_term(uint32_t w, uint32_t i) { return (uint64_t)fmix32(w ^ (uint32_t)(i * 0x9E3779B1u)); }
// bytes (a multiple of 4) at p whose first word has index word0
inline uint64_t checksum(const void *p, int64_t bytes, uint32_t word0) {
    uint64_t sum = 0;
    const uint8_t *b = (const uint8_t *)p;
    for (int64_t i = 0; i < bytes / 4; i++) {
        uint32_t w;
        memcpy(&w, b + 4 * i, 4);
        sum += word_term(w, word0 + (uint32_t)i);
    }
    return sum;
}

// ---- fingerprints: 64 bits that name the tables a stream's decoder state refers to -----------------------------------------------------
inline uint64_t mix64(uint64_t x) {        // splitmix64's finaliser
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
inline uint64_t hash_bytes(uint64_t h, const void *p, size_t n) {
    const uint8_t *b = (const uint8_t *)p;
    h = mix64(h ^ (uint64_t)n);
    for (; n >= 8; n -= 8, b += 8) { uint64_t w; memcpy(&w, b, 8); h = mix64(h ^ w); }
    if (n) { uint64_t w = 0; memcpy(&w, b, n); h = mix64(h ^ w); }
    return h;
}
// One tensor of the weight set: its name, type and shape, and a BOUNDED sample of its bytes -- everything up to 1 KiB, else the first and the
// last 256 bytes and 32 windows of 16 bytes at evenly spaced offsets (1 KiB of a tensor of any size; 1.2 GB are not hashed).  The set's
// fingerprint is the sum of its tensors' (the order in which a loader hands them over does not matter)
constexpr size_t FP_FULL = 1024, FP_EDGE = 256, FP_WINDOWS = 32, FP_WINDOW = 16;
inline uint64_t tensor_fingerprint(const char *name, int type, int n_dims, const int64_t *ne, const void *data, size_t bytes) {
    uint64_t h = hash_bytes(0x6E617372ull, name, strlen(name));
    h = mix64(h ^ (uint64_t)(uint32_t)type);
    for (int i = 0; i < n_dims && i < 4; i++) h = mix64(h ^ (uint64_t)ne[i]);
    const uint8_t *b = (const uint8_t *)data;
    if (!b || bytes <= FP_FULL) return hash_bytes(h, b, b ? bytes : 0);
    h = hash_bytes(h, b, FP_EDGE);
    h = hash_bytes(h, b + bytes - FP_EDGE, FP_EDGE);
    const size_t span = bytes - 2 * FP_EDGE - FP_WINDOW;
    for (size_t k = 0; k < FP_WINDOWS; k++) h = hash_bytes(h, b + FP_EDGE + span / FP_WINDOWS * k, FP_WINDOW);
    return h;
}

// ---- header and mirror -------------------------------------------------------------------------------------------------------------------
// what the saving and the restoring engine must agree on
struct Config {
    uint32_t dtype = 0, esz = 0, n_layers = 0, kernel_size = 0;
    uint32_t kvc = KVC, lctx = LCTX, mel_ring = MEL_RING, nmel = NMEL, abuf_cap = ABUF_CAP, hist_max = nasr_rs::HIST_MAX, tok_cap = TOK_CAP;
    uint32_t token_logprobs = 0, alt_k = 0, frame_blank = 0, phrase_boost = 0, lm_fusion = 0;      // DecFeatures
    uint32_t entropy_milli = 0;                    // ... and "token_entropy", which sits in the high word of the once reserved bytes
    uint64_t fp_weights = 0, fp_boost = 0, fp_lm = 0;
};
inline Config make_config(int dtype, int esz, int n_layers, int kernel_size, const DecFeatures &f, uint64_t fp_weights, uint64_t fp_boost, uint64_t fp_lm) {
    Config c;
    c.dtype = (uint32_t)dtype; c.esz = (uint32_t)esz; c.n_layers = (uint32_t)n_layers; c.kernel_size = (uint32_t)kernel_size;
    c.token_logprobs = f.token_logprobs; c.alt_k = (uint32_t)f.alt_k; c.frame_blank = f.frame_blank; c.phrase_boost = f.phrase_boost; c.lm_fusion = f.lm_fusion;
    c.entropy_milli = (uint32_t)f.entropy_milli;
    c.fp_weights = fp_weights; c.fp_boost = fp_boost; c.fp_lm = fp_lm;
    return c;
}
inline DecFeatures features_of(const Config &c) {
    DecFeatures f;
    f.token_logprobs = c.token_logprobs != 0; f.alt_k = (int)c.alt_k; f.frame_blank = c.frame_blank != 0; f.phrase_boost = c.phrase_boost != 0; f.lm_fusion = c.lm_fusion != 0;
    f.entropy_milli = (int)c.entropy_milli;
    return f;
}
struct Header { Config cfg; uint64_t total_bytes = 0, mirror_bytes = 0, device_bytes = 0, device_sum = 0, head_sum = 0; };

// THE record of what a stream is on the host: struct nasr_stream (nasr_engine_priv.h) derives from it and adds only what is not state -- the
// engine and the slot, T (1 + R), the tap fields, aud_plan and aud_table (recomputed from the format the way nasr_stream_set_audio_format
// does).  Create, reset, fork, save and restore all go through this one declaration.  The two enable flags are words, not bools: parse must
// be able to hold a 7 in order to refuse it.  The audio format is nasr_audio_format's four integers (encoding 0 = NASR_AUDIO_S16)
struct Mirror {
    int32_t R = 0, prompt = -1;
    int32_t abuf_cnt = 0, abuf_par = 0;            // samples waiting in the audio buffer (pre-seeded 256 zeros), and its parity
    int32_t mel_start = 0, mel_count = 0;          // mel ring window
    int32_t valid_len = 0, kv_head = 0, cc_par = 0;    // cache_valid_len, K/V ring head, conv-cache parity
    int32_t chunks = 0, tok_read = 0;
    int64_t samples_in = 0;
    uint32_t boost_enabled = 1, lm_enabled = 1;    // nasr_stream_set_boost / nasr_stream_set_lm (engine options "phrase_boost" / "lm_fusion")
    int32_t sample_rate = 16000, encoding = 0, channels = 1, channel = 0;      // nasr_stream_set_audio_format: survives a reset, the counters below do not
    int64_t aud_in = 0, aud_out = 0;               // input frames taken / 16 kHz samples produced since create or reset
    int32_t aud_par = 0;                           // parity of the history buffer that holds the frames before the next push
    std::vector<int32_t> tok_queue;                // tokens gathered from the device, not yet handed to the caller
    bool default_format() const { return sample_rate == 16000 && encoding == 0 && channels == 1 && channel == 0; }
};

// THE field table: f(name, field, lo, hi) for every fixed field in wire order, [lo, hi] its inclusive range.  write_head, parse and
// mirror_fault are written over it.  Three ranges say less than the rule: R is one of 0, 1, 6, 13, prompt ends at the restoring engine's
// num_prompts - 1, and the four format fields are judged together (audio_format_fault) -- mirror_fault keeps those explicit
template <class M, class F>
inline void visit_fields(M &m, F &&f) {
    f("R", m.R, 0, 13); f("prompt", m.prompt, -1, INT32_MAX);
    f("abuf_cnt", m.abuf_cnt, 0, ABUF_CAP); f("abuf_par", m.abuf_par, 0, 1);
    f("mel_start", m.mel_start, 0, MEL_RING - 1); f("mel_count", m.mel_count, 0, MEL_RING);
    f("valid_len", m.valid_len, 0, LCTX); f("kv_head", m.kv_head, 0, KVC - 1); f("cc_par", m.cc_par, 0, 1);
    f("chunks", m.chunks, 0, INT32_MAX); f("tok_read", m.tok_read, 0, INT32_MAX);
    f("samples_in", m.samples_in, 0, INT64_MAX);
    f("boost_enabled", m.boost_enabled, 0, 1); f("lm_enabled", m.lm_enabled, 0, 1);
    f("sample_rate", m.sample_rate, INT32_MIN, INT32_MAX); f("encoding", m.encoding, INT32_MIN, INT32_MAX);
    f("channels", m.channels, INT32_MIN, INT32_MAX); f("channel", m.channel, INT32_MIN, INT32_MAX);
    f("aud_in", m.aud_in, 0, INT64_MAX); f("aud_out", m.aud_out, 0, INT64_MAX);
    f("aud_par", m.aud_par, 0, 1);
}

// What a reset leaves of the record (k_stream_reset is the device's half).  Both modes start the mel window, the validity mask, the
// counters, the audio converter and the token queue over; only a fresh reset also forgets the preprocessor's carry and the ring positions
// (keep_reference_state: what the reference's nemo_stream_context::reset() leaves behind, see stream_zero_state).  R, prompt, the audio
// format and the two enable flags survive both.  A default record through the fresh reset is a new stream
inline void reset_state(Mirror &m, bool keep_reference_state) {
    if (!keep_reference_state) {
        m.abuf_cnt = NFFT / 2;                     // 256 zero samples pre-seeded, src/preprocessor.cpp:220-221
        m.abuf_par = 0;
        m.kv_head = 0;
        m.cc_par = 0;
    }
    m.mel_start = 0;
    m.mel_count = PRE_CACHE;                       // 9 literal-zero frames, src/nemo-stream.cpp:73-74 (reset: :100-102)
    m.valid_len = 0;                               // :81 (reset: :112)
    m.chunks = 0;
    m.tok_read = 0;
    m.samples_in = 0;
    m.aud_in = m.aud_out = 0;                      // the audio converter starts over in both modes; the format stays
    m.aud_par = 0;
    m.tok_queue.clear();
}

// the record, as far as it says what of the slot is live (the fork plan's input)
inline nasr_fork::Source live_part(const Mirror &m) { return {m.kv_head, m.mel_start, m.mel_count, m.abuf_cnt, m.abuf_par}; }

inline int64_t pad16(int64_t n) { return (n + 15) & ~(int64_t)15; }
inline int64_t mirror_bytes(size_t n_queue) { return pad16(MIRROR_FIXED + 4 * (int64_t)n_queue); }

struct Writer {
    std::vector<uint8_t> &out;
    void u32(uint32_t v) { for (int i = 0; i < 4; i++) out.push_back((uint8_t)(v >> (8 * i))); }
    void u64(uint64_t v) { for (int i = 0; i < 8; i++) out.push_back((uint8_t)(v >> (8 * i))); }
    template <class V> void field(V v) { if (sizeof(V) == 8) u64((uint64_t)v); else u32((uint32_t)v); }       // a 32- or 64-bit field of the mirror
};
struct Reader {
    const uint8_t *p;
    uint32_t u32() { uint32_t v = 0; for (int i = 0; i < 4; i++) v |= (uint32_t)p[i] << (8 * i); p += 4; return v; }
    uint64_t u64() { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i); p += 8; return v; }
    template <class V> void field(V &v) { v = sizeof(V) == 8 ? (V)u64() : (V)u32(); }
};

// header + mirror (HEADER_BYTES + mirror_bytes bytes) into out, with the sizes and the head checksum filled in; device_bytes and device_sum are the caller's
inline void write_head(Header h, const Mirror &m, std::vector<uint8_t> &out) {
    out.clear();
    Writer w{out};
    const Config &c = h.cfg;
    h.mirror_bytes = (uint64_t)mirror_bytes(m.tok_queue.size());
    h.total_bytes = (uint64_t)HEADER_BYTES + h.mirror_bytes + h.device_bytes;
    w.u32(MAGIC); w.u32(VERSION); w.u64(h.total_bytes);
    for (uint32_t v : {c.dtype, c.esz, c.n_layers, c.kernel_size, c.kvc, c.lctx, c.mel_ring, c.nmel, c.abuf_cap, c.hist_max, c.tok_cap,
                       c.token_logprobs, c.alt_k, c.frame_blank, c.phrase_boost, c.lm_fusion}) w.u32(v);
    w.u64(c.fp_weights); w.u64(c.fp_boost); w.u64(c.fp_lm);
    w.u64(h.mirror_bytes); w.u64(h.device_bytes); w.u64(h.device_sum);
    w.u32(0);                                                  // reserved
    w.u32(c.entropy_milli);
    w.u64(0);                                                  // the head checksum, below
    visit_fields(m, [&](const char *, auto v, long long, long long) { w.field(v); });
    w.u32((uint32_t)m.tok_queue.size());
    for (int32_t t : m.tok_queue) w.u32((uint32_t)t);
    out.resize((size_t)(HEADER_BYTES + (int64_t)h.mirror_bytes), 0);
    const uint64_t sum = checksum(out.data(), HEAD_SUM_AT, 0) + checksum(out.data() + HEADER_BYTES, (int64_t)h.mirror_bytes, (uint32_t)(HEADER_BYTES / 4));
    for (int i = 0; i < 8; i++) out[(size_t)HEAD_SUM_AT + i] = (uint8_t)(sum >> (8 * i));
}

inline bool refuse(std::string &err, const char *fmt, long long a = 0, long long b = 0) {
    char buf[256];
    snprintf(buf, sizeof(buf), fmt, a, b);
    err = buf;
    return false;
}

// The structure of a blob of n bytes: magic, version, sizes, reserved bytes, the head checksum, the mirror's own length.  true, or false and
// one message per cause.  Ranges of the mirror's values: mirror_fault; agreement with an engine: config_mismatch
inline bool parse(const uint8_t *p, int64_t n, Header &h, Mirror &m, std::string &err) {
    if (!p || n < HEADER_BYTES) return refuse(err, "truncated: %lld bytes are no header (%lld)", n, HEADER_BYTES);
    Reader r{p};
    if (r.u32() != MAGIC) return refuse(err, "bad magic (not a stream snapshot)");
    const uint32_t version = r.u32();
    if (version != VERSION) return refuse(err, "format version %lld, this build reads version %lld", version, VERSION);
    h.total_bytes = r.u64();
    Config &c = h.cfg;
    for (uint32_t *v : {&c.dtype, &c.esz, &c.n_layers, &c.kernel_size, &c.kvc, &c.lctx, &c.mel_ring, &c.nmel, &c.abuf_cap, &c.hist_max, &c.tok_cap,
                        &c.token_logprobs, &c.alt_k, &c.frame_blank, &c.phrase_boost, &c.lm_fusion}) *v = r.u32();
    c.fp_weights = r.u64(); c.fp_boost = r.u64(); c.fp_lm = r.u64();
    h.mirror_bytes = r.u64(); h.device_bytes = r.u64(); h.device_sum = r.u64();
    const uint32_t reserved = r.u32();
    c.entropy_milli = r.u32();
    h.head_sum = r.u64();
    if (h.total_bytes > (uint64_t)n) return refuse(err, "truncated: %lld bytes of %lld", n, (long long)h.total_bytes);
    if (h.total_bytes < (uint64_t)n) return refuse(err, "trailing bytes: %lld bytes, the snapshot ends at %lld", n, (long long)h.total_bytes);
    const uint64_t most = (uint64_t)mirror_bytes((size_t)TOK_CAP);
    if (h.mirror_bytes < (uint64_t)MIRROR_FIXED || h.mirror_bytes > most || (h.mirror_bytes & 15)) return refuse(err, "mirror section of %lld bytes (at most %lld, in 16s)", (long long)h.mirror_bytes, (long long)most);
    if ((h.device_bytes & 15) || h.device_bytes > h.total_bytes || (uint64_t)HEADER_BYTES + h.mirror_bytes + h.device_bytes != h.total_bytes)
        return refuse(err, "section sizes do not add up to the total (%lld + mirror + device against %lld)", HEADER_BYTES, (long long)h.total_bytes);
    if (reserved) return refuse(err, "reserved header bytes are not zero");
    const uint64_t sum = checksum(p, HEAD_SUM_AT, 0) + checksum(p + HEADER_BYTES, (int64_t)h.mirror_bytes, (uint32_t)(HEADER_BYTES / 4));
    if (sum != h.head_sum) return refuse(err, "header / mirror checksum mismatch (the snapshot is corrupted)");
    r.p = p + HEADER_BYTES;
    visit_fields(m, [&](const char *, auto &v, long long, long long) { r.field(v); });
    const uint32_t n_queue = r.u32();
    if (n_queue > (uint32_t)TOK_CAP) return refuse(err, "tok_queue of %lld tokens is longer than the token ring (%lld)", n_queue, TOK_CAP);
    if ((uint64_t)mirror_bytes(n_queue) != h.mirror_bytes) return refuse(err, "tok_queue of %lld tokens does not fill a mirror section of %lld bytes", n_queue, (long long)h.mirror_bytes);
    m.tok_queue.resize(n_queue);
    for (uint32_t i = 0; i < n_queue; i++) m.tok_queue[i] = (int32_t)r.u32();
    for (const uint8_t *q = r.p; q < p + HEADER_BYTES + h.mirror_bytes; q++) if (*q) return refuse(err, "mirror padding is not zero");
    return true;
}

// a blob's configuration against the restoring engine's: the first field that differs, by name, with both values
inline bool config_mismatch(const Config &blob, const Config &eng, std::string &err) {
    const struct { const char *name; uint32_t a, b; } f32[] = {
        {"dtype", blob.dtype, eng.dtype}, {"element size", blob.esz, eng.esz}, {"n_layers", blob.n_layers, eng.n_layers}, {"kernel_size", blob.kernel_size, eng.kernel_size},
        {"KVC", blob.kvc, eng.kvc}, {"LCTX", blob.lctx, eng.lctx}, {"MEL_RING", blob.mel_ring, eng.mel_ring}, {"NMEL", blob.nmel, eng.nmel}, {"ABUF_CAP", blob.abuf_cap, eng.abuf_cap},
        {"HIST_MAX", blob.hist_max, eng.hist_max}, {"TOK_CAP", blob.tok_cap, eng.tok_cap},
        {"option token_logprobs", blob.token_logprobs, eng.token_logprobs}, {"option token_alternatives", blob.alt_k, eng.alt_k},
        {"option frame_blank_logprobs", blob.frame_blank, eng.frame_blank}, {"option phrase_boost", blob.phrase_boost, eng.phrase_boost},
        {"option lm_fusion", blob.lm_fusion, eng.lm_fusion}, {"option token_entropy", blob.entropy_milli, eng.entropy_milli}};
    for (const auto &f : f32)
        if (f.a != f.b) { refuse(err, (std::string(f.name) + " mismatch: the snapshot has %lld, the engine %lld").c_str(), f.a, f.b); return true; }
    const struct { const char *name; uint64_t a, b; } f64[] = {
        {"weight set", blob.fp_weights, eng.fp_weights}, {"boost set", blob.fp_boost, eng.fp_boost}, {"language model", blob.fp_lm, eng.fp_lm}};
    for (const auto &f : f64)
        if (f.a != f.b) { refuse(err, (std::string(f.name) + " mismatch: the snapshot's fingerprint is %016llx, the engine's %016llx").c_str(), (long long)f.a, (long long)f.b); return true; }
    return false;
}

// the audio format, by the rules of nasr_stream_set_audio_format; nullptr or the field that is wrong
inline const char *audio_format_fault(int sample_rate, int encoding, int channels, int channel) {
    nasr_rs::Plan p;
    if (!nasr_rs::make_plan(sample_rate, &p)) return "sample_rate";
    if (encoding < 0 || encoding > 3) return "encoding";
    if (channels < 1 || channels > nasr_rs::MAX_CHANNELS) return "channels";
    if (channel < -1 || channel >= channels) return "channel";
    return nullptr;
}

// every field of the mirror in its range; num_prompts: the restoring engine's.  true = a fault, named in err
inline bool mirror_fault(const Mirror &m, int num_prompts, std::string &err) {
    const auto out = [&](const char *name, long long v, long long lo, long long hi) {
        if (v >= lo && v <= hi) return false;
        char buf[200];
        snprintf(buf, sizeof(buf), "mirror field %s = %lld is outside %lld .. %lld", name, v, lo, hi);
        err = buf;
        return true;
    };
    if (m.R != 0 && m.R != 1 && m.R != 6 && m.R != 13) { refuse(err, "mirror field R = %lld is none of 0, 1, 6, 13", m.R); return true; }
    if (out("prompt", m.prompt, -1, num_prompts > 0 ? num_prompts - 1 : -1)) return true;
    bool bad = false;                              // the first field outside its range, in wire order
    visit_fields(m, [&](const char *name, auto v, long long lo, long long hi) { bad = bad || out(name, (long long)v, lo, hi); });
    if (bad) return true;
    if (const char *what = audio_format_fault(m.sample_rate, m.encoding, m.channels, m.channel)) {
        err = std::string("mirror audio format: unsupported ") + what;
        return true;
    }
    if (m.tok_queue.size() > (size_t)TOK_CAP) { refuse(err, "tok_queue of %lld tokens is longer than the token ring (%lld)", (long long)m.tok_queue.size(), TOK_CAP); return true; }
    return false;
}

// ---- the plan: the fork plan with a third address -------------------------------------------------------------------------------------
// The segments of slot `slot` that make up the stream described by m (fork_plan for src = dst = slot, so a later decode option lands here
// through dec_set_slot_layout as it does in a fork), each with its offset in the device section (Seg::blob): dense, in plan order, every
// segment padded to 16 bytes.  SAVE copies [src, src + bytes) of the slot to blob; RESTORE copies blob to [dst, dst + bytes).
inline std::vector<Seg> snapshot_plan(const Mirror &m, int slot, int esz, int n_layers, int kernel_size, DecodeSet &d, const DecFeatures &f, int64_t *section_bytes) {
    std::vector<Seg> segs = nasr_fork::fork_plan(live_part(m), slot, slot, esz, n_layers, kernel_size, d, f);
    int64_t at = 0;
    for (Seg &s : segs) { s.blob = at; at += pad16(s.bytes); }
    if (section_bytes) *section_bytes = at;
    return segs;
}
// the mirror with the most bytes to move (a full mel ring, a full audio buffer; the token queue at the ring's length is the mirror section's)
inline Mirror largest_mirror() {
    Mirror m;
    m.mel_count = MEL_RING; m.abuf_cnt = ABUF_CAP;
    return m;
}

// plan_fault's tests for a plan whose other side is the blob: every segment inside its own slot's part of its buffer and made of 16-byte
// vectors (word items: 4-byte words), the blob offsets 16-byte aligned, ascending, dense up to the padding, ending at section_bytes
inline const char *snapshot_plan_fault(const std::vector<Seg> &segs, int slot, int64_t section_bytes) {
    if (slot < 0) return "negative slot";
    int64_t at = 0;
    for (const Seg &s : segs) {
        if (const char *what = nasr_fork::seg_fault(s, s.src, slot, "slot range leaves its slot")) return what;
        if (s.dst != s.src) return "a snapshot segment has one slot side";
        if (s.blob != at) return "blob offsets are not dense";
        at += pad16(s.bytes);
    }
    return at == section_bytes ? nullptr : "device section size disagrees with the plan";
}

// the pieces of a pack (slot -> staging) or an unpack (staging -> slot) launch: Piece::pad carries the index of the piece's first word in the section
inline void cut_snapshot_pieces(std::vector<nasr_fork::Piece> &out, const Seg &s, char *slot_base, char *stage, int64_t piece_bytes, bool unpack) {
    for (int64_t at = 0; at < s.bytes; at += piece_bytes) {
        const int64_t n = s.bytes - at < piece_bytes ? s.bytes - at : piece_bytes;
        char *in_slot = slot_base + s.src + at, *in_blob = stage + s.blob + at;
        out.push_back(nasr_fork::Piece{unpack ? in_blob : in_slot, unpack ? in_slot : in_blob, (uint32_t)n, (uint32_t)((s.blob + at) / 4)});
    }
}

// ---- what the decoder's per-slot state holds that a kernel uses as an index WITHOUT masking: checked on the host, after the
// section's checksum has passed, on the bytes of the blob.  DecCtrl: cur picks one of the two LSTM state versions, prev_token a row of the
// embedding; a drained stream is not active, and t, n_frames, symbols, row and dirty are kept to what a decode leaves.  boost_state is a row
// of the automaton tables (n_boost_states rows).  n_tok, frame0 and frame_next are masked where they index a ring; lm_state and lm_next go
// through nasr_lm::lookup, which puts a state outside the model back to 0.  DecCtrl holds no pointer and no slot number (row is the batch row
// of the last step, rewritten by k_dec_begin), which is why a fork may copy it verbatim -- and a snapshot too.
// Also: the padding behind every segment is zero
inline bool device_fault(const uint8_t *section, const std::vector<Seg> &segs, const Mirror &m, int n_boost_states, std::string &err) {
    for (const Seg &s : segs) {
        for (int64_t i = s.bytes; i < pad16(s.bytes); i++)
            if (section[s.blob + i]) { err = std::string("device section: the padding behind '") + s.name + "' is not zero"; return true; }
        if (s.buf != nasr_fork::BUF_DEC) continue;
        if (!strcmp(s.name, "ctrl")) {
            DecCtrl c;
            if (s.bytes != (int64_t)sizeof(c)) { err = "device section: ctrl has another size"; return true; }
            memcpy(&c, section + s.blob, sizeof(c));
            const auto out = [&](const char *name, long long v, long long lo, long long hi) {
                if (v >= lo && v <= hi) return false;
                char buf[200];
                snprintf(buf, sizeof(buf), "decoder ctrl field %s = %lld is outside %lld .. %lld", name, v, lo, hi);
                err = buf;
                return true;
            };
            if (out("cur", c.cur, 0, 1) || out("prev_token", c.prev_token, 0, BLANK) || out("active", c.active, 0, 0) || out("dirty", c.dirty, 0, 1) ||
                out("n_frames", c.n_frames, 0, MAXNEW) || out("t", c.t, 0, c.n_frames) || out("symbols", c.symbols, 0, MAX_SYMBOLS - 1) ||
                out("row", c.row, 0, 65535) || out("n_tok", c.n_tok, m.tok_read, (long long)m.tok_read + TOK_CAP) || out("iterations", c.iterations, 0, INT32_MAX) ||
                out("frame0", c.frame0, 0, INT32_MAX) || out("frame_next", c.frame_next, c.frame0, INT32_MAX))
                return true;
        } else if (!strcmp(s.name, "boost_state")) {
            int32_t st;
            memcpy(&st, section + s.blob, 4);
            if (st < 0 || st >= n_boost_states) { refuse(err, "decoder boost_state = %lld is no state of the boost set in force (%lld states)", st, n_boost_states); return true; }
        }
    }
    return false;
}

}  // namespace nasr_snap
