// stream_envelope.h -- what nemo_stream_save puts around the engine's snapshot blob (nasr_stream_save): the parts of a nemo_stream_context
// that nemo_stream_fork carries beside the engine stream -- transcript, tokens, language prompt, audio format, endpoint detector state and
// events, the counters.  Little-endian, version 1: magic "NASE", version, then the fields in the order of struct Envelope; a byte string is a
// 64-bit length and its bytes, a list a 64-bit count and its entries.  Every length is checked against what is left of the buffer before
// anything is read or allocated, and nothing may follow the last field.  Pure: no engine, no HIP (fuzzed on a CPU under sanitizers with the
// snapshot parser, tests/test_snapshot_format.py).  Like the blob inside it the envelope is integrity-checked by its lengths only, not authenticated.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace nemo_env {

constexpr uint32_t MAGIC = 0x4553414Eu, VERSION = 1;        // "NASE"

struct Event { int64_t frame = 0, utt_start = 0; int32_t rule = 0, tokens = 0; };
struct Envelope {
    std::vector<uint8_t> engine_blob;
    std::string transcript;
    std::vector<int32_t> tokens;
    int32_t right_context = 0, prompt_index = -1;
    int32_t audio_rate = 16000, audio_encoding = 0, audio_channels = 1, audio_channel = 0;
    // the endpoint detector: on / off, its configuration (the threshold as the bits of a float), its state, what it has consumed, its events
    uint32_t ep_on = 0, ep_min_blank_bits = 0;
    int32_t ep_idle = 0, ep_after_speech = 0, ep_max_utterance = 0;
    int64_t ep_utt_start = 0;
    int32_t ep_state_tokens = 0, ep_trailing = 0;
    int64_t ep_frames = 0, ep_tokens = 0;
    std::vector<Event> ep_events;
    uint64_t audio_seconds_bits = 0;                         // total_audio_seconds as the bits of a double
    int32_t chunks_processed = 0;
};

struct Writer {
    std::vector<uint8_t> &out;
    void u32(uint32_t v) { for (int i = 0; i < 4; i++) out.push_back((uint8_t)(v >> (8 * i))); }
    void u64(uint64_t v) { for (int i = 0; i < 8; i++) out.push_back((uint8_t)(v >> (8 * i))); }
    void bytes(const void *p, size_t n) { u64(n); const uint8_t *b = (const uint8_t *)p; out.insert(out.end(), b, b + n); }
};

inline void write(const Envelope &e, std::vector<uint8_t> &out) {
    out.clear();
    Writer w{out};
    w.u32(MAGIC); w.u32(VERSION);
    w.bytes(e.engine_blob.data(), e.engine_blob.size());
    w.bytes(e.transcript.data(), e.transcript.size());
    w.u64(e.tokens.size());
    for (int32_t t : e.tokens) w.u32((uint32_t)t);
    for (int32_t v : {e.right_context, e.prompt_index, e.audio_rate, e.audio_encoding, e.audio_channels, e.audio_channel}) w.u32((uint32_t)v);
    w.u32(e.ep_on); w.u32(e.ep_min_blank_bits);
    for (int32_t v : {e.ep_idle, e.ep_after_speech, e.ep_max_utterance}) w.u32((uint32_t)v);
    w.u64((uint64_t)e.ep_utt_start); w.u32((uint32_t)e.ep_state_tokens); w.u32((uint32_t)e.ep_trailing);
    w.u64((uint64_t)e.ep_frames); w.u64((uint64_t)e.ep_tokens);
    w.u64(e.ep_events.size());
    for (const Event &ev : e.ep_events) { w.u64((uint64_t)ev.frame); w.u64((uint64_t)ev.utt_start); w.u32((uint32_t)ev.rule); w.u32((uint32_t)ev.tokens); }
    w.u64(e.audio_seconds_bits); w.u32((uint32_t)e.chunks_processed);
}

// true, or false and what is wrong
inline bool parse(const uint8_t *p, int64_t n, Envelope &e, std::string &err) {
    if (!p || n < 8) { err = "envelope truncated: no magic and version"; return false; }
    const uint8_t *end = p + n;
    const auto left = [&]() { return (uint64_t)(end - p); };
    const auto u32 = [&]() { uint32_t v = 0; for (int i = 0; i < 4; i++) v |= (uint32_t)p[i] << (8 * i); p += 4; return v; };
    const auto u64 = [&]() { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i); p += 8; return v; };
    const auto need = [&](uint64_t k, const char *what) { if (left() >= k) return true; err = std::string("envelope truncated in ") + what; return false; };
    const auto count = [&](uint64_t unit, uint64_t *k, const char *what) {           // a length or count whose entries must still be there
        if (!need(8, what)) return false;
        *k = u64();
        if (*k > left() / unit) { err = std::string("envelope field ") + what + " is longer than what is left"; return false; }
        return true;
    };
    if (u32() != MAGIC) { err = "bad envelope magic (not a saved stream)"; return false; }
    if (u32() != VERSION) { err = "envelope version is not 1"; return false; }
    uint64_t k;
    if (!count(1, &k, "engine blob")) return false;
    e.engine_blob.assign(p, p + k); p += k;
    if (!count(1, &k, "transcript")) return false;
    e.transcript.assign((const char *)p, (size_t)k); p += k;
    if (!count(4, &k, "tokens")) return false;
    e.tokens.resize((size_t)k);
    for (uint64_t i = 0; i < k; i++) e.tokens[(size_t)i] = (int32_t)u32();
    if (!need(6 * 4 + 2 * 4 + 3 * 4 + 8 + 4 + 4 + 8 + 8, "the fixed fields")) return false;
    for (int32_t *v : {&e.right_context, &e.prompt_index, &e.audio_rate, &e.audio_encoding, &e.audio_channels, &e.audio_channel}) *v = (int32_t)u32();
    e.ep_on = u32(); e.ep_min_blank_bits = u32();
    for (int32_t *v : {&e.ep_idle, &e.ep_after_speech, &e.ep_max_utterance}) *v = (int32_t)u32();
    e.ep_utt_start = (int64_t)u64(); e.ep_state_tokens = (int32_t)u32(); e.ep_trailing = (int32_t)u32();
    e.ep_frames = (int64_t)u64(); e.ep_tokens = (int64_t)u64();
    if (e.ep_on > 1) { err = "envelope field ep_on is neither 0 nor 1"; return false; }
    if (!count(24, &k, "endpoint events")) return false;
    e.ep_events.resize((size_t)k);
    for (uint64_t i = 0; i < k; i++) { Event &ev = e.ep_events[(size_t)i]; ev.frame = (int64_t)u64(); ev.utt_start = (int64_t)u64(); ev.rule = (int32_t)u32(); ev.tokens = (int32_t)u32(); }
    if (!need(12, "the counters")) return false;
    e.audio_seconds_bits = u64(); e.chunks_processed = (int32_t)u32();
    if (p != end) { err = "envelope has trailing bytes"; return false; }
    return true;
}

}  // namespace nemo_env
