// wav_header.h -- RIFF/WAVE header parser of the command-line tools: pure (no I/O, no allocation) and bounds-checked, so the CPU suite
// runs it over a corpus of damaged headers under AddressSanitizer (tests/test_resample_math.py).  It finds the `fmt ` and `data` chunks in
// the first n bytes of a file and names the audio format in the engine's terms (nasr_audio_format, include/nemotron_asr_amd.h).
// Accepted: PCM 16-bit (tag 1), IEEE float 32-bit (tag 3), A-law (tag 6) and mu-law (tag 7) at 8 bits, also inside WAVE_FORMAT_EXTENSIBLE
// (tag 0xFFFE: the first two bytes of the sub-format GUID); anything else is an error that names the format tag.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace wav_header {

enum { OK = 0, NOT_WAV = 1, ERR_TRUNCATED = -1, ERR_NO_FMT = -2, ERR_NO_DATA = -3, ERR_FORMAT = -4 };
enum { ENC_S16 = 0, ENC_F32 = 1, ENC_MULAW = 2, ENC_ALAW = 3 };      // = NASR_AUDIO_*

struct Info {
    int format_tag, channels, sample_rate, bits, encoding;
    size_t data_offset;       // of the first sample, <= n
    uint32_t data_bytes;      // as the header declares it (0 or 0xFFFFFFFF from a writer that could not seek back: read to the end of the file)
};

inline uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// OK: *out is filled.  NOT_WAV: the bytes do not start with RIFF....WAVE (raw audio).  < 0: a WAVE file this tool cannot read, err says why.
inline int parse(const uint8_t *buf, size_t n, Info *out, char *err, size_t err_cap) {
    if (err && err_cap) err[0] = 0;
    if (!buf || !out || n < 12 || memcmp(buf, "RIFF", 4) != 0 || memcmp(buf + 8, "WAVE", 4) != 0) return NOT_WAV;
    memset(out, 0, sizeof(*out));
    bool have_fmt = false;
    size_t pos = 12;
    while (n - pos >= 8) {                                   // pos <= n always
        const uint32_t size = rd32(buf + pos + 4);
        const size_t body = pos + 8, left = n - body;
        if (!memcmp(buf + pos, "fmt ", 4)) {
            if (size < 16 || left < 16) { if (err) snprintf(err, err_cap, "WAVE: the fmt chunk is cut short"); return ERR_TRUNCATED; }
            int tag = (int)rd16(buf + body);
            out->channels = (int)rd16(buf + body + 2);
            out->sample_rate = (int)rd32(buf + body + 4);
            out->bits = (int)rd16(buf + body + 14);
            if (tag == 0xFFFE) {                                 // extensible: the real tag opens the sub-format GUID
                if (size < 40 || left < 40) { if (err) snprintf(err, err_cap, "WAVE: the extensible fmt chunk is cut short"); return ERR_TRUNCATED; }
                tag = (int)rd16(buf + body + 24);
            }
            out->format_tag = tag;
            if (tag == 1 && out->bits == 16) out->encoding = ENC_S16;
            else if (tag == 3 && out->bits == 32) out->encoding = ENC_F32;
            else if (tag == 7 && out->bits == 8) out->encoding = ENC_MULAW;
            else if (tag == 6 && out->bits == 8) out->encoding = ENC_ALAW;
            else {
                if (err) snprintf(err, err_cap, "WAVE: unsupported format tag %d at %d bits (PCM 16, IEEE float 32, mu-law and A-law are read)", tag, out->bits);
                return ERR_FORMAT;
            }
            if (out->channels < 1 || out->channels > 8 || out->sample_rate <= 0) {
                if (err) snprintf(err, err_cap, "WAVE: format tag %d with %d channel(s) at %d Hz", tag, out->channels, out->sample_rate);
                return ERR_FORMAT;
            }
            have_fmt = true;
        } else if (!memcmp(buf + pos, "data", 4)) {
            if (!have_fmt) { if (err) snprintf(err, err_cap, "WAVE: data chunk without a fmt chunk before it"); return ERR_NO_FMT; }
            out->data_offset = body;
            out->data_bytes = size;
            return OK;
        }
        const size_t skip = (size_t)size + (size & 1u);          // chunks are padded to even sizes
        if (skip > left) break;                                  // the chunk runs past the bytes we have
        pos = body + skip;
    }
    if (err) snprintf(err, err_cap, have_fmt ? "WAVE: no data chunk" : "WAVE: no fmt chunk");
    return have_fmt ? ERR_NO_DATA : ERR_NO_FMT;
}

}  // namespace wav_header
