"""The blob of a stream snapshot (nemotron-asr.cpp_amd/csrc/nasr_snapshot.h: format, parser, checksum, the save / restore plan) and the
envelope host/nemo_amd puts around it (host/stream_envelope.h).  No GPU: the headers are compiled with the host compiler under
AddressSanitizer and UBSan into a stand-alone program, like tests/test_fork_plan.py; nothing is loaded into Python.

The format is restated here, not read from the header: little-endian; a 144-byte header -- magic "NASS", version 1, total size (u64), then
sixteen u32: dtype, element size, n_layers, kernel_size, KVC 326, LCTX 70, MEL_RING 4096, NMEL 128, ABUF_CAP 328256, HIST_MAX 193, TOK_CAP
4096, token_logprobs, token_alternatives K, frame_blank_logprobs, phrase_boost, lm_fusion; three u64 fingerprints (weights, boost set, LM);
u64 mirror bytes, device bytes, device checksum, 8 reserved bytes, u64 head checksum -- then the mirror: eleven i32 (R, prompt, abuf_cnt,
abuf_par, mel_start, mel_count, valid_len, kv_head, cc_par, chunks, tok_read), i64 samples_in, u32 boost and LM enable, four i32 of audio
format, i64 aud_in, i64 aud_out, i32 aud_par, u32 queue length, the queued tokens, zeros up to 16 bytes -- then the device section: the fork
plan's segments in plan order, each zero-padded to 16 bytes.  Checksum of words w_i at word index i: sum of fmix32(w_i ^ i * 0x9E3779B1) mod
2^64; the head checksum runs over the header without its last 8 bytes and the mirror (word indices from 0 and from 36)."""
import itertools
import re
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

from tests.test_fork_plan import ALL, COMBOS, KV_HEADS, MELS
from tests.test_gemm_plan import HIP_STUB

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"
HOST = ROOT / "nemotron-asr.cpp_amd" / "host"

DRIVER = r"""
#include "nasr_internal.h"
#include "nasr_decode_set.h"
#include "nasr_fork_plan.h"
#include "nasr_snapshot.h"
#include "stream_envelope.h"
#include <cstdio>
#include <cstdlib>
using namespace nasr;
using nasr_fork::Seg;
// one command per line of stdin, one answer per line of stdout
//   P kv_head mel_start mel_count abuf_cnt abuf_par esz n_layers ks slot other_slot <5 features>
//         "<buf:layer:name:slot offset:bytes:slot_bytes:blob of the snapshot plan> | <the same of the fork plan slot -> other_slot, blob 0> | <snapshot_plan_fault or ok> |
//          <section bytes> <pack pieces> <bytes in them> <largest> <unpack pieces into other_slot that are not the pack pieces with the two sides exchanged> <snapshot_plan_fault with the section one vector short>"
//   S <25 mirror values: R prompt abuf_cnt abuf_par mel_start mel_count valid_len kv_head cc_par chunks tok_read samples_in boost lm rate enc channels channel aud_in aud_out aud_par n_queue>
//     dtype esz n_layers ks <5 features> num_prompts boost_states     sets the BASE blob (a valid one for an engine of that configuration); "<bytes> <hex of header and mirror>"
//   V fix newlen n (offset value)*      the base blob with n bytes set, cut or zero-extended to newlen (-1: as it is), fix = 1: the head checksum (2: the device checksum too) put right afterwards;
//                                        through every host check of a restore: "refused: <message>" or "accepted same" / "accepted DIFFERENT" (re-serialised against the input)
//   G field delta                        the base blob against an engine whose configuration field (0 .. 18) is larger by delta
//   C                                    the checksum's properties: "<pieces ok> <flips that did not change the sum of 2048>"
//   F seed count                         count deterministic mutations of the base blob (bit flips, truncations, splices, with and without the checksums put right): "<refused> <accepted same> <accepted DIFFERENT>"
//   E seed count                         the same for an envelope around the head of the base blob
//   R keep <the 22 mirror values of S>   the record (n_queue tokens queued) after reset_state(keep): "<its 22 values>"
//   D                                    a default record after the fresh reset: "<its 22 values>"
//   M <the 22 mirror values of S>        the field table: "<bytes of the visitor's fields, 4 per 32-bit and 8 per 64-bit one, plus the queue-length word> <fields visited>
//                                        <1: write, parse, write gave the same bytes and parse gave the same fields> <hex of header and mirror>"
struct Base {
    std::vector<uint8_t> blob;
    nasr_snap::Config cfg;
    int num_prompts = 0, boost_states = 0;
} g;
static unsigned long long g_rng = 1;
static unsigned rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_rng >> 33); }

static bool read_features(DecFeatures &f) {
    int lp, k, fb, pb, lm;
    if (scanf("%d %d %d %d %d", &lp, &k, &fb, &pb, &lm) != 5) return false;
    f.token_logprobs = lp; f.alt_k = k; f.frame_blank = fb; f.phrase_boost = pb; f.lm_fusion = lm;
    return true;
}
static void put64(std::vector<uint8_t> &b, size_t at, unsigned long long v) { for (int i = 0; i < 8; i++) b[at + i] = (uint8_t)(v >> (8 * i)); }
static unsigned long long get64(const std::vector<uint8_t> &b, size_t at) { unsigned long long v = 0; for (int i = 0; i < 8; i++) v |= (unsigned long long)b[at + i] << (8 * i); return v; }
static void fix_sums(std::vector<uint8_t> &b, bool device) {
    if ((int64_t)b.size() < nasr_snap::HEADER_BYTES) return;
    const unsigned long long mb = get64(b, 104), db = get64(b, 112);
    if (mb > b.size() || db > b.size() || nasr_snap::HEADER_BYTES + mb + db > b.size() || (mb & 3) || (db & 3)) return;
    if (device) put64(b, 120, nasr_snap::checksum(b.data() + nasr_snap::HEADER_BYTES + mb, (int64_t)db, 0));
    put64(b, 136, nasr_snap::checksum(b.data(), 136, 0) + nasr_snap::checksum(b.data() + nasr_snap::HEADER_BYTES, (int64_t)mb, 36));
}
// every host check of nasr_stream_restore, with the host's checksum of the device section in the place of k_stream_unpack's; "" = accepted
static std::string validate(const std::vector<uint8_t> &b, const nasr_snap::Config &eng, bool *same) {
    nasr_snap::Header h;
    nasr_snap::Mirror m;
    std::string err;
    if (!nasr_snap::parse(b.data(), (int64_t)b.size(), h, m, err)) return err;
    if (nasr_snap::config_mismatch(h.cfg, eng, err)) return err;
    if (nasr_snap::mirror_fault(m, g.num_prompts, err)) return err;
    DecodeSet d;
    int64_t section = 0;
    const std::vector<Seg> segs = nasr_snap::snapshot_plan(m, 2, (int)eng.esz, (int)eng.n_layers, (int)eng.kernel_size, d, nasr_snap::features_of(eng), &section);
    if ((unsigned long long)section != h.device_bytes) return "device section size disagrees with the plan for this mirror";
    if (const char *what = nasr_snap::snapshot_plan_fault(segs, 2, section)) return what;
    const uint8_t *payload = b.data() + nasr_snap::HEADER_BYTES + h.mirror_bytes;
    if (nasr_snap::checksum(payload, section, 0) != h.device_sum) return "device section checksum mismatch";
    if (nasr_snap::device_fault(payload, segs, m, g.boost_states, err)) return err;
    std::vector<uint8_t> again;
    nasr_snap::Header h2;
    h2.cfg = h.cfg; h2.device_bytes = h.device_bytes; h2.device_sum = h.device_sum;
    nasr_snap::write_head(h2, m, again);
    *same = again.size() == (size_t)(nasr_snap::HEADER_BYTES + h.mirror_bytes) && !memcmp(again.data(), b.data(), again.size());
    return "";
}
static bool read_mirror(nasr_snap::Mirror &m) {
    long long si, ai, ao;
    unsigned be, le, nq;
    if (scanf("%d %d %d %d %d %d %d %d %d %d %d %lld %u %u %d %d %d %d %lld %lld %d %u", &m.R, &m.prompt, &m.abuf_cnt, &m.abuf_par, &m.mel_start, &m.mel_count, &m.valid_len, &m.kv_head,
              &m.cc_par, &m.chunks, &m.tok_read, &si, &be, &le, &m.sample_rate, &m.encoding, &m.channels, &m.channel, &ai, &ao, &m.aud_par, &nq) != 22) return false;
    m.samples_in = si; m.aud_in = ai; m.aud_out = ao; m.boost_enabled = be; m.lm_enabled = le;
    for (unsigned i = 0; i < nq; i++) m.tok_queue.push_back((int32_t)(i * 7 % 1024));
    return true;
}
static void print_mirror(const nasr_snap::Mirror &m) {
    printf("%d %d %d %d %d %d %d %d %d %d %d %lld %u %u %d %d %d %d %lld %lld %d %zu\n", m.R, m.prompt, m.abuf_cnt, m.abuf_par, m.mel_start, m.mel_count, m.valid_len, m.kv_head, m.cc_par, m.chunks,
           m.tok_read, (long long)m.samples_in, m.boost_enabled, m.lm_enabled, m.sample_rate, m.encoding, m.channels, m.channel, (long long)m.aud_in, (long long)m.aud_out, m.aud_par, m.tok_queue.size());
}
static nasr_snap::Config bumped(nasr_snap::Config c, int field, int delta) {
    uint32_t *f32[] = {&c.dtype, &c.esz, &c.n_layers, &c.kernel_size, &c.kvc, &c.lctx, &c.mel_ring, &c.nmel, &c.abuf_cap, &c.hist_max, &c.tok_cap,
                       &c.token_logprobs, &c.alt_k, &c.frame_blank, &c.phrase_boost, &c.lm_fusion};
    uint64_t *f64[] = {&c.fp_weights, &c.fp_boost, &c.fp_lm};
    if (field < 16) *f32[field] += (uint32_t)delta; else *f64[field - 16] += (uint64_t)delta;
    return c;
}

int main() {
    char op;
    while (scanf(" %c", &op) == 1) {
        if (op == 'P') {
            nasr_snap::Mirror m;
            int esz, n_layers, ks, slot, other;
            DecFeatures f;
            if (scanf("%d %d %d %d %d %d %d %d %d %d", &m.kv_head, &m.mel_start, &m.mel_count, &m.abuf_cnt, &m.abuf_par, &esz, &n_layers, &ks, &slot, &other) != 10 || !read_features(f)) return 2;
            DecodeSet d;
            int64_t section = 0, section2 = 0;
            const std::vector<Seg> segs = nasr_snap::snapshot_plan(m, slot, esz, n_layers, ks, d, f, &section);
            for (const Seg &s : segs) printf("%d:%d:%s:%lld:%lld:%lld:%lld ", s.buf, s.layer, s.name, (long long)s.src, (long long)s.bytes, (long long)s.slot_bytes, (long long)s.blob);
            printf("| ");
            const nasr_fork::Source live = {m.kv_head, m.mel_start, m.mel_count, m.abuf_cnt, m.abuf_par};
            for (const Seg &s : nasr_fork::fork_plan(live, slot, other, esz, n_layers, ks, d, f)) printf("%d:%d:%s:%lld:%lld:%lld:%lld ", s.buf, s.layer, s.name, (long long)s.src, (long long)s.bytes, (long long)s.slot_bytes, (long long)s.blob);
            const char *fault = nasr_snap::snapshot_plan_fault(segs, slot, section);
            const std::vector<Seg> segs2 = nasr_snap::snapshot_plan(m, other, esz, n_layers, ks, d, f, &section2);
            long long n_pack = 0, total = 0, largest = 0, odd = segs2.size() != segs.size() || section2 != section;
            for (size_t i = 0; i < segs.size() && !odd; i++) {
                std::vector<nasr_fork::Piece> pack, unpack;
                nasr_snap::cut_snapshot_pieces(pack, segs[i], nullptr, nullptr, nasr_fork::PIECE_BYTES, false);
                nasr_snap::cut_snapshot_pieces(unpack, segs2[i], nullptr, nullptr, nasr_fork::PIECE_BYTES, true);
                if (pack.size() != unpack.size()) { odd++; continue; }
                const long long shift = (long long)(other - slot) * segs[i].slot_bytes;
                for (size_t k = 0; k < pack.size(); k++) {
                    n_pack++; total += pack[k].bytes;
                    if (pack[k].bytes > largest) largest = pack[k].bytes;
                    // the blob side is the same place, the slot side the same place of the other slot; the word index is the blob offset in words
                    if (unpack[k].src != pack[k].dst || (long long)(intptr_t)unpack[k].dst != (long long)(intptr_t)pack[k].src + shift || unpack[k].bytes != pack[k].bytes ||
                        unpack[k].pad != pack[k].pad || (long long)pack[k].pad * 4 != (long long)(intptr_t)pack[k].dst) odd++;
                }
            }
            const char *short_fault = nasr_snap::snapshot_plan_fault(segs, slot, section - 16);
            printf("| %s | %lld %lld %lld %lld %lld %s\n", fault ? fault : "ok", (long long)section, n_pack, total, largest, odd, short_fault ? "refused" : "ok");
        } else if (op == 'S') {
            nasr_snap::Mirror m;
            int dtype, esz, n_layers, ks;
            DecFeatures f;
            if (!read_mirror(m)) return 2;
            if (scanf("%d %d %d %d", &dtype, &esz, &n_layers, &ks) != 4 || !read_features(f) || scanf("%d %d", &g.num_prompts, &g.boost_states) != 2) return 2;
            g.cfg = nasr_snap::make_config(dtype, esz, n_layers, ks, f, 0x1111222233334444ull, f.phrase_boost ? 0x5555666677778888ull : 0, f.lm_fusion ? 0x9999aaaabbbbccccull : 0);
            DecodeSet d;
            int64_t section = 0;
            const std::vector<Seg> segs = nasr_snap::snapshot_plan(m, 0, esz, n_layers, ks, d, f, &section);
            std::vector<uint8_t> payload((size_t)section, 0);
            for (const Seg &s : segs) {                         // any bytes; the decoder's control block and boost state as a drained stream leaves them
                for (int64_t i = 0; i < s.bytes; i++) payload[(size_t)(s.blob + i)] = (uint8_t)(rnd() >> 8);
                if (!strcmp(s.name, "ctrl")) {
                    DecCtrl c = {};
                    c.t = 3; c.n_frames = 3; c.prev_token = 17; c.cur = 1; c.n_tok = m.tok_read + 2; c.iterations = 40; c.row = 0; c.dirty = 1; c.frame0 = 100; c.frame_next = 103;
                    memcpy(payload.data() + s.blob, &c, sizeof(c));
                }
                if (!strcmp(s.name, "boost_state")) { const int32_t st = g.boost_states - 1; memcpy(payload.data() + s.blob, &st, 4); }
            }
            nasr_snap::Header h;
            h.cfg = g.cfg; h.device_bytes = (uint64_t)section; h.device_sum = nasr_snap::checksum(payload.data(), section, 0);
            nasr_snap::write_head(h, m, g.blob);
            const size_t head = g.blob.size();
            g.blob.insert(g.blob.end(), payload.begin(), payload.end());
            printf("%zu ", g.blob.size());
            for (size_t i = 0; i < head; i++) printf("%02x", g.blob[i]);
            printf("\n");
        } else if (op == 'V') {
            int fix, n;
            long long newlen;
            if (scanf("%d %lld %d", &fix, &newlen, &n) != 3) return 2;
            std::vector<uint8_t> b = g.blob;
            for (int i = 0; i < n; i++) {
                long long off; int val;
                if (scanf("%lld %d", &off, &val) != 2) return 2;
                if (off >= 0 && off < (long long)b.size()) b[(size_t)off] = (uint8_t)val;
            }
            if (newlen >= 0) b.resize((size_t)newlen, 0);
            if (fix) fix_sums(b, fix == 2);
            bool same = false;
            const std::string err = validate(b, g.cfg, &same);
            if (err.empty()) printf("accepted %s\n", same ? "same" : "DIFFERENT"); else printf("refused: %s\n", err.c_str());
        } else if (op == 'G') {
            int field, delta;
            if (scanf("%d %d", &field, &delta) != 2) return 2;
            bool same = false;
            const std::string err = validate(g.blob, bumped(g.cfg, field, delta), &same);
            if (err.empty()) printf("accepted %s\n", same ? "same" : "DIFFERENT"); else printf("refused: %s\n", err.c_str());
        } else if (op == 'C') {
            int pieces_ok = 1;
            for (size_t size : {(size_t)4, (size_t)16, (size_t)20, (size_t)(262144 + 16), (size_t)100004}) {
                std::vector<uint8_t> buf(size);
                for (auto &v : buf) v = (uint8_t)(rnd() >> 8);
                const uint64_t whole = nasr_snap::checksum(buf.data(), (int64_t)size, 5);
                // halves, 256 KiB pieces, and an odd cut of 4-byte, 12-byte and 1 000-byte pieces; every piece with its global word offset
                for (const std::vector<size_t> &cut : {std::vector<size_t>{size >= 8 ? size / 8 * 4 : 4}, std::vector<size_t>{262144}, std::vector<size_t>{4, 12, 1000, 36}}) {
                    uint64_t sum = 0;
                    size_t at = 0, k = 0;
                    while (at < size) { const size_t n = std::min(cut[k++ % cut.size()], size - at); if (!n) break; sum += nasr_snap::checksum(buf.data() + at, (int64_t)n, 5 + (uint32_t)(at / 4)); at += n; }
                    if (at != size || sum != whole) pieces_ok = 0;
                }
                if (size >= 8) {                               // position-sensitive: two different words exchanged
                    std::vector<uint8_t> sw = buf;
                    if (memcmp(sw.data(), sw.data() + 4, 4)) { for (int i = 0; i < 4; i++) std::swap(sw[i], sw[4 + i]); if (nasr_snap::checksum(sw.data(), (int64_t)size, 5) == whole) pieces_ok = 0; }
                }
            }
            std::vector<uint8_t> buf(256);
            for (auto &v : buf) v = (uint8_t)(rnd() >> 8);
            const uint64_t whole = nasr_snap::checksum(buf.data(), 256, 0);
            int unchanged = 0;
            for (int bit = 0; bit < 2048; bit++) { buf[bit / 8] ^= (uint8_t)(1 << (bit % 8)); if (nasr_snap::checksum(buf.data(), 256, 0) == whole) unchanged++; buf[bit / 8] ^= (uint8_t)(1 << (bit % 8)); }
            printf("%d %d\n", pieces_ok, unchanged);
        } else if (op == 'F' || op == 'E') {
            unsigned long long seed; int count;
            if (scanf("%llu %d", &seed, &count) != 2) return 2;
            g_rng = seed;
            std::vector<uint8_t> base = g.blob;
            const size_t head = (size_t)(nasr_snap::HEADER_BYTES + (long long)get64(g.blob, 104));
            if (op == 'E') {
                nemo_env::Envelope e;
                e.engine_blob.assign(g.blob.begin(), g.blob.begin() + (long)head);
                e.transcript = " hello wor"; e.tokens = {5, 6, 7, 1023}; e.right_context = 13; e.prompt_index = 3; e.ep_on = 1; e.ep_idle = 30; e.ep_frames = 77;
                e.ep_events.push_back(nemo_env::Event{40, 2, 2, 3});
                e.ep_events.push_back(nemo_env::Event{90, 41, 1, 0});
                nemo_env::write(e, base);
            }
            const size_t hot = op == 'E' ? base.size() : head;      // where the structure is: most mutations land there
            int refused = 0, accepted = 0, different = 0;
            for (int it = 0; it < count; it++) {
                std::vector<uint8_t> b = base;
                const unsigned kind = rnd() % 6;
                if (kind <= 1) { const int n = 1 + (int)(rnd() % 3); for (int i = 0; i < n; i++) { const size_t at = rnd() % (kind ? hot : b.size()); b[at] ^= (uint8_t)(1u << (rnd() % 8)); } }
                else if (kind == 2) b.resize(rnd() % (rnd() % 2 ? hot + 1 : b.size() + 1));                          // truncation
                else if (kind == 3) b.resize(b.size() + 1 + rnd() % 64, (uint8_t)rnd());                           // trailing bytes
                else if (kind == 4) { const size_t at = rnd() % (hot - 8) / 4 * 4; const unsigned v = rnd() % 3 == 0 ? 0xffffffffu : rnd() % 3 == 1 ? 0x7fffffffu : rnd(); for (int i = 0; i < 4; i++) b[at + i] = (uint8_t)(v >> (8 * i)); }      // a field spliced in
                else { const size_t a = rnd() % (hot - 16), c = rnd() % (hot - 16); for (int i = 0; i < 16; i++) b[a + i] = base[c + i]; }                                // 16 bytes from elsewhere
                bool same = false;
                std::string err;
                if (op == 'F') {
                    if (rnd() % 2) fix_sums(b, rnd() % 2);              // half of them with the checksums put right: the range checks get their turn
                    err = validate(b, g.cfg, &same);
                } else {
                    nemo_env::Envelope e;
                    if (nemo_env::parse(b.data(), (int64_t)b.size(), e, err)) {
                        std::vector<uint8_t> again;
                        nemo_env::write(e, again);
                        same = again == b;
                        // ... and what it carries goes through the engine's parser
                        nasr_snap::Header h; nasr_snap::Mirror m; std::string err2;
                        (void)nasr_snap::parse(e.engine_blob.data(), (int64_t)e.engine_blob.size(), h, m, err2);
                    } else if (err.empty()) err = "refused without a message";
                }
                if (!err.empty()) refused++; else if (same) accepted++; else different++;
            }
            printf("%d %d %d\n", refused, accepted, different);
        } else if (op == 'R' || op == 'D') {
            nasr_snap::Mirror m;
            int keep = 0;
            if (op == 'R' && (scanf("%d", &keep) != 1 || !read_mirror(m))) return 2;
            nasr_snap::reset_state(m, keep != 0);
            print_mirror(m);
        } else if (op == 'M') {
            nasr_snap::Mirror m, back;
            if (!read_mirror(m)) return 2;
            long long bytes = 4, fields = 0;                    // the queue-length word
            nasr_snap::visit_fields(m, [&](const char *, auto &v, long long, long long) { static_assert(sizeof(v) == 4 || sizeof(v) == 8, "a 32- or 64-bit field"); bytes += sizeof(v); fields++; });
            nasr_snap::Header h, h2;
            std::vector<uint8_t> first, again;
            std::string err;
            nasr_snap::write_head(h, m, first);
            int same = nasr_snap::parse(first.data(), (int64_t)first.size(), h2, back, err) ? 1 : 0;
            std::vector<long long> a, b;
            nasr_snap::visit_fields(m, [&](const char *, auto &v, long long, long long) { a.push_back((long long)v); });
            nasr_snap::visit_fields(back, [&](const char *, auto &v, long long, long long) { b.push_back((long long)v); });
            h2.device_bytes = 0; h2.device_sum = 0;
            nasr_snap::write_head(h2, back, again);
            if (a != b || back.tok_queue != m.tok_queue || again != first) same = 0;
            printf("%lld %lld %d ", bytes, fields, same);
            for (uint8_t v : first) printf("%02x", v);
            printf("\n");
        } else return 2;
    }
    return 0;
}
"""

KVC, LCTX, MEL_RING, NMEL, ABUF_CAP, HIST_MAX, TOK_CAP = 326, 70, 4096, 128, 1280 * 256 + 512 + 64, 193, 4096
HEADER_BYTES = 144
MIRROR_NAMES = ("R", "prompt", "abuf_cnt", "abuf_par", "mel_start", "mel_count", "valid_len", "kv_head", "cc_par", "chunks", "tok_read", "samples_in", "boost_enabled", "lm_enabled",
                "sample_rate", "encoding", "channels", "channel", "aud_in", "aud_out", "aud_par", "n_queue")
MIRROR_FMT = "<11iqII4iqqiI"
BASE_MIRROR = dict(R=13, prompt=3, abuf_cnt=7777, abuf_par=1, mel_start=4090, mel_count=57, valid_len=70, kv_head=300, cc_par=1, chunks=41, tok_read=9, samples_in=918273645, boost_enabled=1,
                   lm_enabled=0, sample_rate=44100, encoding=1, channels=2, channel=-1, aud_in=2530000, aud_out=918000, aud_par=1, n_queue=5)
BASE_ENGINE = dict(dtype=1, esz=2, n_layers=2, ks=9, features=ALL, num_prompts=8, boost_states=6)


def fmix32(h):
    h ^= h >> 16
    h = h * 0x85EBCA6B & 0xFFFFFFFF
    h ^= h >> 13
    h = h * 0xC2B2AE35 & 0xFFFFFFFF
    return h ^ h >> 16


def checksum(data, word0=0):
    return sum(fmix32(w ^ ((word0 + i) * 0x9E3779B1 & 0xFFFFFFFF)) for i, (w,) in enumerate(struct.iter_unpack("<I", data))) & (2 ** 64 - 1)


def _expand(fmt):
    return fmt.replace("11i", "i" * 11).replace("4i", "iiii")


def field_offset(name):
    """byte offset of a mirror field in the blob, and its struct code"""
    codes = _expand(MIRROR_FMT)[1:]
    i = MIRROR_NAMES.index(name)
    return HEADER_BYTES + struct.calcsize("<" + codes[:i]), codes[i]


@pytest.fixture(scope="module")
def snap(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("snapshot_format")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(HIP_STUB)
    (d / "drv.cpp").write_text(DRIVER)
    exe = d / "snapshot_format"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{d}", f"-I{CSRC}", f"-I{HOST}", f"-I{ROOT / 'include'}", str(d / "drv.cpp"), "-o", str(exe)])

    def run(cases):
        text = "".join(" ".join(str(v) for v in c) + "\n" for c in cases)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])        # no sanitizer report
        out = r.stdout.splitlines()
        assert len(out) == len(cases)
        return out
    return run


def set_base(mirror=BASE_MIRROR, engine=BASE_ENGINE):
    return ("S",) + tuple(mirror[k] for k in MIRROR_NAMES) + (engine["dtype"], engine["esz"], engine["n_layers"], engine["ks"]) + tuple(engine["features"]) + (engine["num_prompts"], engine["boost_states"])


def set_bytes(offset, code, value, fix=1, newlen=-1):
    raw = struct.pack("<" + code, value)
    return ("V", fix, newlen, len(raw)) + tuple(v for i, b in enumerate(raw) for v in (offset + i, b))


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
def parse_segs(text):
    out = []
    for rec in text.split():
        buf, layer, name, at, nbytes, slot_bytes, blob = rec.split(":")
        out.append(dict(buf=int(buf), layer=int(layer), name=name, at=int(at), bytes=int(nbytes), slot_bytes=int(slot_bytes), blob=int(blob)))
    return out


def test_save_plan_is_the_fork_plan_with_a_third_address(snap):
    """at the mirror points of the fork plan tests (fresh: mel (0, 9) and 256 samples; one chunk; mid chunk: 257 and 7777 samples; kv_head in 257 .. 325; the mel
    window wrapped) under every feature combination: the snapshot plan covers exactly the bytes the fork plan covers, in its order; the blob offsets are
    16-byte aligned, ascending, disjoint and dense up to the padding of a segment to 16 bytes; the section size is their sum; the restore plan into another
    slot is the save plan with source and destination exchanged; a section one vector short is refused"""
    grid = list(itertools.product(KV_HEADS, MELS, (0, 256, 257, 7777), (0, 1), (2, 4)))
    cases = [("P", kv, mel[0], mel[1], cnt, par, esz, 3, 9, 1 + i % 3, 4 + i % 2) + tuple(COMBOS[i % len(COMBOS)] if i % 5 else ALL) for i, (kv, mel, cnt, par, esz) in enumerate(grid)]
    cases += [("P", 0, 0, 9, 256, 0, esz, 2, 9, 0, 1) + tuple(f) for f in COMBOS for esz in (2, 4)]
    seen_padding = set()
    for case, line in zip(cases, snap(cases)):
        save, fork, fault, rest = line.split("|")
        save, fork = parse_segs(save), parse_segs(fork)
        section, n_pack, piece_total, largest, odd, short = rest.split()
        assert fault.strip() == "ok" and short == "refused", (case, fault)
        key = lambda s: (s["buf"], s["layer"], s["name"], s["at"], s["bytes"], s["slot_bytes"])
        assert [key(s) for s in save] == [key(s) for s in fork], case
        at = 0
        for s in save:
            assert s["blob"] == at and at % 16 == 0, (case, s)
            at += -(-s["bytes"] // 16) * 16
            if s["bytes"] % 16:
                seen_padding.add(s["name"])
        assert int(section) == at and all(f["blob"] == 0 for f in fork), case
        assert int(piece_total) == sum(s["bytes"] for s in save) and int(largest) <= 256 * 1024 and int(n_pack) >= len(save) and int(odd) == 0, case
    assert seen_padding == {"last_sample", "aud_hist", "boost_state", "lm_state"}          # the word items, and nothing else


# ---- write, parse, write -------------------------------------------------------------------------------------------------------------------
def test_header_and_mirror_are_written_field_by_field(snap):
    total, head = snap([set_base()])[0].split()
    head = bytes.fromhex(head)
    f = ALL
    mirror_bytes = -(-(100 + 4 * BASE_MIRROR["n_queue"]) // 16) * 16
    assert len(head) == HEADER_BYTES + mirror_bytes
    want = struct.pack("<IIQ16I3Q", 0x5353414E, 1, int(total), 1, 2, 2, 9, KVC, LCTX, MEL_RING, NMEL, ABUF_CAP, HIST_MAX, TOK_CAP, *f,
                       0x1111222233334444, 0x5555666677778888, 0x9999aaaabbbbcccc)
    assert head[:4] == b"NASS" and head[:len(want)] == want
    mb, db, dsum, reserved, hsum = struct.unpack_from("<5Q", head, 104)
    assert (mb, reserved) == (mirror_bytes, 0) and HEADER_BYTES + mb + db == int(total)
    mirror = struct.pack(MIRROR_FMT, *(BASE_MIRROR[k] for k in MIRROR_NAMES)) + struct.pack("<5i", *(i * 7 % 1024 for i in range(5)))
    assert len(mirror) == 120 and head[HEADER_BYTES:] == mirror + bytes(mirror_bytes - len(mirror))
    assert hsum == (checksum(head[:136]) + checksum(head[HEADER_BYTES:], 36)) & (2 ** 64 - 1)
    for name in MIRROR_NAMES:                                         # the offsets the refusal tests below rely on
        off, code = field_offset(name)
        assert struct.unpack_from("<" + code, head, off)[0] == BASE_MIRROR[name], name


def test_write_parse_write_gives_the_same_bytes(snap):
    cases = [set_base(), ("V", 0, -1, 0)]
    for mirror in (dict(BASE_MIRROR, n_queue=0), dict(BASE_MIRROR, n_queue=4096, prompt=-1, channel=1), dict(BASE_MIRROR, R=0, abuf_cnt=0, mel_count=0, sample_rate=16000, encoding=0, channels=1, channel=0),
                   dict(BASE_MIRROR, abuf_cnt=ABUF_CAP, mel_count=MEL_RING, kv_head=325, mel_start=4095)):
        for engine in (BASE_ENGINE, dict(BASE_ENGINE, dtype=0, esz=4, features=(0, 0, 0, 0, 0), boost_states=0), dict(BASE_ENGINE, n_layers=1, ks=5, features=(1, 3, 0, 1, 0))):
            cases += [set_base(mirror, engine), ("V", 0, -1, 0), ("V", 2, -1, 0)]
    out = snap(cases)
    assert [ln for ln in out if not ln[0].isdigit()] == ["accepted same"] * (len(cases) // 3 * 2 + 1)


def test_checksum_is_order_free_position_sensitive_and_sees_every_bit(snap):
    """the sum over a buffer equals the sum over any cut of it into pieces (sizes 4, 16, 20, 262 144 + 16 and 100 004; halves, 256 KiB pieces, an odd cut), each
    piece with its global word offset; two different words exchanged change it; every one of the 2 048 single-bit flips of a 256-byte buffer changes it"""
    assert snap([("C",)]) == ["1 0"]
    assert checksum(b"\x00" * 8) == fmix32(0) + fmix32(0x9E3779B1) and checksum(b"\x01\x00\x00\x00", 2) == fmix32(1 ^ (2 * 0x9E3779B1 & 0xFFFFFFFF))


# ---- the field table and the reset rules ---------------------------------------------------------------------------------------------------
def mirror_case(op, mirror, *front):
    return (op,) + front + tuple(mirror[k] for k in MIRROR_NAMES)


def test_field_table_is_the_wire_format(snap):
    """the visitor's fields take MIRROR_FIXED = 100 bytes with the queue-length word (17 of 32 bits, 4 of 64); a record with every field at its
    maximum (the ranges of test_every_mirror_field_is_range_checked_at_both_ends, R 13, the largest format, a full token queue) is written as
    the format restated above says, and parse followed by write gives the same bytes"""
    big = 2 ** 31 - 1
    top = dict(R=13, prompt=7, abuf_cnt=ABUF_CAP, abuf_par=1, mel_start=MEL_RING - 1, mel_count=MEL_RING, valid_len=LCTX, kv_head=KVC - 1, cc_par=1, chunks=big, tok_read=big,
               samples_in=2 ** 63 - 1, boost_enabled=1, lm_enabled=1, sample_rate=48000, encoding=3, channels=8, channel=7, aud_in=2 ** 63 - 1, aud_out=2 ** 63 - 1, aud_par=1, n_queue=TOK_CAP)
    for mirror in (top, BASE_MIRROR, dict(BASE_MIRROR, n_queue=0)):
        nbytes, fields, same, head = snap([mirror_case("M", mirror)])[0].split()
        assert (int(nbytes), int(fields), int(same)) == (100, 21, 1)
        assert struct.calcsize(MIRROR_FMT) == 100 and len(MIRROR_NAMES) == 22
        head = bytes.fromhex(head)
        want = struct.pack(MIRROR_FMT, *(mirror[k] for k in MIRROR_NAMES)) + struct.pack("<%di" % mirror["n_queue"], *(i * 7 % 1024 for i in range(mirror["n_queue"])))
        assert head[HEADER_BYTES:] == want + bytes(-len(want) % 16)


# what a reset leaves, restated (not read from the header): both modes start these over ...
RESET_BOTH = dict(mel_start=0, mel_count=9, valid_len=0, chunks=0, tok_read=0, samples_in=0, aud_in=0, aud_out=0, aud_par=0, n_queue=0)
# ... only a fresh reset these; R, prompt, the audio format and the two enable flags survive both
RESET_FRESH_ONLY = dict(abuf_cnt=256, abuf_par=0, kv_head=0, cc_par=0)


def test_reset_rules(snap):
    """a record with every field at a distinct non-default value and five queued tokens, after a fresh and after a reference reset, field by field;
    a default record through the fresh reset is what nasr_stream_create makes: 256 waiting samples, 9 mel frames, everything else 0 / default"""
    used = dict(R=6, prompt=2, abuf_cnt=301, abuf_par=1, mel_start=33, mel_count=44, valid_len=55, kv_head=66, cc_par=1, chunks=77, tok_read=88, samples_in=99, boost_enabled=0, lm_enabled=0,
                sample_rate=8000, encoding=1, channels=3, channel=-1, aud_in=111, aud_out=122, aud_par=1, n_queue=5)
    default = dict(R=0, prompt=-1, abuf_cnt=0, abuf_par=0, mel_start=0, mel_count=0, valid_len=0, kv_head=0, cc_par=0, chunks=0, tok_read=0, samples_in=0, boost_enabled=1, lm_enabled=1,
                   sample_rate=16000, encoding=0, channels=1, channel=0, aud_in=0, aud_out=0, aud_par=0, n_queue=0)
    values = [used[k] for k in MIRROR_NAMES if k not in ("abuf_par", "cc_par", "aud_par", "boost_enabled", "lm_enabled")]
    assert len(set(values)) == len(values) and all(used[k] != default[k] for k in MIRROR_NAMES)
    assert set(RESET_BOTH) | set(RESET_FRESH_ONLY) | {"R", "prompt", "boost_enabled", "lm_enabled", "sample_rate", "encoding", "channels", "channel"} == set(MIRROR_NAMES)
    fresh, reference, created = ([int(v) for v in ln.split()] for ln in snap([mirror_case("R", used, 0), mirror_case("R", used, 1), ("D",)]))
    assert dict(zip(MIRROR_NAMES, fresh)) == dict(used, **RESET_BOTH, **RESET_FRESH_ONLY)
    assert dict(zip(MIRROR_NAMES, reference)) == dict(used, **RESET_BOTH)
    assert dict(zip(MIRROR_NAMES, created)) == dict(default, **RESET_BOTH, **RESET_FRESH_ONLY) == dict(default, abuf_cnt=256, mel_count=9)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def refused(line, pattern):
    assert line.startswith("refused: ") and re.search(pattern, line), (line, pattern)
    return line


def test_structure_refusals_each_with_its_own_message(snap):
    total, head = snap([set_base()])[0].split()
    total, head_len = int(total), len(head) // 2
    cases = [
        (("V", 0, -1, 1, 0, ord("X")), r"bad magic"),
        (set_bytes(4, "I", 2, fix=0), r"format version 2, this build reads version 1"),
        (("V", 0, HEADER_BYTES - 1, 0), r"truncated: 143 bytes are no header"),
        (("V", 0, HEADER_BYTES, 0), r"truncated: 144 bytes of %d" % total),
        (("V", 0, head_len, 0), r"truncated: %d bytes of %d" % (head_len, total)),
        (("V", 0, head_len - 1, 0), r"truncated: %d bytes of %d" % (head_len - 1, total)),
        (("V", 0, total - 1, 0), r"truncated: %d bytes of %d" % (total - 1, total)),
        (("V", 0, total + 1, 0), r"trailing bytes: %d bytes, the snapshot ends at %d" % (total + 1, total)),
        (set_bytes(104, "Q", 16 * 9, fix=0), r"section sizes do not add up"),
        (set_bytes(104, "Q", 8, fix=0), r"mirror section of 8 bytes"),
        (set_bytes(128, "Q", 1, fix=0), r"reserved header bytes are not zero"),
        (set_bytes(136, "Q", 12345, fix=0), r"header / mirror checksum mismatch"),
        (set_bytes(field_offset("chunks")[0], "i", 40, fix=0), r"header / mirror checksum mismatch"),
        (set_bytes(20, "I", 4, fix=0), r"header / mirror checksum mismatch"),
        (set_bytes(field_offset("n_queue")[0], "I", 4097), r"tok_queue of 4097 tokens is longer than the token ring \(4096\)"),
        (set_bytes(field_offset("n_queue")[0], "I", 9), r"tok_queue of 9 tokens does not fill a mirror section of 128 bytes"),
        (set_bytes(head_len - 1, "B", 1), r"mirror padding is not zero"),
        (set_bytes(head_len + 1000, "B", 0x5A, fix=1), r"device section checksum mismatch"),
    ]
    out = snap([set_base()] + [c for c, _ in cases])[1:]
    lines = [refused(ln, pat) for ln, (_, pat) in zip(out, cases)]
    assert len({re.sub(r"\d+", "N", ln) for ln in lines}) >= 12               # one message per cause (truncations and the three checksum cases share theirs)


def test_every_mismatching_header_field_is_named_with_both_values(snap):
    names = ["dtype", "element size", "n_layers", "kernel_size", "KVC", "LCTX", "MEL_RING", "NMEL", "ABUF_CAP", "HIST_MAX", "TOK_CAP", "option token_logprobs", "option token_alternatives",
             "option frame_blank_logprobs", "option phrase_boost", "option lm_fusion", "weight set", "boost set", "language model"]
    out = snap([set_base()] + [("G", i, 1) for i in range(19)] + [("G", 3, 0)])[1:]
    values = [1, 2, 2, 9, KVC, LCTX, MEL_RING, NMEL, ABUF_CAP, HIST_MAX, TOK_CAP] + list(ALL)
    for i, name in enumerate(names):
        if i < 16:
            refused(out[i], r"%s mismatch: the snapshot has %d, the engine %d$" % (name, values[i], values[i] + 1))
        else:
            refused(out[i], r"%s mismatch: the snapshot's fingerprint is [0-9a-f]{16}, the engine's [0-9a-f]{16}$" % name)
    assert out[19] == "accepted same" and len(set(out)) == 20
    # the same through the blob's own bytes: each header field changed in the blob (checksum put right) against the unchanged engine
    cases = [set_bytes(16 + 4 * i, "I", values[i] + 1) for i in range(16)] + [set_bytes(80 + 8 * i, "Q", 7) for i in range(3)]
    out2 = snap([set_base()] + cases)[1:]
    for i, name in enumerate(names):
        refused(out2[i], r"%s mismatch" % name)


def test_every_mirror_field_is_range_checked_at_both_ends(snap):
    big = 2 ** 31 - 1
    ranges = dict(prompt=(-1, 7), abuf_cnt=(0, ABUF_CAP), abuf_par=(0, 1), mel_start=(0, MEL_RING - 1), mel_count=(0, MEL_RING), valid_len=(0, LCTX), kv_head=(0, KVC - 1), cc_par=(0, 1),
                  chunks=(0, big), tok_read=(0, big), samples_in=(0, 2 ** 63 - 1), boost_enabled=(0, 1), lm_enabled=(0, 1), aud_in=(0, 2 ** 63 - 1), aud_out=(0, 2 ** 63 - 1), aud_par=(0, 1))
    cases, want = [], []
    for name, (lo, hi) in ranges.items():
        off, code = field_offset(name)
        for v in (lo - 1, hi + 1):
            if code in "I" and v < 0 or v > {"i": big, "I": 2 ** 32 - 1, "q": 2 ** 63 - 1}[code]:
                continue                                               # not representable: the end of the type is the end of the range
            cases.append(set_bytes(off, code, v, fix=2))               # fix = 2: where the plan still fits (the parities), only the range check stands in the way
            want.append(r"mirror field %s = %d is outside %d \.\. %d" % (name, v, lo, hi))
        for v in (lo, hi):                                             # the ends themselves pass the range check (a refusal further on is about something else)
            cases.append(set_bytes(off, code, v, fix=2))
            want.append(None)
    for v in (2, 5, 7, 12, 14, -1):
        cases.append(set_bytes(field_offset("R")[0], "i", v))
        want.append(r"mirror field R = %d is none of 0, 1, 6, 13" % v)
    for name, v, what in (("sample_rate", 12345, "sample_rate"), ("sample_rate", 0, "sample_rate"), ("encoding", 4, "encoding"), ("encoding", -1, "encoding"), ("channels", 0, "channels"),
                          ("channels", 9, "channels"), ("channel", 2, "channel"), ("channel", -2, "channel")):
        cases.append(set_bytes(field_offset(name)[0], "i", v))
        want.append(r"mirror audio format: unsupported %s$" % what)
    out = snap([set_base()] + cases)[1:]
    n_refused = 0
    for ln, pat in zip(out, want):
        if pat is None:
            assert "mirror field" not in ln or "is outside" not in ln, ln
        else:
            refused(ln, pat)
            n_refused += 1
    # below the range: the 14 signed fields (0 - 1 of the two u32 flags is not representable); above it: the 11 whose range ends before their type does
    assert n_refused == 14 + 11 + 6 + 8
    # an English model (no prompts) takes -1 only
    out = snap([set_base(engine=dict(BASE_ENGINE, num_prompts=0))] + [("V", 0, -1, 0)])
    refused(out[1], r"mirror field prompt = 3 is outside -1 \.\. -1")


def test_section_size_and_decoder_fields(snap):
    """a mirror that says another size than the device section has (more samples, fewer mel frames) is refused by the plan, not trusted; what a kernel would use as
    an index without masking is range-checked after the checksum: cur, prev_token, active, the boost state; the padding behind a word item is zero"""
    total, head = snap([set_base()])[0].split()
    head_len = len(head) // 2
    # where ctrl and boost_state are in the device section: 2 layers bf16, kv_head 300 (two runs per plane), mel window wrapped (two runs), 7777 samples
    kv, cc = 2 * 70 * 1024 * 2, 2 * 8 * 1024 * 4
    mel, abuf = 57 * 128 * 4, -(-7777 * 4 // 16) * 16
    ctrl = head_len + 2 * (kv + cc) + mel + abuf + 16 + -(-2 * HIST_MAX * 4 // 16) * 16
    fields = dict(t=0, n_frames=1, symbols=2, prev_token=3, cur=4, n_tok=5, active=6, iterations=7, row=8, dirty=9, frame0=10, frame_next=11)
    after_ctrl = ctrl + 48 + 3 * (4 * 640 * 4) - 4 * 640 * 4 + 640 * 4                 # h, c (4 x 640 f32 each), predg (640 f32)
    cases = [
        (set_bytes(field_offset("abuf_cnt")[0], "i", 7781), r"device section size disagrees with the plan"),
        (set_bytes(field_offset("mel_count")[0], "i", 56), r"device section size disagrees with the plan"),
        (set_bytes(ctrl + 4 * fields["cur"], "i", 2, fix=2), r"decoder ctrl field cur = 2 is outside 0 \.\. 1"),
        (set_bytes(ctrl + 4 * fields["cur"], "i", -1, fix=2), r"decoder ctrl field cur = -1 is outside 0 \.\. 1"),
        (set_bytes(ctrl + 4 * fields["prev_token"], "i", 1025, fix=2), r"decoder ctrl field prev_token = 1025 is outside 0 \.\. 1024"),
        (set_bytes(ctrl + 4 * fields["prev_token"], "i", -1, fix=2), r"decoder ctrl field prev_token = -1 is outside"),
        (set_bytes(ctrl + 4 * fields["active"], "i", 1, fix=2), r"decoder ctrl field active = 1 is outside 0 \.\. 0"),
        (set_bytes(ctrl + 4 * fields["dirty"], "i", 2, fix=2), r"decoder ctrl field dirty = 2 is outside"),
        (set_bytes(ctrl + 4 * fields["n_frames"], "i", 257, fix=2), r"decoder ctrl field n_frames = 257 is outside 0 \.\. 256"),
        (set_bytes(ctrl + 4 * fields["t"], "i", 4, fix=2), r"decoder ctrl field t = 4 is outside 0 \.\. 3"),
        (set_bytes(ctrl + 4 * fields["symbols"], "i", 10, fix=2), r"decoder ctrl field symbols = 10 is outside 0 \.\. 9"),
        (set_bytes(ctrl + 4 * fields["n_tok"], "i", 8, fix=2), r"decoder ctrl field n_tok = 8 is outside 9 \.\. 4105"),
        (set_bytes(ctrl + 4 * fields["row"], "i", -5, fix=2), r"decoder ctrl field row = -5 is outside"),
        (set_bytes(head_len + 2 * (kv + cc) + mel + abuf + 4, "B", 1, fix=2), r"the padding behind 'last_sample' is not zero"),
        (set_bytes(ctrl + 4 * fields["cur"], "i", 2, fix=1), r"device section checksum mismatch"),      # not put right: the checksum speaks first
        (set_bytes(ctrl + 4 * fields["cur"], "i", 0, fix=2), None),
        (set_bytes(ctrl + 4 * fields["prev_token"], "i", 1024, fix=2), None),
    ]
    del after_ctrl
    out = snap([set_base()] + [c for c, _ in cases])[1:]
    for ln, (_, pat) in zip(out, cases):
        if pat is None:
            assert ln == "accepted same", ln
        else:
            refused(ln, pat)
    # boost_state: the last of the segments that are 4 bytes long, before lm_state; found through the plan
    (line,) = snap([("P", 300, 4090, 57, 7777, 1, 2, 2, 9, 0, 1) + ALL])
    segs = {s["name"]: s for s in parse_segs(line.split("|")[0])}
    assert segs["ctrl"]["blob"] == ctrl - head_len and segs["ctrl"]["bytes"] == 48
    at = head_len + segs["boost_state"]["blob"]
    out = snap([set_base(), set_bytes(at, "i", 6, fix=2), set_bytes(at, "i", -1, fix=2), set_bytes(at, "i", 0, fix=2)])[1:]
    refused(out[0], r"boost_state = 6 is no state of the boost set in force \(6 states\)")
    refused(out[1], r"boost_state = -1 is no state")
    assert out[2] == "accepted same"


# ---- fuzz ----------------------------------------------------------------------------------------------------------------------------------
def test_fuzz_corpus_of_blobs_and_envelopes(snap):
    """a few hundred deterministic mutations of valid blobs (bit flips, truncations, trailing bytes, fields spliced in, bytes moved), half of them with the checksums
    put right so that the range checks get their turn, and of an envelope of host/nemo_amd around one: no sanitizer report (the fixture asserts an empty stderr),
    and every outcome is a refusal or "accepted and byte-identical on re-serialisation" """
    small = dict(BASE_MIRROR, n_queue=3)
    cases = [set_base(small, dict(BASE_ENGINE, n_layers=1)), ("F", 1, 300), ("F", 2, 300), ("E", 3, 400), ("E", 4, 400),
             set_base(dict(small, mel_count=0, abuf_cnt=0), dict(BASE_ENGINE, n_layers=1, features=(0, 0, 0, 0, 0), boost_states=0)), ("F", 5, 200)]
    out = [ln for ln in snap(cases) if len(ln.split()) == 3]
    assert len(out) == 5
    for ln, n, blob in zip(out, (300, 300, 400, 400, 200), (True, True, False, False, True)):
        refused_n, accepted, different = (int(v) for v in ln.split())
        assert refused_n + accepted == n and different == 0, ln
        # a blob is checksummed: a mutation is accepted only where the checksums were put right and it hit a don't-care place (a float of the payload);
        # the envelope checks lengths only (what it carries is checksummed by the engine's parser), so a flip inside a field's bytes is accepted unchanged
        assert refused_n >= (n // 2 if blob else 1), ln
    assert sum(int(ln.split()[1]) for ln in out) >= 1


def test_headers_are_pure_host_code():
    src = (CSRC / "nasr_snapshot.h").read_text()
    assert "#include <hip" not in src and "__global__" not in src and "hipLaunch" not in src and "hipMemcpy" not in src
    for name in ("inline bool parse", "inline bool mirror_fault", "inline bool config_mismatch", "inline std::vector<Seg> snapshot_plan", "inline const char *snapshot_plan_fault", "word_term"):
        assert name in src, name
    assert "INTEGRITY-CHECKED, NOT AUTHENTICATED" in src and "forged blob" in src
    env = (HOST / "stream_envelope.h").read_text()
    assert "#include <hip" not in env and "nasr_internal" not in env
    assert "memcpy(&m" not in src and "memcpy(m" not in src            # the mirror is written field by field, never as a struct
