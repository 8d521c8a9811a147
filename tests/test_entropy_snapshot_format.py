"""Engine option "token_entropy" in the stream snapshot format (csrc/nasr_snapshot.h), no GPU: the header is compiled with the host
compiler under AddressSanitizer and UBSan, like tests/test_snapshot_format.py.

The option travels WITHOUT a new format version: of the header's 8 once-reserved bytes at offset 128 the low word stays reserved (zero,
"reserved header bytes are not zero") and the high word, offset 132, holds round(1000 alpha).  With the option off a blob is byte for
byte what the writer before the option wrote -- restated here in Python from the format (tests/test_snapshot_format.py's docstring):
little-endian, magic "NASS", version 1, u64 total, sixteen u32, three u64 fingerprints, u64 mirror bytes / device bytes / device checksum,
8 zero bytes, u64 head checksum over the header's first 136 bytes and the mirror."""
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

from tests.test_gemm_plan import HIP_STUB

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nemotron-asr.cpp_amd" / "csrc"

DRIVER = r"""
#include "nasr_internal.h"
#include "nasr_decode_set.h"
#include "nasr_fork_plan.h"
#include "nasr_snapshot.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace nasr;
// W milli device_bytes device_sum n_queue   -> hex of header + mirror of a stream (R = 13, 3 chunks, n_queue queued tokens 7, 8, ...) of an engine
//                                              with token_logprobs = 1, alt_k = 4 and token_entropy = milli
// V milli_blob milli_engine at value        -> the W blob (no device section) with the u32 at `at` set to value and the head checksum put right,
//                                              through parse and config_mismatch against the engine: "ok <entropy_milli parsed>" or "refused: <message>"
// P milli slots                             -> "<section bytes of the largest mirror's snapshot plan> <1 if it has a tok_entropy segment> <that segment's bytes>"
static nasr_snap::Config config(int milli) {
    DecFeatures f;
    f.token_logprobs = true; f.alt_k = 4; f.entropy_milli = milli;
    return nasr_snap::make_config(1, 2, 24, 9, f, 0x1111222233334444ull, 0, 0);
}
static std::vector<uint8_t> blob(int milli, uint64_t device_bytes, uint64_t device_sum, int n_queue) {
    nasr_snap::Header h;
    h.cfg = config(milli); h.device_bytes = device_bytes; h.device_sum = device_sum;
    nasr_snap::Mirror m;
    m.R = 13; m.chunks = 3; m.mel_count = 9; m.abuf_cnt = 256;
    for (int i = 0; i < n_queue; i++) m.tok_queue.push_back(7 + i);
    std::vector<uint8_t> out;
    nasr_snap::write_head(h, m, out);
    return out;
}
int main() {
    char op;
    while (scanf(" %c", &op) == 1) {
        if (op == 'W') {
            int milli, nq; unsigned long long db, ds;
            if (scanf("%d %llu %llu %d", &milli, &db, &ds, &nq) != 4) return 2;
            for (uint8_t b : blob(milli, db, ds, nq)) printf("%02x", b);
            printf("\n");
        } else if (op == 'V') {
            int mb, me, at; unsigned value;
            if (scanf("%d %d %d %u", &mb, &me, &at, &value) != 4) return 2;
            std::vector<uint8_t> b = blob(mb, 0, 0, 2);
            if (at >= 0) for (int i = 0; i < 4; i++) b[(size_t)at + i] = (uint8_t)(value >> (8 * i));
            const uint64_t mbytes = b.size() - nasr_snap::HEADER_BYTES;
            const uint64_t sum = nasr_snap::checksum(b.data(), 136, 0) + nasr_snap::checksum(b.data() + nasr_snap::HEADER_BYTES, (int64_t)mbytes, 36);
            for (int i = 0; i < 8; i++) b[136 + i] = (uint8_t)(sum >> (8 * i));
            nasr_snap::Header h; nasr_snap::Mirror m; std::string err;
            if (!nasr_snap::parse(b.data(), (int64_t)b.size(), h, m, err) || nasr_snap::config_mismatch(h.cfg, config(me), err)) printf("refused: %s\n", err.c_str());
            else printf("ok %u %d\n", h.cfg.entropy_milli, nasr_snap::features_of(h.cfg).entropy_milli);
        } else if (op == 'P') {
            int milli, slots;
            if (scanf("%d %d", &milli, &slots) != 2) return 2;
            DecFeatures f;
            f.token_logprobs = true; f.entropy_milli = milli;
            DecodeSet d;
            int64_t section = 0;
            int has = 0; long long bytes = 0;
            for (const nasr_fork::Seg &s : nasr_snap::snapshot_plan(nasr_snap::largest_mirror(), slots - 1, 2, 24, 9, d, f, &section))
                if (!strcmp(s.name, "tok_entropy")) { has++; bytes = s.bytes; }
            printf("%lld %d %lld\n", (long long)section, has, bytes);
        } else return 2;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("ent_snapshot")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(HIP_STUB)
    (d / "drv.cpp").write_text(DRIVER)
    exe = d / "ent_snapshot"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{d}", f"-I{CSRC}", f"-I{ROOT / 'include'}", str(d / "drv.cpp"), "-o", str(exe)])

    def go(*lines):
        r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return go


def fmix32(h):
    h ^= h >> 16; h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13; h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def checksum(data, word0):
    words = struct.unpack(f"<{len(data) // 4}I", data)
    return sum(fmix32(w ^ (((word0 + i) * 0x9E3779B1) & 0xFFFFFFFF)) for i, w in enumerate(words)) & 0xFFFFFFFFFFFFFFFF


def parent_writer(device_bytes, device_sum, queue):
    """header + mirror as the writer before "token_entropy" wrote them, for the driver's stream and engine"""
    mirror = struct.pack("<11i", 13, -1, 256, 0, 0, 9, 0, 0, 0, 3, 0) + struct.pack("<q", 0) + struct.pack("<2I", 1, 1) + struct.pack("<4i", 16000, 0, 1, 0)
    mirror += struct.pack("<2q", 0, 0) + struct.pack("<i", 0) + struct.pack("<I", len(queue)) + b"".join(struct.pack("<i", t) for t in queue)
    mirror += bytes(-len(mirror) % 16)
    cfg = (1, 2, 24, 9, 326, 70, 4096, 128, 1280 * 256 + 512 + 64, 193, 4096, 1, 4, 0, 0, 0)
    head = struct.pack("<2IQ", 0x5353414E, 1, 144 + len(mirror) + device_bytes) + struct.pack("<16I", *cfg) + struct.pack("<3Q", 0x1111222233334444, 0, 0)
    head += struct.pack("<3Q", len(mirror), device_bytes, device_sum) + bytes(8)
    assert len(head) == 136
    return head + struct.pack("<Q", (checksum(head, 0) + checksum(mirror, 36)) & 0xFFFFFFFFFFFFFFFF) + mirror


@pytest.mark.parametrize("device_bytes,device_sum,n_queue", [(0, 0, 0), (4096, 0x0123456789ABCDEF, 3), (1 << 20, 1, 4096)])
def test_option_off_is_byte_for_byte_the_parent_writer(run, device_bytes, device_sum, n_queue):
    off, = run(f"W 0 {device_bytes} {device_sum} {n_queue}")
    blob = bytes.fromhex(off)
    assert blob[128:136] == bytes(8)
    assert blob == parent_writer(device_bytes, device_sum, [7 + i for i in range(n_queue)])


@pytest.mark.parametrize("milli", [50, 333, 1000, 4000])
def test_option_on_sits_in_the_high_reserved_word(run, milli):
    off, on = (bytes.fromhex(h) for h in run("W 0 4096 99 3", f"W {milli} 4096 99 3"))
    assert struct.unpack_from("<2I", on, 128) == (0, milli)
    assert len(on) == len(off) and struct.unpack_from("<2I", on, 0) == (0x5353414E, 1)       # the same version
    differ = [i for i in range(len(on)) if on[i] != off[i]]
    assert differ and all(132 <= i < 144 for i in differ)                                    # the word and the head checksum over it, nothing else
    assert run(f"V {milli} {milli} -1 0") == [f"ok {milli} {milli}"]


def test_disagreement_is_refused_by_name_and_the_low_word_stays_reserved(run):
    out = run("V 333 1000 -1 0", "V 333 0 -1 0", "V 0 333 -1 0", "V 0 0 -1 0", "V 333 333 128 1", "V 0 0 128 1", "V 0 0 132 333", "V 333 333 132 0", "V 333 333 60 0")
    assert out[0] == "refused: option token_entropy mismatch: the snapshot has 333, the engine 1000"
    assert out[1] == "refused: option token_entropy mismatch: the snapshot has 333, the engine 0"
    assert out[2] == "refused: option token_entropy mismatch: the snapshot has 0, the engine 333"
    assert out[3] == "ok 0 0"
    assert out[4] == out[5] == "refused: reserved header bytes are not zero"
    # the word is part of the configuration like the sixteen in front of it: edited (checksum put right) it is what restore compares
    assert out[6] == "refused: option token_entropy mismatch: the snapshot has 333, the engine 0"
    assert out[7] == "refused: option token_entropy mismatch: the snapshot has 0, the engine 333"
    # an older disagreement is named first (offset 60: token_logprobs)
    assert out[8] == "refused: option token_logprobs mismatch: the snapshot has 0, the engine 1"


def test_device_section_grows_by_the_slots_ring(run):
    off, on = ([int(v) for v in ln.split()] for ln in run("P 0 3", "P 333 3"))
    assert off[1:] == [0, 0] and on[1:] == [1, 4096 * 4]
    assert on[0] - off[0] == 4096 * 4
