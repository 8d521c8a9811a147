"""Host-side restatement of the index arithmetic of the offline attention kernel (nemotron-asr.cpp_amd/csrc/kernels_offline.hip,
k_off_attn_bf16): no GPU.  The constants are READ from the source.  Checked: the LDS fits the stated workgroups per CU, every
position-band row a tile reads lies in the 4 095-row table for every T <= 2048, the band covers each (query, key) score exactly,
and masked keys / unwritten rows are exactly the ragged tail -- no row of another utterance is read or written."""
import re
from pathlib import Path

import numpy as np
import pytest

CSRC = Path(__file__).resolve().parent.parent / "nemotron-asr.cpp_amd" / "csrc"
SRC = (CSRC / "kernels_offline.hip").read_text()
HDR = (CSRC / "nasr_offline_plan.h").read_text()


def _named(text, name):
    m = re.search(rf"\b{name} = (\d+)\b", text)
    assert m, name
    return int(m.group(1))


QB, QB32, BN, BAND, VTP, SPP, WGS = (_named(SRC, n) for n in ("OFF_QB_BF16", "OFF_QB_F32", "OFF_BN", "OFF_BAND", "OFF_VT_PITCH",
                                                                  "OFF_SP_PITCH", "OFF_WG_PER_CU"))
MAXT = _named(HDR, "OFFLINE_MAX_FRAMES")
NREL = 2 * MAXT - 1
DH = 128


def test_lds_fits_the_stated_workgroups_per_cu():
    lds = DH * VTP * 2 + 4 * 16 * SPP * 4
    assert WGS * lds <= 160 * 1024 and WGS >= 4
    assert QB == 4 * 16 and QB32 == 4 * 4 and BN == 64
    assert "__shared__ __attribute__((aligned(16))) bf16_t vt[DH * OFF_VT_PITCH];" in SRC
    assert "__shared__ __attribute__((aligned(16))) float sp[4][16 * OFF_SP_PITCH];" in SRC
    # V^T rows: 64 keys + pad, 8-byte reads at 32 ks + 16 h + 4 q stay in the row
    assert VTP >= BN and (VTP * 2) % 8 == 0 and max(32 * ks + 16 + 4 * q + 3 for ks in range(2) for q in range(4)) < BN
    assert SPP >= BAND >= 16 + BN - 1


def tiles(T):
    for q0 in range(0, T, QB):
        for wave in range(4):
            i0 = q0 + 16 * wave
            for j0 in range(0, T, BN):
                yield i0, j0


@pytest.mark.parametrize("T", [1, 2, 15, 16, 17, 63, 64, 65, 300, 1000, 1983, 1984, 1985, 2047, 2048])
def test_band_rows_stay_in_the_table_and_cover_every_score(T):
    assert "const int rbase = j0 - i0 + (OFFLINE_MAX_T - 16);" in SRC
    assert "sp[wave][r * OFF_SP_PITCH + jl - r + 15]" in SRC
    for i0, j0 in tiles(T):
        rbase = j0 - i0 + (MAXT - 16)
        rows = np.minimum(rbase + np.arange(BAND), NREL - 1)           # the kernel's clamp
        assert rows.min() >= 0 and rows.max() <= NREL - 1
        i = i0 + np.arange(16)[:, None]
        j = j0 + np.arange(BN)[None, :]
        band = (j - j0) - (i - i0) + 15
        assert band.min() >= 0 and band.max() <= BAND - 2                 # band row 79 (the clamped one) is never read
        live = (i < T) & (j < T)
        # the band row read for a live score is the table row of rel = i - j: j - i + 2047 (unclamped)
        assert np.array_equal((rbase + band)[live], (j - i + MAXT - 1)[live])


@pytest.mark.parametrize("lens", [[1, 2, 63, 64, 65, 300], [2048], [5, 2048, 7]])
def test_masked_keys_and_unwritten_rows_cover_the_ragged_tail(lens):
    """packed rows: utterance b = rows [off_b, off_b + T_b).  Keys read unmasked and rows written must be its own rows exactly."""
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    assert "if (j0 + jl >= T) v = -INFINITY;" in SRC and "if (i0 + r < T) {" in SRC
    assert "if (jr > T - 1) jr = T - 1;" in SRC and "if (iq > T - 1) iq = T - 1;" in SRC
    assert "j0 + j < T ? *(const uint4 *)(Vb" in SRC
    for o, T in zip(off, lens):
        written, keys_used, rows_read = set(), set(), set()
        for i0, j0 in tiles(T):
            for r in range(16):
                if i0 + r < T:
                    written.add(o + i0 + r)
                rows_read.add(o + min(i0 + r, T - 1))                      # query rows (clamped)
            for jl in range(BN):
                if j0 + jl < T:
                    keys_used.add(o + j0 + jl)
                rows_read.add(o + min(j0 + jl, T - 1))                     # key rows (clamped), V rows only below T
        assert written == set(range(o, o + T)) == keys_used
        assert rows_read == set(range(o, o + T))                           # never a row of a neighbouring utterance
