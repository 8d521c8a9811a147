"""The fused small-M kernels other than the M <= 2 LayerNorm forms compute, bit for bit, what they computed before the one-problem kernel took its
first-needed arguments as leading, preloaded scalars (csrc/kernels_fused.hip: FusedLead; profiles/kernarg_preload.md).

tests/test_gpu_fused_ln_identity.py pins the bits of k_fused_skinny<PRO_LN, 1 | 2>.  This file does the same, in the same way, for single launches of
the kinds it does not cover: PRO_PLAIN, PRO_ATTN and PRO_DWCONV at M = 1 and 2, and one M = 3 row-staging launch of PRO_LN and of PRO_DWCONV.  One
launch through tests/helpers/layer_harness.hip on seeded inputs; the SHA-256 of the output buffers (whole, with their guards; for PRO_DWCONV the
conv-cache pool too) is compared with a constant.  The constants were recorded from the library of the commit before that change:
NASR_KINDS_IDENTITY_RECORD=1 makes every test print its digests instead of comparing them, and NASR_LIB_PATH names the library to load.
test_gpu_layer_kernels.py bounds the error of the same kernels against float64; this file pins the bits.

Each kind runs at its own K with the smallest N its launcher takes: 64 (four workgroups per K slice) for PRO_PLAIN, PRO_LN and PRO_DWCONV, 128
(one column group per head) for PRO_ATTN.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

from tests import gemm_ref as R
from tests.test_gpu_fused_ln_identity import digest, small_problem
from tests.test_gpu_layer_kernels import (KVC, LCTX, NH, PRO_ATTN, PRO_DWCONV, PRO_LN, PRO_PLAIN, AttnSetup, ConvSetup, D, Dev, FusedCase, _no_handles, act_bits,
                                          bounded_case, fused_kernel, rng_of, run_fused, slack_rows, takes)

pytestmark = pytest.mark.gpu

RECORD = os.environ.get("NASR_KINDS_IDENTITY_RECORD") == "1"

# (M, K, splits) -> digest of out_f32 [splits][M][64]
PLAIN = {
    (1, 4096, 4): '6dd011d9bf8f7ded3e05293713ba6d81a64acda727f6d3d91dd97508e2be51e7',
    (1, 1024, 4): '981ee8dd2755397b1f281eca882b7d2252e8a07ed12599c7a38f2784b3acc47e',
    (2, 4096, 4): '84b1bba260f533a02cf5ef4145e47bf0507a942659aad2319fac1dce5767b696',
    (2, 1024, 4): 'ad0ca0544aceacb46cd4b9ec697db30e25cc6549c82414f7ca44da1cd170738e',
}
# case -> digest of out_f32 [8 heads][M][128]; M = 1: valid_len 0 / 3 / 70 with a kv_head whose window wraps the ring
ATTN = {
    'M1 valid 0': 'c518d6988ce817baefc193d6c245ccf05d727298a098aefb3f31881b03ac00ad',
    'M1 valid 3': '55b6c637ace8b7daabef92663a4a1caba1beb2dac0e78c7a3c8d60acdf51ff9c',
    'M1 valid 70': 'c231a9edcb30a572e6ac4c27caf19d715678b16e9142bd43bfed1b8656e984ae',
    'M2 B2 T1': '43ab4ec3ee51e75c1dc820db615bef432a4d4d01b65d3c8ac5b975c7515a2cf2',
    'M2 B1 T2': '74ea4cd2ae6c3423c975d357099c7f622ef5a81ffe520b23465b558fc419f5d6',
}
# (M, cc_par of stream 0) -> digest of out_f32 [4][M][64] and of the conv-cache pool; M = 2: two streams of one row, the second with the other parity
DWCONV = {
    (1, 0): '8cd7343b58c10171dd25eeb722b5893d5f28ed4208fea8e811ef8967e69082b0',
    (1, 1): 'eb7ff1db9ef01a684f21037f7ef04f5488032ebcefa65dadd1a93c19fabae0f2',
    (2, 0): 'ac6cfad5df7c7adc884fceec91480a50702ff664def5220d92e5fd27843c5b61',
    (2, 1): '2cb5bf80d15dbd27bd2e69fde8312a47671610b4ff4153e9f6514868e2b4d1a4',
}
# the row-staging form, M = 3: PRO_LN (4 partials, norm_out of the layer before) -> x_out and out_f32; PRO_DWCONV (three streams of one row) -> out_f32 and the pool
STAGED = {
    'PRO_LN': '7316f813705301c4f2d1a3aacf83ca03ee1710fa72d0fce9193d0dc8a92e1047',
    'PRO_DWCONV': '238d3634edc3b8500f955f943f9439c96f57988ca01150ddaba3ed844a5acf11',
}


def kinds_weight(N, K, seed):
    """every weight a small multiple of 1/8 (exact in bf16), dense: each output column sums K products"""
    return (rng_of("kinds W", N, K, seed).integers(-12, 13, (N, K)) / 8.0).astype(np.float32)


def compare(got, want, what):
    if RECORD:
        print(f"RECORD {what} = {got!r}")
        return
    bad = {k: v for k, v in got.items() if want.get(k) != v}
    assert not bad and got.keys() == want.keys(), f"{what}: the output bits differ from the recorded ones for {list(bad)}"


def test_plain_bits():
    got = {}
    for M, K, splits in PLAIN:
        takes(fused_kernel(PRO_PLAIN, M, K, splits), f"k_fused_skinny<PRO_PLAIN,{M}>")
        A = rng_of("kinds plain A", M, K).standard_normal((M, K)).astype(np.float32)
        with Dev() as dev:
            c = _no_handles(FusedCase())
            c.pro, c.M, c.N, c.K, c.splits, c.epi, c.ldo, c.lda, c.T = PRO_PLAIN, M, 64, K, splits, R.EPI_PART_F32, 64, K, 1
            c.A, c.W = dev.bf16_of(A, slack_rows(M) * K * 4), dev.packed(kinds_weight(64, K, M))
            c.out_f32 = dev.new(splits * M * 64 * 4)
            run_fused(dev, c)
            got[(M, K, splits)] = digest(dev, [c.out_f32])
    compare(got, PLAIN, "PLAIN")


def attn_problem(dev, s: AttnSetup, seed):
    """PRO_ATTN, N = 128, K = 1024, 8 heads = 8 K slices -> (FusedCase, output handle)"""
    M = s.B * s.TS
    q, Kv, Vv, P, bu, bv, _, _ = bounded_case(s, True, "row1")
    c = _no_handles(FusedCase())
    c.pro, c.M, c.N, c.K, c.splits, c.epi, c.ldo, c.T = PRO_ATTN, M, 128, D, NH, R.EPI_PART_F32, 128, 1
    c.W = dev.packed(kinds_weight(128, D, seed))
    c.out_f32 = dev.new(NH * M * 128 * 4)
    a = c.at
    a.q = dev.up(q, slack_rows(M) * D * 4)
    a.kv_pool, a.n_slots, a.act_bf16 = dev.up(s.pool(Kv, Vv, True)), s.n_slots, 1
    a.posproj = dev.up(act_bits(P, True))
    a.bias_u, a.bias_v, a.rows = dev.up(bu), dev.up(bv), dev.up(s.rows())
    a.B, a.T, a.TS = s.B, s.T, s.TS
    return c, c.out_f32


def test_attention_bits():
    cases = [(f"M1 valid {v}", 1, 1, [v], [KVC - 30]) for v in (0, 3, LCTX)] + \
            [("M2 B2 T1", 2, 1, [LCTX, 5], [KVC - 1, 17]), ("M2 B1 T2", 1, 2, [63], [KVC - LCTX - 1])]
    got = {}
    for i, (name, B, T, valid, head) in enumerate(cases):
        M = B * T
        takes(fused_kernel(PRO_ATTN, M, D, NH), f"k_fused_skinny<PRO_ATTN,{M}>")
        s = AttnSetup(B, T, T)
        s.valid, s.head = valid, head
        assert any(h + LCTX + T > KVC for h in head), "a window that wraps the ring"
        with Dev() as dev:
            c, h_out = attn_problem(dev, s, i)
            run_fused(dev, c)
            got[name] = digest(dev, [h_out])
    compare(got, ATTN, "ATTN")


def conv_problem(dev, s: ConvSetup, seed):
    """PRO_DWCONV, N = 64, K = 1024 in 4 slices -> (FusedCase, output handles: the partials and the conv-cache pool)"""
    M = s.B * s.T
    c = _no_handles(FusedCase())
    c.pro, c.M, c.N, c.K, c.splits, c.epi, c.ldo, c.T = PRO_DWCONV, M, 64, D, 4, R.EPI_PART_F32, 64, 1
    c.W = dev.packed(kinds_weight(64, D, seed))
    c.out_f32 = dev.new(4 * M * 64 * 4)
    s.fill(dev, c.cv, act_bf16=True, with_out=False)
    return c, [c.out_f32, c.cv.cc_pool]


def test_dwconv_bits():
    got = {}
    for M, par0 in DWCONV:
        takes(fused_kernel(PRO_DWCONV, M, D, 4), f"k_fused_skinny<PRO_DWCONV,{M}>")
        s = ConvSetup(M, 1, 9, seed=7)
        s.par = [(par0 + b) & 1 for b in range(M)]
        with Dev() as dev:
            c, outs = conv_problem(dev, s, 10 * M + par0)
            run_fused(dev, c)
            got[(M, par0)] = digest(dev, outs)
    compare(got, DWCONV, "DWCONV")


def test_row_staging_bits():
    got = {}
    takes(fused_kernel(PRO_LN, 3, D, 1), "k_fused_skinny<PRO_LN,16>")
    with Dev() as dev:
        c, outs = small_problem(dev, 3, 4, 1, 31)
        run_fused(dev, c)
        got["PRO_LN"] = digest(dev, outs)
    takes(fused_kernel(PRO_DWCONV, 3, D, 4), "k_fused_skinny<PRO_DWCONV,16>")
    s = ConvSetup(3, 1, 9, seed=9)
    with Dev() as dev:
        c, outs = conv_problem(dev, s, 32)
        run_fused(dev, c)
        got["PRO_DWCONV"] = digest(dev, outs)
    compare(got, STAGED, "STAGED")
