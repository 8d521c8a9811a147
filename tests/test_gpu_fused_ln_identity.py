"""The M <= 2 LayerNorm prologue of the fused small-M GEMM (k_fused_skinny<PRO_LN, 1 | 2> and the group forms) computes, bit for bit, what it
computed before its loads were put in order (profiles/fused_ln_load_order.md).

One launch through tests/helpers/layer_harness.hip on seeded inputs; the SHA-256 of the output buffers (x_out and what the epilogue writes, whole, with
their guards) is compared with a constant.  The constants were recorded from the library of the commit before that change, which computed the same
prologue with conditional partial loads: NASR_LN_IDENTITY_RECORD=1 makes every test print its digests instead of comparing them, and NASR_LIB_PATH names
the library to load.  test_gpu_layer_kernels.py::test_fused_ln bounds the error of the same kernels against float64; this file pins the bits, so a change
of the order of additions, of a contraction or of a rounding shows here even where it stays inside that bound.
"""
from __future__ import annotations

import hashlib
import os

import numpy as np
import pytest

from tests import gemm_ref as R
from tests.test_gpu_layer_kernels import PRO_LN, D, Dev, FusedCase, LnSetup, PostSetup, _no_handles, fused_kernel, rng_of, run_fused, slack_rows, takes

pytestmark = pytest.mark.gpu

RECORD = os.environ.get("NASR_LN_IDENTITY_RECORD") == "1"

# (grouped, M) -> {(part_splits, lno): digest}: K = 1024, N = 64 (four workgroups), f32 GEMM output; "0+4": a group of a problem without partials and one with 4
SMALL = {
    (0, 1): {
        (0, 0): '57112ef8dcdc20fd0cd6ba90d81ee83c8cf51e989d2533dadbea8c887f78a718',
        (0, 1): '1aa2c4c7160fe6680d6a66a49f24af875cfc318ecd5d648e7ddb753470d76d65',
        (4, 0): 'c314174d3fa4e03185d010126c70e4a84783403d7552386b1e33e8a77ace374c',
        (4, 1): 'a3f3aacaf03369c4bae01cbcf94749ce3fd478b2f5db5738344260921d3802b1',
        (8, 0): '9a65c326ed6b789136f42d61c36492211870b7bcb26c44aafb1c334d424d0ab8',
        (8, 1): '17d5e329f9bd1ae5e03e93ad642b2cd4b1f39781ad5812527c152168f0ece3de',
    },
    (0, 2): {
        (0, 0): 'c308e0a1503dc1ec940c16eb24357519fa4f1fb6ed19055b7a66844778d6aea9',
        (0, 1): '7c2dcc26a3818dde9e7f8fef2caabee52b10b4f8ba618407808b82d8eed9258e',
        (4, 0): 'a839a8835eb299e54a9621b4b3e718b73e20ccaa9d8fb5da7eb9697d26ccd9b5',
        (4, 1): 'c10334503e5f6881680cdf9638592b7319a576d99fc71caf5af63f9dd46e2e33',
        (8, 0): '239e5c91af1c1af0462216cc3dd71aa112465ccc0ee679afeecba26e0aab8d3d',
        (8, 1): '505f57c0c9dd83d36637e1585d6899c2d0e1008e91685b72c4e156f3e863d2b7',
    },
    (1, 1): {
        (0, 0): '1f7e5dea90617ca7380b3a6582f0e6221b27371208a466cde581315cc5c7f430',
        (0, 1): '24ac8d3d929f877ab38c7efad65c72ad51975cc35dc3afee619e073fdae43745',
        (4, 0): 'bcb78b035cf9831a004f50228910cbd23aec151a036444b13ef69f4755e0ee30',
        (4, 1): '3950a591cdef1569989568f7062d0726d687a39acd9936ca426d62385686db36',
        (8, 0): 'ced2695453335b651f004009ecd11ba71d8fee70ba2958f3d7303b9d27ae8974',
        (8, 1): 'b174609a4d15aa8c4db9d2a1a5eb1115ec063ceaf2c6072bfb9308008a4c1504',
        '0+4': '5cd8ac69c611483dd3cb0f89519325a18638cd9d05fd093a0387fe3a763992f7',
    },
    (1, 2): {
        (0, 0): 'a78d4d38f2b5b73b2aa182ad01202e4efe1132c4e05f805743db5272d400c02e',
        (0, 1): '23748fa74c11921595effac87ae22faf52c1f8a60c130efd71d4baf4d4067c80',
        (4, 0): 'a5b7fe8cbbbc55c1b9639d7163e3e9255ea98443e304821501c9463da54be50c',
        (4, 1): '981736c478aa86a857678806489c174ad99c9e3dea96866645a49c8dd5f9d26d',
        (8, 0): '7b873a094268bc2a74e73781ee4a21f9245ab8d22ac56c190ee1c55d7dae6c38',
        (8, 1): '8fbe06f3fc86de4739c5bce93250850692365f592defe5bd61bce25eb5115018',
        '0+4': 'ef367e20679fb59a6c38ae78645a150185591298bca9da3e199c11f75028c7f2',
    },
}
# epilogue -> digest: M = 1 at the layer's own N (4096 SiLU, 2048 GLU, 3072 QKV into the K / V rings), dense weights
REAL = {
    'SILU_ACT': '6661e648ac866a3ee32b3ed33477fc31752602f14bd3020c3eabccb72f87069e',
    'GLU': 'd848d14d6f3ce9ba099b9110b26f44fccd07653561cd34a789d324bf46ae8c5b',
    'QKV': '7aabbc1cd43b591cdb248ac31bcfa46c0c8456b1fd4b151fe473051001a0564e',
}


def dense_weight(N, seed):
    """every weight a small multiple of 1/8 (exact in bf16), no zeros pattern: each output column sums 1024 products"""
    return (rng_of("identity W", N, seed).integers(-12, 13, (N, D)) / 8.0).astype(np.float32)


def small_problem(dev, M, part_splits, lno, seed):
    p = PostSetup(M, part_splits, seed=seed)
    c = _no_handles(FusedCase())
    c.pro, c.M, c.N, c.K, c.splits, c.epi, c.ldo, c.T = PRO_LN, M, 64, D, 1, R.EPI_PART_F32, 64, M
    c.W = dev.packed(dense_weight(64, seed))
    c.x_in, c.x_out = dev.up(p.x, slack_rows(M) * D * 4), dev.new((M + slack_rows(M)) * D * 4)
    if part_splits:
        c.part, c.part_splits, c.scale = dev.up(p.part), part_splits, p.scale
    if lno:
        c.lno_w, c.lno_b = dev.up(p.ln[0][0]), dev.up(p.ln[0][1])
    c.ln_w, c.ln_b = dev.up(p.ln[1][0]), dev.up(p.ln[1][1])
    c.out_f32 = dev.new(M * 64 * 4)
    return c, [c.x_out, c.out_f32]


def digest(dev, handles):
    h = hashlib.sha256()
    for b in handles:
        raw = dev.raw(b)
        assert not np.all(raw == raw[0]), "an output buffer was not written"
        h.update(raw.tobytes())
    return h.hexdigest()


def compare(got, want, what):
    if RECORD:
        print(f"RECORD {what} = {got!r}")
        return
    bad = {k: v for k, v in got.items() if want.get(k) != v}
    assert not bad and got.keys() == want.keys(), f"{what}: the output bits differ from the recorded ones for {list(bad)}"


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("grouped", [0, 1], ids=["single", "group"])
def test_ln_prologue_bits(grouped, M):
    takes(fused_kernel(PRO_LN, M, D, 1, grouped=bool(grouped)), f"k_fused_skinny{'_grp' if grouped else ''}<PRO_LN,{M}>")
    got = {}
    for part_splits in (0, 4, 8):
        for lno in (0, 1):
            with Dev() as dev:
                if grouped:                                                   # two problems in one launch, each with its own inputs and weights
                    cases, outs = zip(*[small_problem(dev, M, part_splits, lno, seed) for seed in (11, 12)])
                    run_fused(dev, list(cases), n=2, grouped=1)
                    got[(part_splits, lno)] = digest(dev, [h for o in outs for h in o])
                else:
                    c, outs = small_problem(dev, M, part_splits, lno, 11)
                    run_fused(dev, c)
                    got[(part_splits, lno)] = digest(dev, outs)
    if grouped:                                                               # what the pipeline's first stage does: layer 0 (no partials, no norm_out) beside a later layer
        with Dev() as dev:
            cases, outs = zip(small_problem(dev, M, 0, 0, 11), small_problem(dev, M, 4, 1, 12))
            run_fused(dev, list(cases), n=2, grouped=1)
            got["0+4"] = digest(dev, [h for o in outs for h in o])
    compare(got, SMALL[(grouped, M)], f"SMALL[({grouped}, {M})]")


def test_partial_counts_the_small_forms_are_not_built_for():
    """the M <= 2 kernels load 4 or 8 partials.  Any other count takes the row-staging form (checked against float64 like every other case); a group
    whose problems disagree on the count is launched problem by problem, with the bits of the single launches"""
    for M, part_splits in ((1, 3), (2, 5)):
        s = LnSetup(M, part_splits, 1, R.EPI_GLU, seed=5)
        with Dev() as dev:
            c = s.problem(dev)
            run_fused(dev, c)
            print(f"fused PRO_LN M {M}, {part_splits} partials: worst |got - ref| / bound = {s.check(dev, c):.3f}")
    with Dev() as dev:
        single = []
        for part_splits, seed in ((4, 11), (8, 12)):
            c, outs = small_problem(dev, 1, part_splits, 1, seed)
            run_fused(dev, c)
            single.append(digest(dev, outs))
        cases, outs = zip(small_problem(dev, 1, 4, 1, 11), small_problem(dev, 1, 8, 1, 12))
        run_fused(dev, list(cases), n=2, grouped=1)
        assert [digest(dev, o) for o in outs] == single


def test_ln_prologue_bits_at_the_layer_shapes():
    takes(fused_kernel(PRO_LN, 1, D, 1), "k_fused_skinny<PRO_LN,1>")
    got = {}
    for epi, part_splits, lno in ((R.EPI_SILU_ACT, 4, 1), (R.EPI_GLU, 8, 0), (R.EPI_QKV, 4, 0)):
        s = LnSetup(1, part_splits, lno, epi, seed=21)
        with Dev() as dev:
            c = s.problem(dev)
            c.W = dev.packed(dense_weight(s.N, epi))
            run_fused(dev, c)
            got[R.EPI_NAMES[epi]] = digest(dev, s.outputs(c))
    compare(got, REAL, "REAL")
