"""k_dec_joint_split and k_joint_weight_planes alone (engine option "joint_split"), through launch_decode_iter and
tests/helpers/joint_split_harness.hip: one joint-alone call with DecParams::out_planes null (k_dec_joint_tiled) and one with it set, on the cases of
tests/decode_kernel_cases.py against tests/decode_ref.py.
  planes        `==` the numpy split hi = RNE_bf16(w), lo = RNE_bf16(w - hi) of the row-major matrix: tile nt, k step ks = [hi, lo][lane (q, r)][8] = W[16 nt + r][32 ks + 8 q .. + 8).
  exact         small-integer operands are exact in bf16 (lo = 0) and every sum is an exact integer: every output of every form is the f32 tiled kernel's bit for
                bit, ties of the maximum at every border included (15|16, 63|64, 1023|1024: the first maximum wins across lanes, waves and workgroups).
  bounded       random f32 operands, per logit |got - float64| <= (3 2^-16 + 3 640 2^-23) (|out_w| x + |out_b|) + |out_w| (u |e + g|): section 23's bound at K = 640 plus the
                operand-rounding term of tests/test_gpu_decode_kernels.py.  The logit is read from the key of rows with a planted winner.
  independence  a row's key and parts do not depend on the row count or on its position.
Shapes: 65 rows (a second row block of one row, nmt = 1), 128 (whole blocks), 129; the full vocabulary (tile 64 holds blank alone; three waves of workgroup column 16 have no tile)."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi
from tests import decode_kernel_cases as K
from tests import decode_ref as DR
from tests import gemm_ref as R

pytestmark = pytest.mark.gpu
HELPER = Path(__file__).resolve().parent / "helpers" / "libjoint_split_harness.so"
SHAPES = [(5, 13), (8, 16), (3, 43)]
FORMS = [dict(), dict(LP=True), dict(LP=True, BOOST=True), dict(LP=True, ALT=True), dict(LP=True, BOOST=True, LMF=True), dict(LP=True, ENT=True)]
OUTPUTS = {"key": np.uint64, "lp_part": np.uint32, "alt_key": np.uint64, "boost_raw": np.uint32, "ent_part": np.uint32}


class JsCase(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("B", "T", "pool", "n_rows", "n_states", "alt_k", "lp", "boost", "alt", "lmf", "ent", "repeat")] + [("ent_alpha", C.c_float)]


@pytest.fixture(scope="module")
def lib():
    assert HELPER.exists(), "tests/helpers/libjoint_split_harness.so not built (python __graft_entry__.py)"
    C.CDLL(str(capi.LIB_PATH), mode=C.RTLD_GLOBAL)
    L = C.CDLL(str(HELPER))
    L.joint_split_error.restype = C.c_char_p
    L.joint_split_run.argtypes = [C.c_int, C.POINTER(JsCase)] + [C.c_void_p] * 16
    return L


def run(lib, st, w, form=K.PLAIN, alt_k=4):
    """-> planes [65][20][2][64][8] and every output as [2 (out_planes null, set)][B T]..., bit patterns"""
    BT = st["B"] * st["T"]
    case = JsCase(st["B"], st["T"], st["pool"], st["n_rows"], len(st["boost_bonus"]), alt_k, *(int(bool(form.get(n))) for n in ("LP", "BOOST", "ALT", "LMF", "ENT")), 1, 1.0 / 3)
    ins = [np.ascontiguousarray(a) for a in (st["rows"], st["encproj"], st["predg"], w["out_w"], w["out_b"], st["rowmap"], st["boost_bonus"], st["boost_state"], st["lm_row"])]
    assert [a.dtype.itemsize for a in ins] == [4] * 9
    out = {"planes": np.zeros((65, 20, 2, 64, 8), np.uint16), "key": np.zeros((2, BT), np.uint64), "lp_part": np.zeros((2, BT, 17, 2), np.uint32),
           "alt_key": np.zeros((2, BT, 17, alt_k), np.uint64), "boost_raw": np.zeros((2, BT, 17), np.uint32), "ent_part": np.zeros((2, BT, 17), np.uint32)}
    rc = lib.joint_split_run(0, C.byref(case), *(a.ctypes.data for a in ins), *(a.ctypes.data for a in out.values()), None)
    assert rc == 0, lib.joint_split_error().decode()
    return out


def split_bound(st, w):
    """(3 2^-16 + 3 640 2^-23) (|W| x + |b|) + |W| (u |e + g|), x = relu(e + g): [n_rows][VOCAB]"""
    f = np.float64
    e, g = st["encproj"][st["ki"]].astype(f), st["predg"][st["slots"][st["rb"]]].astype(f)
    aw = np.abs(w["out_w"]).astype(f)
    return (3 * 2.0 ** -16 + 3 * DR.JNT * 2.0 ** -23) * (np.maximum(e + g, 0) @ aw.T + np.abs(w["out_b"])) + (K.U24 * np.abs(e + g)) @ aw.T


def test_planes_are_the_numpy_split_in_fragment_order(lib):
    w = K.bounded_weights()
    got = run(lib, K.joint_case(5, 13, 65, False), w)["planes"]
    W = np.zeros((65 * 16, DR.JNT), np.float32)
    W[:DR.VOCAB] = w["out_w"]
    hi = R.bf16_round(W)
    frag = lambda x: R.bf16_bits(x).reshape(65, 16, 20, 4, 8).transpose(0, 2, 3, 1, 4).reshape(65, 20, 64, 8)      # [nt][r][ks][q][8] -> [nt][ks][q * 16 + r][8]
    assert np.array_equal(got, np.stack([frag(hi), frag(W - hi)], axis=2))
    assert got[:, :, 1].any() and not got[64, :, :, 1:16].any()          # lo planes carry bits; rows past 1025 are 0 (lanes r = 1 .. 15 of q = 0 in tile 64)


@pytest.mark.parametrize("form", FORMS, ids=K.form_id)
@pytest.mark.parametrize("B,T", SHAPES)
def test_exact_operands_give_the_f32_tiled_kernels_bits(lib, B, T, form):
    w = K.exact_weights()
    st = K.joint_case(B, T, B * T, True)
    out = run(lib, st, w, form)
    for name in OUTPUTS:
        assert np.array_equal(out[name][0], out[name][1]), name
    bias = K.joint_bias(st, form)
    keyed = K.joint_logits(st, w) + (0.0 if bias is None else bias)
    assert np.array_equal(DR.key_index(out["key"][1][st["ki"]]), DR.first_argmax(keyed))          # not two empty runs: the winners, ties included
    if form.get("LP"):
        assert np.isfinite(out["lp_part"][1][st["ki"]].view(np.float32)[..., 1]).all()


@pytest.mark.parametrize("B,T", SHAPES)
def test_random_operands_stay_within_the_split_bound(lib, B, T):
    w = K.bounded_weights()
    st = K.joint_case(B, T, B * T, False, seed=1)
    win = K.plant_winners(st, w)
    ref, bound = K.joint_logits(st, w), split_bound(st, w)
    assert np.array_equal(DR.first_argmax(ref), win) and (K.margins(ref) >= 4 * bound.max(-1)).all()          # every row: the key names the planted winner whatever the error
    key = run(lib, st, w)["key"][1][st["ki"]]
    rows = np.arange(len(win))
    assert np.array_equal(DR.key_index(key), win)
    ratio = (np.abs(DR.key_logit(key).astype(np.float64) - ref[rows, win]) / bound[rows, win]).max()
    print(f"RATIO joint_split {B}x{T}: {ratio:.4f}")
    assert ratio <= 1.0


def test_a_rows_bits_do_not_depend_on_row_count_or_position(lib):
    w = K.bounded_weights()
    big, small = K.joint_case(3, 43, 129, False, seed=2), K.joint_case(5, 13, 65, False, seed=3)
    i, j = 70, 64                                       # row 70 of 129 (second block, m-tile 0 of 4); row 64 of 65: alone in its block
    small["encproj"][small["ki"][j]] = big["encproj"][big["ki"][i]]
    small["predg"][small["slots"][small["rb"][j]]] = big["predg"][big["slots"][big["rb"][i]]]
    a, b = run(lib, big, w, dict(LP=True)), run(lib, small, w, dict(LP=True))
    assert a["key"][1][big["ki"][i]] == b["key"][1][small["ki"][j]] != 0
    assert np.array_equal(a["lp_part"][1][big["ki"][i]], b["lp_part"][1][small["ki"][j]])
