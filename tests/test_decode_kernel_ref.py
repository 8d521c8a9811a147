"""The cases of tests/test_gpu_decode_kernels.py, checked without a GPU: the exact-mode expectations follow from the float64 reference, every margin and
cap condition holds for every case, the commit's restatement agrees with the per-stream greedy loop, and the kernel-name rule matches the source."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

from tests import decode_kernel_cases as K
from tests import decode_ref as DR
from tests import test_gpu_decode_kernels as G
from tests.decode_ref import BLANK, CT, DEC_CTRL, HID, JNT, VOCAB

CSRC = Path(__file__).resolve().parent.parent / "nemotron-asr.cpp_amd" / "csrc"


@pytest.fixture(scope="module")
def exact_w():
    return {c: K.exact_weights(c) for c in K.LSTM_CONFIGS}


@pytest.fixture(scope="module")
def bounded_w():
    return K.bounded_weights()


def test_exact_lstm_expectation_follows_from_the_float64_reference(exact_w):
    cases = [("g", nd, 0) for nd in K.ND_SWEEP] + [(c, 97, c) for c in K.LSTM_CONFIGS if c != "g"]
    seen = set()
    for cfg, nd, seed in cases:
        w = exact_w[cfg]
        st = K.candidate_case(nd, True, seed=seed)
        assert sorted(st["dlist"].tolist()) == list(range(st["B"])) and st["pool"] == K.POOL and st["B"] < K.POOL
        s, cur, x0, h, c = K.candidate_inputs(st, w)
        h2, c2, g, ok, (pre0, pre1) = K.exact_candidates(w, x0, h, c)
        assert ok, (cfg, nd)                                    # every pre-activation 0 (gate g), >= 32 or <= -128; tanhf(c') exact wherever h' shows it; all below 2^24
        rh, rc, rg = DR.candidates(w, x0, h, c)
        assert np.abs(rh - h2).max() < 1e-12 and np.abs(rc - c2).max() < 1e-9 and np.abs(rg - g).max() < 1e-9
        assert np.array_equal(g, np.round(g)) and np.array_equal(c2.astype(np.float32), c2)
        for L, pre in ((0, pre0), (1, pre1)):                   # every gate is seen open and closed (g: -, 0, +) unless it is the one held fixed
            for j in range(4):
                seen |= {(L, j, int(v)) for v in np.unique(np.sign(pre[:, j]) * (np.abs(pre[:, j]) >= 32))}
        # the tags name their place: the committed c rows read are distinct, and c' = c wherever i is closed and f open
        keep = (pre0[:, 0] <= -128) & (pre0[:, 1] >= 32)
        assert keep.any() and np.array_equal(c2[:, 0][keep], c[:, 0][keep].astype(np.float64))
        assert np.all(h2[:, 0][pre0[:, 3] <= -128] == 0)
    assert seen >= {(L, j, v) for L in range(2) for j in range(4) for v in ((-1, 1) if j != 2 else (-1, 0, 1))}
    tags = K.c_tags(K.POOL)
    assert np.unique(np.abs(tags)).size == tags.size and np.abs(tags).min() >= 8192 and np.abs(tags).max() + 1 < 2 ** 24


def joint_shapes():
    for n in K.SMALL_ROWS_SWEEP:
        for B, T, ragged in G.small_layouts(n):
            yield B, T, n, ragged
    for n in K.TILED_ROWS_SWEEP:
        yield 15, 14, n, True
    yield 5, 4, 17, False
    yield 22, 4, 81, False


def test_exact_joint_cases(exact_w):
    w = exact_w["g"]
    assert set(np.unique(w["out_w"])) <= {-2, -1, 0, 1, 2} and np.array_equal(w["out_b"], np.round(w["out_b"]))
    kinds = set()
    for B, T, n, ragged in joint_shapes():
        assert (B * T <= 64) == (n in K.SMALL_ROWS_SWEEP or (B, T) == (5, 4)) or B * T > 64
        st = K.joint_case(B, T, n, True, ragged=ragged)
        assert len(st["rm"]) == n and len(set(st["rm"].tolist())) == n and st["pool"] > B
        assert np.all((st["rowmap"] & 0xffff) < B) and np.all((st["rowmap"] >> 16) < T)            # every entry in range, the ones behind n_rows too
        n_dec = st["rows"][:, 5]
        assert np.all(st["rf"] < n_dec[st["rb"]])                                                    # no evaluated row is a sentinel row of encproj
        enc = st["encproj"].reshape(B, T, JNT)
        for b in range(B):
            assert np.all(np.isnan(enc[b, n_dec[b]:])) and np.all(np.isfinite(enc[b, :n_dec[b]]))
        L = K.joint_logits(st, w)
        x = st["encproj"][st["ki"]] + st["predg"][st["slots"][st["rb"]]]
        assert 0.3 < (x[:, :K.SEL0] < 0).mean() < 0.6                                                # the ReLU cuts about half the k
        assert np.array_equal(L, np.round(L)) and (np.abs(x) @ np.abs(w["out_w"]).T).max() + 8 < 2 ** 24
        for form in (K.PLAIN, K.RICH, K.RICH_LMF):
            bias = K.joint_bias(st, form)
            if bias is not None:
                assert np.array_equal(bias, np.round(bias)) and np.all(bias[:, BLANK] == 0)
        kind = st["kind"][st["ki"]]
        for i in range(n):
            if kind[i] < len(K.TIES):
                tie = list(K.TIES[kind[i]])
                assert np.all(L[i, tie] == L[i].max()) and (L[i] == L[i].max()).sum() == len(tie) and DR.first_argmax(L[i]) == tie[0]
                kinds.add(int(kind[i]))
        if n >= len(K.TIES):
            assert set(kind.tolist()) >= set(range(len(K.TIES)))
        assert len({L[i].tobytes() for i in range(n)}) == n                                          # a wrong row, frame or slot gives other integers
    assert kinds == set(range(len(K.TIES))) and len(K.TIES) == len(K.TIE_SPANS)
    # what the pairs span: lane = v // 4 within a tile of 16, tile = v // 16, workgroup of the tiled kernel = v // 64
    (a, b), (c, d), (e, f), (g, h), (i, j) = K.TIES[:5]
    assert a // 4 == b // 4 and c // 16 == d // 16 and (c // 4) ^ (d // 4) == 1 and e // 16 == f // 16 and ((e // 4) ^ (f // 4)) & 3 == 2
    assert g // 16 != h // 16 and g // 64 == h // 64 and i // 64 != j // 64


def test_bounded_joint_margins(bounded_w):
    w = bounded_w
    for B, T, n, ragged in joint_shapes():
        st = K.joint_case(B, T, n, False, ragged=ragged)
        win = K.plant_winners(st, w, 0)
        L = K.joint_logits(st, w)
        bound = K.logit_bound(st, w)
        for form in (K.PLAIN, K.RICH, K.RICH_LMF, dict(LP=True, BOOST=True, ALT=True, BEAMB=True)):
            bias = K.joint_bias(st, form)
            V = L if bias is None else L + bias
            assert np.array_equal(DR.first_argmax(V), win)
            assert np.all(K.margins(V) >= 4 * (bound.max(-1) + K.U24 * np.abs(V).max(-1))), (B, T, n, K.form_id(form))     # every row, none left out


def test_encproj_cases():
    src = "".join((CSRC / f).read_text() for f in ("nasr_diar.hip", "nasr_encoder.hip"))
    assert len(re.findall(r"\blaunch_encproj\(", src)) == 4                                          # encoder (D, JNT); SE fc1, fc2; the speaker embedding
    assert "blk.cout, blk.cout / 8" in src and "blk.cout / 8, blk.cout" in src and "2 * SPK_C, SPK_EMB" in src and "M, D, JNT" in src
    topo = re.search(r"SPK_TOPO\[5\] = (.*?);", src, re.S).group(1)
    couts = {int(m.group(1)) for m in re.finditer(r"\{\d+, \d+, \d+, \d+, (\d+),", topo)}
    internal = (CSRC / "nasr_internal.h").read_text()
    spk_c, spk_emb = (int(re.search(rf"{n} = (\d+)", internal).group(1)) for n in ("SPK_C", "SPK_EMB"))
    sites = {(1024, 640), (2 * spk_c, spk_emb)} | {(c, c // 8) for c in couts} | {(c // 8, c) for c in couts}
    assert sites == set(K.ENCPROJ_SITES)
    for Kd, N in K.ENCPROJ_SITES:
        assert Kd % 64 == 0 and N % 16 == 0, "k_encproj gives each of its four waves K / 64 k-groups: another K would drop the remainder without a word"
    for M, Kd, N in G.ENCPROJ_CASES:
        x, W, b, ref, bound = K.encproj_case(M, Kd, N, True)
        assert np.array_equal(ref, np.round(ref)) and (np.abs(x) @ np.abs(W).T).max() + 8 < 2 ** 24


def test_commit_cases_are_consistent():
    for T in (4, 6):
        for form in G.COMMIT_FORMS:
            st, streams, logits, best, parts = G.commit_case(T, form, 8, 1.0)
            B = st["B"]
            na, dl, rm = DR.build_lists(st["ctrl"], st["slots"])
            n = len(rm)
            assert set(st["rowmap"][:n].tolist()) == rm and n > 0        # the planted rowmap is what build_lists leaves for the planted control blocks
            assert np.all((st["rowmap"] & 0xffff) < B) and np.all((st["rowmap"] >> 16) < T)
            for e in rm:
                ki = (e & 0xffff) * T + (e >> 16)
                assert DR.key_index(st["key"][ki]) == best[ki] == DR.first_argmax(logits[ki])
            want, soft = G.expect_commit(st, streams, logits, best, parts, form, 8, 1.0)
            ct = want["ctrl"][st["slots"]]
            assert set(ct[:, CT["symbols"]].tolist()) >= {0, 1, 4} and 0 in ct[:, CT["active"]] and 1 in ct[:, CT["active"]]
            masked = [s.get("n_tok") for s in streams if "n_tok" in s]
            assert masked == [4095, 4096, 8191]
            f0 = [s["frame0"] for s in streams if "frame0" in s][0]
            assert f0 // 4096 != (f0 + T - 1) // 4096                    # frame0 + f crosses a multiple of 4096


def test_commit_restatement_agrees_with_the_greedy_loop():
    """the device's schedule (evaluate every remaining frame against the cached g, commit up to the first non-blank) in float64, by decode_ref.commit_stream,
    against the reference's symbol-by-symbol loop: tokens, frames, iterations and the final state are the same"""
    w = K.chain_weights(G.CHAIN_SEED)
    st = G.chain_case(3, 4)
    enc = st["encproj"].reshape(3, 4, JNT)
    blanks = tokens = 0
    for b, slot in enumerate(st["slots"]):
        ct = dict(zip(DEC_CTRL, (int(v) for v in st["ctrl"][slot])))
        nf = int(st["rows"][b, 5])
        h, c = st["h"][slot, ct["cur"]].astype(np.float64), st["c"][slot, ct["cur"]].astype(np.float64)
        toks, frames, it, h_, c_, prev, sym, evals = DR.greedy_stream(w, enc[b], nf, h, c, ct["prev_token"])
        ct.update(t=0, n_frames=nf, symbols=0, active=1, iterations=0, n_tok=0)
        got_t, got_f, calls = [], [], 0
        while ct["active"]:
            calls += 1
            assert calls <= 10 * 4 + 1
            h2, c2, g = DR.candidates(w, w["embed"][ct["prev_token"]][None].astype(np.float64), h[None], c[None])
            tok, f, _, _ = DR.commit_stream(ct, lambda f: int(DR.first_argmax(DR.joint(enc[b, f][None], g, w["out_w"], w["out_b"])[0])))
            if tok is not None:
                got_t.append(tok)
                got_f.append(f)
                h, c = h2[0], c2[0]
        assert (got_t, got_f, ct["iterations"], ct["prev_token"], ct["symbols"]) == (toks, frames, it, prev, sym)
        assert np.array_equal(h, h_) and np.array_equal(c, c_)
        tokens += len(toks)
        blanks += it - len(toks)
    assert tokens > 0 and blanks > 0


@pytest.mark.parametrize("B,T", [(3, 4), (20, 4)])
def test_chained_margins(B, T):
    w = K.chain_weights(G.CHAIN_SEED)
    st = G.chain_case(B, T)
    ref, worst = G.chain_reference(st, w)
    assert worst >= 4.0, worst                                          # along the whole trajectory of every stream
    assert sum(len(r["toks"]) for r in ref) > 0 and sum(r["it"] - len(r["toks"]) for r in ref) > 0
    assert max(r["it"] for r in ref) <= 10 * T + T


def test_kernel_names_match_the_source():
    G.test_every_decode_kernel_is_reached()


def test_constants_match_the_headers():
    text = "".join((CSRC / f).read_text() for f in ("nasr_constants.h", "nasr_logprob.h", "nasr_boost.h", "nasr_lm.h"))
    for name, val in (("HID", HID), ("JNT", JNT), ("VOCAB", VOCAB), ("BLANK", BLANK), ("TOK_CAP", DR.TOK_CAP), ("FRAME_CAP", DR.FRAME_CAP), ("MAX_SYMBOLS", DR.MAX_SYMBOLS),
                      ("SMALL_ROWS", DR.SMALL_ROWS), ("COLS", DR.COLS), ("ROW_COLS", DR.COLS)):
        m = re.search(rf"\b{name}\s*=\s*(\d+)", text)
        assert m and int(m.group(1)) == val, name
