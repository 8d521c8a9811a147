"""Load order of the M <= 2 LayerNorm prologue of the fused small-M GEMM, from the BINARY (CPU suite; no GPU needed).

k_fused_skinny<PRO_LN, 1 | 2> and their group forms are meant to put every global load of the launch in flight at once: the prologue's
inputs (LayerNorm weights, x_in, the split-K partials the previous launch has just written), then the wave's `nt` weight loads, and only then
the first wait -- one that leaves the weight loads outstanding, so that the weight stream runs under the LayerNorm (csrc/kernels_fused.hip,
profiles/fused_ln_load_order.md).  hipcc once turned a per-partial `sI < part_splits ? load : zero` into a branch around each load and a
full `s_waitcnt vmcnt(0)` behind the first one, ahead of the weight loads: the source looked right, the binary waited for the previous
kernel's output before it had asked for a single weight.

Checked here on a disassembly of the built library, for every instantiation of those four kernels, between the kernel's entry and its first
`s_barrier` in listing order:
 1. every `nt` global load stands in front of the first `s_waitcnt` that has a vmcnt field;
 2. every such wait has a count >= the number of `nt` loads (the vector-memory counter retires in order: such a wait cannot wait for a weight).
"""
from __future__ import annotations

import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LLVM = Path("/opt/rocm/lib/llvm/bin")
LIB = ROOT / "nemotron-asr.cpp_amd" / "libnemotron_asr_amd.so"

SYMBOL = re.compile(r"^[0-9a-f]+ <(\S+)>:\s*$")
INSN = re.compile(r"^\s+([a-z_0-9]+)\s*(.*?)\s*(//.*)?$")
VMCNT = re.compile(r"\bvmcnt\((\d+)\)")
# mangled nasr::k_fused_skinny[_grp]<PRO_LN = 0, MMAX, ...>: every further template argument is another instantiation of the same kernel
KERNELS = {f"k_fused_skinny{grp}<PRO_LN,{m}>": re.compile(rf"^_ZN4nasr\d+k_fused_skinny{grp}ILi0ELi{m}E") for grp in ("", "_grp") for m in (1, 2)}


def kernels_of(listing: str) -> dict[str, list[tuple[str, str]]]:
    """llvm-objdump -d text -> {symbol: [(mnemonic, operands)...]}"""
    out: dict[str, list[tuple[str, str]]] = {}
    cur = None
    for line in listing.splitlines():
        m = SYMBOL.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = INSN.match(line)
        if m and cur is not None:
            cur.append((m.group(1), m.group(2)))
    return out


def load_order(insns: list[tuple[str, str]]) -> tuple[int, list[str]]:
    """-> (number of nt loads in front of the first s_barrier, what is wrong with the waits there)"""
    head = []
    for mn, ops in insns:
        if mn == "s_barrier":
            break
        head.append((mn, ops))
    else:
        return 0, ["no s_barrier in the kernel"]
    nt = [i for i, (mn, ops) in enumerate(head) if mn.startswith("global_load") and re.search(r"\bnt\b", ops)]
    waits = [(i, int(VMCNT.search(ops).group(1))) for i, (mn, ops) in enumerate(head) if mn == "s_waitcnt" and VMCNT.search(ops)]
    bad = []
    if not nt:
        bad.append("no nt weight load in front of the first s_barrier")
    if waits and nt and waits[0][0] < nt[-1]:
        late = sum(1 for i in nt if i > waits[0][0])
        bad.append(f"s_waitcnt vmcnt({waits[0][1]}) at #{waits[0][0]} stands in front of {late} of the {len(nt)} nt loads")
    bad += [f"s_waitcnt vmcnt({c}) at #{i} leaves fewer than the {len(nt)} nt loads outstanding" for i, c in waits if c < len(nt)]
    return len(nt), bad


GOOD = """
0000000000001900 <_ZN4nasr14k_fused_skinnyILi0ELi1ELi4EEEvNS_11FusedParamsE>:
	s_load_dwordx4 s[8:11], s[0:1], 0x100                      // 000000001900: C00A0200 00000100
	s_waitcnt lgkmcnt(0)                                       // 000000001908: BF8CC07F
	global_load_dwordx4 v[6:9], v1, s[8:9]                     // 00000000190C: DC5C8000 06080001
	global_load_dwordx4 v[54:57], v[14:15], off                // 000000001914: DC5C8000 367F000E
	global_load_dwordx4 v[42:45], v[16:17], off nt             // 00000000191C: DC5E8000 2A7F0010
	global_load_dwordx4 v[38:41], v[18:19], off nt             // 000000001924: DC5E8000 267F0012
	s_waitcnt vmcnt(2)                                         // 00000000192C: BF8C0F72
	v_add_f32_e32 v54, v54, v6                                 // 000000001930: 026C0D36
	s_waitcnt lgkmcnt(0)                                       // 000000001934: BF8CC07F
	s_barrier                                                  // 000000001938: BF8A0000
	s_waitcnt vmcnt(0)                                         // 00000000193C: BF8C0F70
	s_endpgm                                                   // 000000001940: BF810000
"""
# the drain this test is there for: partial 0 is loaded, waited for with the whole counter, copied, and only then are the weights requested
DRAIN = """
0000000000001900 <_ZN4nasr14k_fused_skinnyILi0ELi1EEEvNS_11FusedParamsE>:
	global_load_dwordx4 v[6:9], v1, s[8:9]                     // 00000000190C: DC5C8000 06080001
	s_cmp_lt_i32 s4, 1                                         // 000000001914: BF048104
	s_cbranch_scc1 4                                           // 000000001918: BF850004
	global_load_dwordx4 v[54:57], v[14:15], off                // 00000000191C: DC5C8000 367F000E
	s_waitcnt vmcnt(0)                                         // 000000001924: BF8C0F70
	v_mov_b32_e32 v87, v56                                     // 000000001928: 7EAE0338
	global_load_dwordx4 v[42:45], v[16:17], off nt             // 00000000192C: DC5E8000 2A7F0010
	global_load_dwordx4 v[38:41], v[18:19], off nt             // 000000001934: DC5E8000 267F0012
	s_waitcnt vmcnt(2)                                         // 00000000193C: BF8C0F72
	s_waitcnt lgkmcnt(0)                                       // 000000001940: BF8CC07F
	s_barrier                                                  // 000000001944: BF8A0000
	s_endpgm                                                   // 000000001948: BF810000
"""


def test_parser_sees_the_drain():
    """the check itself: the good listing passes, the one with the early drain does not"""
    (name, insns), = kernels_of(GOOD).items()
    assert KERNELS["k_fused_skinny<PRO_LN,1>"].match(name) and len(insns) == 12
    assert load_order(insns) == (2, [])                                            # vmcnt(0) behind the barrier is not looked at
    (name, insns), = kernels_of(DRAIN).items()
    assert KERNELS["k_fused_skinny<PRO_LN,1>"].match(name) and not KERNELS["k_fused_skinny_grp<PRO_LN,1>"].match(name)
    n_nt, bad = load_order(insns)
    assert n_nt == 2 and len(bad) == 2                                             # the wait stands in front of the weights, and its count is below 2
    assert "in front of 2 of the 2 nt loads" in bad[0] and "vmcnt(0)" in bad[1]
    late_low = [("global_load_dwordx4", "v[42:45], v[16:17], off nt"), ("global_load_dwordx4", "v[38:41], v[18:19], off nt"),
                ("s_waitcnt", "vmcnt(1) lgkmcnt(0)"), ("s_barrier", "")]
    assert len(load_order(late_low)[1]) == 1                                       # behind the weights, but it waits for one of them
    assert load_order([("s_waitcnt", "vmcnt(0)"), ("s_endpgm", "")])[1] == ["no s_barrier in the kernel"]


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not in this image")
def test_ln_prologue_requests_the_weights_before_it_waits(tmp_path: Path):
    if not LIB.exists():
        pytest.fail(f"{LIB} not built: run __graft_entry__.build()")
    shutil.copy(LIB, tmp_path / LIB.name)                    # llvm-objdump --offloading writes beside its input: keep that out of the tree
    subprocess.check_call([str(LLVM / "llvm-objdump"), "--offloading", LIB.name], cwd=tmp_path, stdout=subprocess.DEVNULL)
    kernels: dict[str, list[tuple[str, str]]] = {}
    for co in sorted(tmp_path.glob("*.hipv4-amdgcn-amd-amdhsa--gfx950")):
        kernels.update(kernels_of(subprocess.check_output([str(LLVM / "llvm-objdump"), "-d", co.name], cwd=tmp_path, text=True)))
    assert kernels, f"no gfx950 code object in {LIB.name}"
    problems = []
    for kernel, pat in KERNELS.items():
        found = [s for s in kernels if pat.match(s)]
        assert found, f"{kernel}: no such symbol in {LIB.name}"
        for sym in found:
            n_nt, bad = load_order(kernels[sym])
            print(f"{kernel} ({sym}): {n_nt} nt loads in front of the first barrier, {len(bad)} problem(s)")
            problems += [f"{kernel} ({sym}): {b}" for b in bad]
    assert not problems, "\n".join(problems)
