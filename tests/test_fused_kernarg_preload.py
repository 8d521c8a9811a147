"""Kernel-argument preload of the one-problem fused small-M kernels, from the kernel descriptors of the BINARY (CPU suite; no GPU needed).

k_fused_skinny<PRO, MMAX[, NPART]> takes what its first loads need -- the pointers of its prologue and of its weight stream, the shape words -- as
leading scalar arguments, and csrc/Makefile builds kernels_fused.hip so that gfx950's command processor writes them into user SGPRs before the first
wave starts (csrc/kernels_fused.hip: FusedLead; profiles/kernarg_preload.md).  Whether that happens is a property of the kernel descriptor, not of
the source: a kernel whose first parameter is a by-value struct gets a preload length of 0 whatever the flag says, and so does the whole file when
the Makefile line is lost.

Checked here on the descriptors `llvm-objdump -d -j .rodata` prints for the built library:
 1. every instantiation of k_fused_skinny has a non-zero `.amdhsa_user_sgpr_kernarg_preload_length`;
 2. every instantiation of k_fused_skinny_grp has 0 (its problem is picked by blockIdx.z: nothing to preload), and so has every other kernel of the
    library (the flag reaches one translation unit).
llvm-objdump leaves the directive out of a descriptor whose length is 0.
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

KD = re.compile(r"^\.amdhsa_kernel\s+(\S+)\s*$")
PRELOAD = re.compile(r"^\s*\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)\s*$")
END = re.compile(r"^\.end_amdhsa_kernel\s*$")
SINGLE = re.compile(r"^_ZN4nasr\d+k_fused_skinnyILi\d+ELi\d+E")          # mangled nasr::k_fused_skinny<PRO, MMAX, ...>
GROUP = re.compile(r"^_ZN4nasr\d+k_fused_skinny_grpILi\d+ELi\d+E")


def preload_lengths(listing: str) -> dict[str, int]:
    """llvm-objdump -d -j .rodata text -> {kernel: kernarg preload length in dwords}; a descriptor without the directive has 0"""
    out: dict[str, int] = {}
    cur = None
    for line in listing.splitlines():
        m = KD.match(line)
        if m:
            cur = m.group(1)
            assert cur not in out, f"two descriptors of {cur}"
            out[cur] = 0
            continue
        if cur is None:
            continue
        m = PRELOAD.match(line)
        if m:
            out[cur] = int(m.group(1))
        elif END.match(line):
            cur = None
    assert cur is None, f"the descriptor of {cur} does not end"
    return out


PRELOADED = """
00000000000067c0 <_ZN4nasr14k_fused_skinnyILi0ELi1ELi4EEEvPKvS2_S2_S2_S2_iiS2_NS_11FusedParamsE.kd>:
.amdhsa_kernel _ZN4nasr14k_fused_skinnyILi0ELi1ELi4EEEvPKvS2_S2_S2_S2_iiS2_NS_11FusedParamsE
	.amdhsa_group_segment_fixed_size 0
	.amdhsa_kernarg_size 624
	.amdhsa_next_free_vgpr 88
	.amdhsa_user_sgpr_kernarg_segment_ptr 1
	.amdhsa_uses_dynamic_stack 0
	.amdhsa_user_sgpr_kernarg_preload_length 14
.end_amdhsa_kernel
"""
# a by-value struct in front: no directive at all, and the group form right behind it
NOT_PRELOADED = """
0000000000006000 <_ZN4nasr14k_fused_skinnyILi0ELi1ELi4EEEvNS_11FusedParamsE.kd>:
.amdhsa_kernel _ZN4nasr14k_fused_skinnyILi0ELi1ELi4EEEvNS_11FusedParamsE
	.amdhsa_group_segment_fixed_size 0
	.amdhsa_kernarg_size 568
	.amdhsa_user_sgpr_kernarg_segment_ptr 1
	.amdhsa_uses_dynamic_stack 0
.end_amdhsa_kernel

0000000000006040 <_ZN4nasr18k_fused_skinny_grpILi0ELi1ELi4EEEvNS_16FusedParamsGroupE.kd>:
.amdhsa_kernel _ZN4nasr18k_fused_skinny_grpILi0ELi1ELi4EEEvNS_16FusedParamsGroupE
	.amdhsa_group_segment_fixed_size 0
	.amdhsa_kernarg_size 2272
	.amdhsa_user_sgpr_kernarg_segment_ptr 1
	.amdhsa_uses_dynamic_stack 0
.end_amdhsa_kernel
"""


def test_parser_sees_the_length():
    """the check itself: a descriptor with the directive, one without it, and the group form is not taken for the single form"""
    (name, n), = preload_lengths(PRELOADED).items()
    assert SINGLE.match(name) and not GROUP.match(name) and n == 14
    got = preload_lengths(NOT_PRELOADED)
    assert len(got) == 2 and set(got.values()) == {0}
    single = [k for k in got if SINGLE.match(k)]
    group = [k for k in got if GROUP.match(k)]
    assert len(single) == 1 and len(group) == 1 and single != group
    with pytest.raises(AssertionError):
        preload_lengths(PRELOADED.replace(".end_amdhsa_kernel", ""))


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not in this image")
def test_single_kernels_are_preloaded_and_nothing_else_is(tmp_path: Path):
    if not LIB.exists():
        pytest.fail(f"{LIB} not built: run __graft_entry__.build()")
    shutil.copy(LIB, tmp_path / LIB.name)                    # llvm-objdump --offloading writes beside its input: keep that out of the tree
    subprocess.check_call([str(LLVM / "llvm-objdump"), "--offloading", LIB.name], cwd=tmp_path, stdout=subprocess.DEVNULL)
    lengths: dict[str, int] = {}
    for co in sorted(tmp_path.glob("*.hipv4-amdgcn-amd-amdhsa--gfx950")):
        lengths.update(preload_lengths(subprocess.check_output([str(LLVM / "llvm-objdump"), "-d", "-j", ".rodata", co.name], cwd=tmp_path, text=True)))
    assert lengths, f"no gfx950 kernel descriptor in {LIB.name}"
    single = {k: n for k, n in lengths.items() if SINGLE.match(k)}
    group = {k: n for k, n in lengths.items() if GROUP.match(k)}
    assert len(single) >= 14 and len(group) >= 10, f"{len(single)} k_fused_skinny and {len(group)} k_fused_skinny_grp descriptors in {LIB.name}"
    for k, n in sorted(single.items()):
        print(f"{k}: {n} dwords preloaded")
    assert not [k for k, n in single.items() if n == 0], "k_fused_skinny instantiations without kernel-argument preload"
    assert not [k for k, n in group.items() if n != 0], "k_fused_skinny_grp cannot be preloaded: its arguments are one struct"
    others = {k: n for k, n in lengths.items() if n != 0 and k not in single}
    assert not others, f"kernels other than k_fused_skinny with a preload length: {others}"
