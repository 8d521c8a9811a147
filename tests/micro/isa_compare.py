#!/usr/bin/env python3
"""Compare two `hipcc -O3 --cuda-device-only -S` outputs of one .hip file kernel by kernel (refactors that must not change the code):

    python tests/micro/isa_compare.py before.s after.s          # prints a markdown table, exit status 1 on any difference that is not a register exchange

Per kernel symbol: the instruction lines (comments and assembler directives dropped, labels kept), and the code-object notes (VGPRs, SGPRs,
LDS bytes, scratch bytes, spills).  "identical" = the same text.  "registers exchanged" = the same number of lines, and replacing every
register name by a placeholder gives the same text, and the pairs (before, after) form ONE one-to-one map per register class over the whole
kernel -- i.e. the same opcodes, immediates, branch targets and memory offsets with registers renamed consistently."""
import re
import subprocess
import sys

REG = re.compile(r"\b([sva])(\d+)\b|\b([sva])\[(\d+):(\d+)\]")


def kernels(path):
    text = open(path).read()
    body, cur, out = {}, None, {}
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            body[cur] = []
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
            continue
        s = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].strip())          # the label prefix is the number of the function in the file: instantiation order
        if not s or (s.startswith(".") and not s.endswith(":")):
            continue
        body[cur].append(s)
    notes = {}
    for entry in re.split(r"\n  - (?=\.agpr_count)", text):
        name = re.search(r"\n    \.name:\s+(\S+)", entry)
        if not name:
            continue
        get = lambda k: int(re.search(rf"\n    \.{k}:\s+(\d+)", entry).group(1))
        notes[name.group(1)] = dict(vgpr=get("vgpr_count"), sgpr=get("sgpr_count"), lds=get("group_segment_fixed_size"), scratch=get("private_segment_fixed_size"),
                                    spill=get("vgpr_spill_count") + get("sgpr_spill_count"))
    for k, v in body.items():
        if k in notes:
            out[k] = (v, notes[k])
    return out


def regs(line):
    found = []
    for m in REG.finditer(line):
        if m.group(1):
            found.append((m.group(1), int(m.group(2)), 1))
        else:
            found.append((m.group(3), int(m.group(4)), int(m.group(5)) - int(m.group(4)) + 1))
    return REG.sub("R", line), found


def renamed(a, b):
    """None if b is a with registers renamed one-to-one, else the reason."""
    fwd, back, changed = {}, {}, 0
    for la, lb in zip(a, b):
        sa, ra = regs(la)
        sb, rb = regs(lb)
        if sa != sb or [(c, n) for c, _, n in ra] != [(c, n) for c, _, n in rb]:
            return f"instruction differs: `{la}` / `{lb}`"
        changed += la != lb
        for (c, x, n), (_, y, _) in zip(ra, rb):
            for i in range(n):
                if fwd.setdefault((c, x + i), y + i) != y + i or back.setdefault((c, y + i), x + i) != x + i:
                    return f"register map not one-to-one at `{la}` / `{lb}`"
    moved = sorted(f"{c}{x}->{c}{y}" for (c, x), y in fwd.items() if x != y)
    return None, changed, moved


def main(before, after):
    A, B = kernels(before), kernels(after)
    names = subprocess.run(["c++filt"], input="\n".join(sorted(A)), capture_output=True, text=True).stdout.split("\n")
    pretty = dict(zip(sorted(A), (re.sub(r"\(.*", "", n.replace("void nasr::", "")) for n in names)))
    bad = 0
    print("| kernel | instructions before / after | VGPR, SGPR, LDS, scratch, spills before | after | result |")
    print("|---|---|---|---|---|")
    for k in sorted(A):
        if k not in B:
            print(f"| {pretty[k]} | {len(A[k][0])} / - | | | MISSING |")
            bad += 1
            continue
        (ia, na), (ib, nb) = A[k], B[k]
        if ia == ib:
            res = "identical"
        elif len(ia) != len(ib):
            res = "DIFFERENT instruction count"
        else:
            r = renamed(ia, ib)
            res = f"registers exchanged in {r[1]} instructions ({', '.join(r[2])}); opcodes, immediates, labels, offsets identical" if r[0] is None else "DIFFERENT: " + r
        if na != nb or res.startswith("DIFFERENT"):
            bad += 1
            if na != nb:
                res += "; NOTES DIFFER"
        fmt = lambda n: f"{n['vgpr']}, {n['sgpr']}, {n['lds']}, {n['scratch']}, {n['spill']}"
        print(f"| {pretty[k]} | {len(ia)} / {len(ib)} | {fmt(na)} | {fmt(nb)} | {res} |")
    extra = sorted(set(B) - set(A))
    for k in extra:
        print(f"| {k} | - / {len(B[k][0])} | | | NEW |")
    print(f"\n{len(A)} kernels before, {len(B)} after, {bad + len(extra)} not accepted")
    return 1 if bad or extra else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
