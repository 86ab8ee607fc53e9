#!/usr/bin/env python3
"""Compare the gfx950 code of selected kernels between two `hipcc --save-temps` assembly listings (the *-gfx950.s files).

For every kernel whose demangled-insensitive symbol contains one of the given substrings (default: the step kernels, `k_step`), the instructions, the
kernel descriptor (.amdhsa_kernel block) and the metadata entry (amdhsa.kernels) of both listings are compared after normalising what depends on a
function's position in the translation unit only (the function number in local labels).  Exit status 0 and "identical" when nothing differs: the
evidence a change needs before the committed profiles may be re-stamped (tests/test_profiles_consistency.py).  With --stats, prints the register and
scratch figures of the matching kernels of the second listing instead.

    python tools/compare_kernel_isa.py BEFORE.s AFTER.s [--match k_step]
    python tools/compare_kernel_isa.py AFTER.s AFTER.s --match k_rollout --stats
"""
import argparse
import re
import sys


def normalise(text):
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    text = re.sub(r"\.Ltmp\d+", ".Ltmp", text)
    text = re.sub(r"(Header|header|Loop|Child Loop)( *=? *)BB\d+_", r"\1\2BB_", text)  # the same function number inside the assembler's loop comments
    text = re.sub(r"^(\.LBB_\d+:) +;", r"\1 ;", text, flags=re.M)  # a label's comment is padded to a column: one space more or less when the function number changes width (.LBB8_3 / .LBB10_3)
    return text


def kernels(path, match):
    s = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", s, re.M | re.S):
        name = m.group(1)
        if not any(x in name for x in match):
            continue
        body = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.amdhsa_kernel %s\n" % (re.escape(name), re.escape(name)), s, re.M | re.S)
        assert body, name
        out[name] = {"code": normalise(body.group(1)), "descriptor": normalise(m.group(2))}
    meta = s[s.index("amdhsa.kernels:"):]
    for entry in re.split(r"^  - (?=\.)", meta, flags=re.M)[1:]:
        nm = re.search(r"^\s+\.name:\s+(\S+)", entry, re.M)
        if nm and nm.group(1) in out:
            out[nm.group(1)]["metadata"] = entry.split("amdhsa.target")[0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before"); ap.add_argument("after")
    ap.add_argument("--match", action="append")
    ap.add_argument("--stats", action="store_true")
    a = ap.parse_args()
    match = a.match or ["k_step"]
    A, B = kernels(a.before, match), kernels(a.after, match)
    if a.stats:
        for name, k in sorted(B.items()):
            md = k["metadata"]
            get = lambda key: re.search(r"\.%s:\s+(\S+)" % key, md).group(1)
            n_instr = sum(1 for l in k["code"].splitlines() if l.startswith("\t") and not l.startswith("\t.") and not l.startswith("\t;"))
            print(f"{name}: vgpr {get('vgpr_count')} agpr {get('agpr_count')} sgpr {get('sgpr_count')} vgpr_spills {get('vgpr_spill_count')} sgpr_spills {get('sgpr_spill_count')} "
                  f"private_segment_fixed_size {get('private_segment_fixed_size')} lds {get('group_segment_fixed_size')} instructions {n_instr}")
        return 0
    bad = 0
    if set(A) != set(B):
        print("kernel sets differ:", sorted(set(A) ^ set(B))); bad += 1
    for name in sorted(set(A) & set(B)):
        for part in ("code", "descriptor", "metadata"):
            if A[name][part] != B[name][part]:
                print(f"DIFFERENT {part}: {name}"); bad += 1
    print(f"{len(set(A) & set(B))} kernels matching {match} compared:", "identical" if not bad else f"{bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
