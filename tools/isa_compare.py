#!/usr/bin/env python3
"""Compare the instruction streams of the kernels of two `make asm` outputs: the listings of the three translation units,
build/rmav_abi.gfx950.s, build/rmav_policy_abi.gfx950.s and build/rmav_range_abi.gfx950.s.

    python tools/isa_compare.py OLD_DIR NEW_DIR

Every kernel symbol of OLD_DIR's assembly is looked up in NEW_DIR's; their bodies (from the symbol's label to `s_endpgm` /
`.Lfunc_end`) are compared after normalising what a change elsewhere in the translation unit moves without changing the code:
local labels (`.LBB12_3` -> `L<k>` in order of first appearance), comments, directives and blank lines.  Prints one line per
symbol that differs or is missing, a summary, and exits 1 if any pre-existing kernel changed.  Symbols only in NEW_DIR are listed
as added.  A typical use: `make asm` on the parent commit, copy build/ aside, `make asm` on the branch, compare.

One difference is reported apart: `s_mov_b32 s15, <k>` in front of a call is the LDS kernel id the backend passes to a non-inlined
device function that reads LDS (the index of the calling kernel in the module's LDS lookup table), and it moves when kernels are
added to the module; a function whose only differences are such immediates is listed as "kernel id only" and does not count as
changed."""
import argparse
import os
import re
import sys

UNITS = ("rmav_abi.gfx950.s", "rmav_policy_abi.gfx950.s", "rmav_range_abi.gfx950.s")
_LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)*")
_KERNEL_ID = re.compile(r"^s_mov_b32 s15, \d+$")


def kernels(path):
    """{symbol: [normalised instruction lines]} of every function in one .s file"""
    out, name, body = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        s = line.split(";")[0].strip()
        if not s or (s.startswith(".") and not s.startswith(".L")):   # directives; local labels are kept (normalised below)
            continue
        body.append(s)
    for k, b in out.items():
        seen = {}
        out[k] = [_LABEL.sub(lambda m: seen.setdefault(m.group(0), f"L{len(seen)}"), s) for s in b]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    args = ap.parse_args()
    changed, missing, same, added, kid = [], [], 0, [], []
    for unit in UNITS:
        old, new = kernels(os.path.join(args.old, unit)), kernels(os.path.join(args.new, unit))
        for k, body in sorted(old.items()):
            if k not in new:
                missing.append((unit, k))
            elif new[k] == body:
                same += 1
            elif len(new[k]) == len(body) and all(a == b or (_KERNEL_ID.match(a) and _KERNEL_ID.match(b)) for a, b in zip(body, new[k])):
                kid.append((unit, k))
            else:
                diff = sum(1 for a, b in zip(body, new[k]) if a != b) + abs(len(body) - len(new[k]))
                changed.append((unit, k, len(body), len(new[k]), diff))
        added += [(unit, k) for k in sorted(set(new) - set(old))]
    for unit, k, n0, n1, d in changed:
        print(f"CHANGED {unit} {k}: {n0} -> {n1} lines, {d} differ")
    for unit, k in missing:
        print(f"MISSING {unit} {k}")
    for unit, k in kid:
        print(f"KERNEL-ID-ONLY {unit} {k}")
    print(f"{same} pre-existing functions identical, {len(kid)} identical but for the LDS kernel id, {len(changed)} changed, "
          f"{len(missing)} missing; {len(added)} added")
    for unit, k in added:
        print(f"  added {unit} {k}")
    return 1 if changed or missing else 0


if __name__ == "__main__":
    sys.exit(main())
