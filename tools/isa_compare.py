#!/usr/bin/env python3
"""Compare the instruction streams of the kernels of two `make asm` outputs: every listing build/<unit>.gfx950.s of each directory,
by symbol over their union - a kernel that moved to another translation unit is neither missing nor added.  A symbol that two listings
of one directory define is an error, with two exceptions: the internal-linkage `_ZN4rmavL...` helpers, and functions no listing exports
(non-inlined device function templates such as `mlp_mfma32`, which every unit whose kernels call them instantiates).  Every unit has a
copy of such a function, which is compared with the copy of the unit of the same name; a copy less is reported, not counted as missing.

    python tools/isa_compare.py OLD_DIR NEW_DIR

Every kernel symbol of OLD_DIR's assembly is looked up in NEW_DIR's; their bodies (from the symbol's label to `s_endpgm` /
`.Lfunc_end`) are compared after normalising what a change elsewhere in the translation unit moves without changing the code:
local labels (`.LBB12_3` -> `L<k>` in order of first appearance), comments, directives and blank lines.  Prints one line per
symbol that differs or is missing, a summary, and exits 1 if any pre-existing kernel changed.  Symbols only in NEW_DIR are listed
as added.  A typical use: `make asm` on the parent commit, copy build/ aside, `make asm` on the branch, compare.

One difference is reported apart: `s_mov_b32 s15, <k>` in front of a call is the LDS kernel id the backend passes to a non-inlined
device function that reads LDS (the index of the calling kernel in the module's LDS lookup table), and it moves when kernels are
added to the module (an id above 64 is written `s_movk_i32 s15, 0x<k>`: the same size, the same register); a function whose only differences are such immediates is listed as "kernel id only" and does not count as
changed."""
import argparse
import glob
import os
import re
import sys

_LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)*")
_KERNEL_ID = re.compile(r"^(?:s_mov_b32 s15, \d+|s_movk_i32 s15, 0x[0-9a-f]+)$")   # (an id above 64 is no inline constant: s_movk_i32)


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


def _local(symbol, shared=()):
    """internal linkage (every unit that includes its header has a copy of its own), or a function that several units of one directory
    define and none exports - a non-inlined device function template such as mlp_mfma32: keyed by (unit, symbol), compared unit to unit"""
    return symbol.startswith("_ZN4rmavL") or symbol in shared


def directory(path):
    """{symbol: (unit, body)} over every listing of a build directory; a per-unit function (see _local) is keyed by (unit, symbol)"""
    per_unit = {}
    for f in sorted(glob.glob(os.path.join(path, "*.gfx950.s"))):
        per_unit[os.path.basename(f)[:-len(".gfx950.s")]] = (kernels(f), open(f).read())
    # functions that more than one unit defines and none exports (no .globl / .weak NAME: the backend has internalised every copy, as it
    # does with a device function that only the unit's own kernels call); an exported symbol - every kernel - defined twice stays an error
    count, exported = {}, set()
    for unit, (ks, txt) in per_unit.items():
        exported |= set(re.findall(r"^\s*\.(?:globl|weak)\s+(\w+)\s*$", txt, flags=re.M))
        for k in ks:
            count[k] = count.get(k, 0) + 1
    shared = {k for k, c in count.items() if c > 1 and k not in exported}
    out = {}
    for unit, (ks, _) in per_unit.items():
        for k, body in ks.items():
            if not _local(k, shared) and k in out:
                sys.exit(f"ERROR {path}: {k} is defined in {out[k][0]} and in {unit}")
            out[(unit, k) if _local(k, shared) else k] = (unit, body)
    if not out:
        sys.exit(f"ERROR {path}: no *.gfx950.s listing with a function in it")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    args = ap.parse_args()
    changed, missing, same, kid, moved, dropped = [], [], 0, [], 0, 0
    old, new = directory(args.old), directory(args.new)
    name = lambda key: key[1] if isinstance(key, tuple) else key
    new_names = {name(key) for key in new}
    for key, (unit, body) in sorted(old.items(), key=str):
        if key not in new:   # keyed per unit on one side only: a function that a second unit defines on the other side
            alt = (unit, name(key)) if not isinstance(key, tuple) else name(key)
            key = alt if alt in new else key
        if key not in new:
            # a unit's copy of an internal-linkage helper that another unit still defines is a copy less, not a kernel less
            if isinstance(key, tuple) and name(key) in new_names:
                dropped += 1
            else:
                missing.append((unit, name(key)))
            continue
        unit1, body1 = new[key]
        moved += unit1 != unit
        if body1 == body:
            same += 1
        elif len(body1) == len(body) and all(a == b or (_KERNEL_ID.match(a) and _KERNEL_ID.match(b)) for a, b in zip(body, body1)):
            kid.append((unit1, name(key)))
        else:
            diff = sum(1 for a, b in zip(body, body1) if a != b) + abs(len(body) - len(body1))
            changed.append((unit1, name(key), len(body), len(body1), diff))
    old_names = {name(key) for key in old}
    added = sorted((new[key][0], name(key)) for key in new if name(key) not in old_names)
    for unit, k, n0, n1, d in changed:
        print(f"CHANGED {unit} {k}: {n0} -> {n1} lines, {d} differ")
    for unit, k in missing:
        print(f"MISSING {unit} {k}")
    for unit, k in kid:
        print(f"KERNEL-ID-ONLY {unit} {k}")
    print(f"{same} pre-existing functions identical, {len(kid)} identical but for the LDS kernel id, {len(changed)} changed, "
          f"{len(missing)} missing; {len(added)} added; {moved} in another translation unit, {dropped} copies of internal-linkage helpers dropped")
    for unit, k in added:
        print(f"  added {unit} {k}")
    return 1 if changed or missing else 0


if __name__ == "__main__":
    sys.exit(main())
