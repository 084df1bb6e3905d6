#!/usr/bin/env python3
"""Summarise `hipcc -Rpass-analysis=kernel-resource-usage` output (make -C reinmav-gym_amd asm).

    python tools/resource_usage.py [FILE]          one line per kernel
    python tools/resource_usage.py OLD NEW         compare two builds kernel by kernel: every figure of every remark, whatever the order the
                                                   kernels come in and whatever source lines the remarks quote (a header that lost lines moves
                                                   them, so the two files are not byte-equal even when no kernel changed); exits 1 on a difference"""
import re
import sys


def blocks(path):
    return re.split(r"remark: [^\n]*Function Name: ", open(path).read())[1:]


def g(b, k):
    m = re.search(k + r": (\d+)", b)
    return m.group(1) if m else "?"


def figures(path):
    """{kernel: every `remark: <name>: <value>` of its block, in order}"""
    return {b.split()[0]: tuple(re.findall(r"remark:\s+([A-Za-z][^:\n]*: [^\n\[]+?)\s*\[-Rpass", b)) for b in blocks(path)}


if len(sys.argv) > 2:
    old, new = figures(sys.argv[1]), figures(sys.argv[2])
    differ = sorted(k for k in old.keys() & new.keys() if old[k] != new[k])
    for k in differ:
        print("DIFFERS", k, [x for x in zip(old[k], new[k]) if x[0] != x[1]])
    for k in sorted(old.keys() - new.keys()):
        print("MISSING", k)
    for k in sorted(new.keys() - old.keys()):
        print("ADDED", k)
    print(f"{len(old)} kernels in {sys.argv[1]}, {len(new)} in {sys.argv[2]}: {len(differ)} differ, {len(old.keys() - new.keys())} missing, "
          f"{len(new.keys() - old.keys())} added")
    sys.exit(1 if differ or old.keys() != new.keys() else 0)

for b in blocks(sys.argv[1] if len(sys.argv) > 1 else "reinmav-gym_amd/build/resource_usage.txt"):
    name = b.split()[0]
    print("%-58s VGPR %3s AGPR %2s SGPR %3s scratch %3s occ %s LDS %s" % (
        name[:58], g(b, " VGPRs"), g(b, "AGPRs"), g(b, "TotalSGPRs"), g(b, r"ScratchSize \[bytes/lane\]"),
        g(b, r"Occupancy \[waves/SIMD\]"), g(b, r"LDS Size \[bytes/block\]")))
