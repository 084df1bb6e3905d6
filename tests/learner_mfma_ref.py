"""The tolerance rule and the shapes of the matrix-core learner's tests (rmav_ppo_grad_shared_mfma, csrc/rmav_learner_mfma.hpp).  The
oracle, the restatement with its mutants and the inputs are learner_shared_ref's (the same loss on the same 9 tensors); what is the
kernel's own is its geometry, and with it the chain of sequential roundings the bound is derived from.

Geometry: a wavefront owns a tile of 32 samples, a workgroup of 4 wavefronts a step of 128; step s belongs to workgroup s mod groups,
groups = min(steps, GROUPS).  ``chain_mfma`` counts the longest run of sequential roundings of one gradient element:
    64   over K in a layer (the fp32-input matrix instruction is a k-ordered fmaf chain)
    32   per wavefront tile (the sample index is K of the weight gradients), tile after tile in a wavefront
     4   the wavefronts of a workgroup, added in wavefront order
     g   the workgroups' partial records, added in workgroup order by the fold
``margin_mfma`` is learner_ref.margin's rule on that chain: MARGIN for every chain up to the 162 roundings MARGIN was rounded for
(profiles/r23/learner.md), beyond it the chain over the shortest a blocked or pairwise sum can have, 6 + log2 B, never below MARGIN.
profiles/r29/learner_mfma.md has the derivation and the values at every tested B."""
import math

import learner_ref
import learner_shared_ref as R   # noqa: F401  (re-exported: the tests take oracle, restate, make_case, ... from here)
from learner_ref import FLOOR, MARGIN   # noqa: F401

TILE, STEP, GROUPS = 32, 128, 256   # kMatTile, kMatStep, kMatMaxGroups of csrc/rmav_learner_mfma.hpp
BATCHES = (1, 31, 32, 33, 127, 128, 129, 2125)   # the wavefront-tile and workgroup-step edges
# Batches at which a wavefront walks several tiles, as (kind, B, statistics, idx route, ent_coef): G steps + 1 sample (workgroup 0 walks
# a second step that is a one-sample tail: one live lane in wavefront 0, none in the other three); 2 G steps + 129 (workgroup 0 walks
# three, its third full, workgroup 1's third a one-sample tail); three full steps per workgroup at the widest state
WALKS = (("quad3d", GROUPS * STEP + 1, True, True, 0.01), ("quad3d", 2 * GROUPS * STEP + 129, True, True, 0.01),
         ("quad3d_sl", 3 * GROUPS * STEP, False, False, 0.0))


def steps(B):
    return -(-B // STEP)


def groups(B):
    return min(steps(B), GROUPS)


def chain_mfma(B):
    """the longest run of sequential roundings of a kernel sum"""
    return 64 + TILE * -(-steps(B) // GROUPS) + 4 + groups(B)


def margin_mfma(B):
    """The factor of the bound err(kernel) <= margin_mfma(B) * max(err(torch fp32), FLOOR): learner_ref.margin's rule, evaluated on this
    kernel's chain.  10 at every B of BATCHES (chains 101 .. 117); 18.5, 19.1 and 18.6 at the three WALKS (chains 388, 420, 420)."""
    c = chain_mfma(B)
    return MARGIN if c <= 162 else max(MARGIN, c / (6.0 + math.log2(B)))


assert learner_ref.chain(2125) == 162   # (the chain MARGIN was rounded for)
