"""The oracle and the inputs of the shared-trunk fused-learner tests (rmav_ppo_grad_shared, csrc/rmav_learner_shared.hpp): the
counterpart of learner_ref.py for an ``MlpPolicy(value_network="shared")`` - one 2 x 64 trunk, the mean head ``pi.2`` and the scalar
value head ``vf.0`` on its latent.

* ``oracle``: ``PPO.loss`` on a ``.double()`` copy of the policy on the CPU with autograd -> the flat gradient in the ABI order of
  include/rmav_ppo.h (9 tensors), the four statistics, and the three clearance distances learner_ref.py defines.
* ``restate``: what the kernel computes, by hand in fp64 numpy - ONE forward, the two heads, the summed delta of the trunk - with
  switches for the arithmetic mutants the host test uses: learner_ref's seven and two that cut one head's delta off the trunk.
* ``make_case`` / ``trained_policy``: the inputs the GPU test and the host test share; built as learner_ref's, from the fp64 SHARED
  policy's outputs, with one more mode (``both_clipped``).
Everything but ``trained_policy`` and ``restate`` IS learner_ref's function, called with this module's ``ARCH`` record; ``chain`` and
``margin`` (one tile walk, one rule for both learners) are re-exported from there.

SEED was chosen before any GPU run, on the CPU (profiles/r24/learner_shared.md): among seeds 0..7 the one whose one-element tensor
``vf.0.bias`` - the sum of per-sample terms that may cancel - has the mildest worst cancellation sum|d_j| / |sum d_j| over every
(kind, B, statistics) case the GPU test draws."""
import math
from functools import partial

import numpy as np
import torch

import learner_ref as R
from learner_ref import (BATCHES, CLEAR, CLIP, FLOOR, HYPER_BATCHES, HYPER_KINDS, HYPERS, KINDS, MARGIN, VF_COEF, WALKS, TableNorm,  # noqa: F401
                         adv_moments, chain, make_norm, margin)

NAMES = tuple(f"pi.{k}.{w}" for k in range(3) for w in ("weight", "bias")) + ("vf.0.weight", "vf.0.bias", "logstd")
NET = NAMES[:8]   # the eight tensors of the net (everything but logstd)
SEED = 3   # (worst cancellation 77; the other seven: 206 .. 2906)
MODES = ("mixed", "pg_clipped", "vf_clipped", "both_clipped")


def trained_policy(kind, seed, norm=None):
    """An fp32 CPU shared-trunk MlpPolicy with trained-looking weights: non-zero biases, a pi.2 gain that does not hide W3's path (the
    default init's is 0.01) and a value head whose output is of order 1."""
    from gym_reinmav_amd.ppo import MlpPolicy

    nS, nA = KINDS[kind]
    g = torch.Generator().manual_seed(5000 + seed)
    pol = MlpPolicy(nS, nA, value_network="shared", obs_norm=norm)
    with torch.no_grad():
        for k, lin in enumerate(pol.pi):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * (0.6 / math.sqrt(lin.in_features) if k < 2 else 0.12))
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
        pol.vf[0].weight.copy_(torch.randn(pol.vf[0].weight.shape, generator=g) * 0.25)
        pol.vf[0].bias.copy_(torch.randn(1, generator=g) * 0.1)
        pol.logstd.copy_(torch.rand(nA, generator=g) * 0.8 - 0.5)
    return pol


# learner_ref's functions for this architecture (same signatures: the record is their last, keyword argument)
ARCH = R.Arch(NAMES, lambda nS, nA: [64 * nS, 64, 4096, 64, 64 * nA, nA, 64, 1, nA], 6000, trained_policy, MODES, True)
policy64, make_case, flat_grad, slices, torch_learner, oracle, params64, tensor_errors = (
    partial(f, arch=ARCH) for f in (R.policy64, R.make_case, R.flat_grad, R.slices, R.torch_learner, R.oracle, R.params64, R.tensor_errors))

# ---- the restatement: what the kernel computes, by hand, in fp64 ---------------------------------------------------------------------
MUTANTS = R.MUTANTS + ("value_skips_trunk", "policy_skips_trunk")


def restate(P, case, norm=None, clip=CLIP, vf_coef=VF_COEF, ent_coef=0.0, mutant=None, parts=False):
    """P: the 9 fp64 arrays in the ABI order -> (flat gradient, stats [loss, pg, vf, max ratio]).  ``parts=True``: also the per-sample
    value delta d_v [B] (the terms of vf.0.bias)."""
    assert mutant is None or mutant in MUTANTS
    W1, b1, W2, b2, W3, b3, wv, bv, logstd = P
    c, x, inv_b = R.inputs64(case, norm, mutant)
    # one forward, two heads
    h1 = np.tanh(W1 @ x + b1[:, None])
    h2 = np.tanh(W2 @ h1 + b2[:, None])
    mean = W3 @ h2 + b3[:, None]
    v = (wv @ h2 + bv[:, None])[0]
    pg_s, ratio, d_mean, g_logstd = R.policy_term(c, mean, logstd, inv_b, clip, ent_coef, mutant)
    vf_s, d_v = R.value_term(c, v, inv_b, clip, vf_coef, mutant)
    # the trunk gets the sum of both heads' deltas
    back = (0.0 if mutant == "policy_skips_trunk" else W3.T @ d_mean) + (0.0 if mutant == "value_skips_trunk" else wv.T @ d_v)
    d2 = back * (1.0 if mutant == "no_tanh_prime" else (1.0 - h2 * h2))
    d1 = (W2.T @ d2) * (1.0 - h1 * h1)
    grads = [d1 @ x.T, d1.sum(1), d2 @ h1.T, d2.sum(1), d_mean @ h2.T, d_mean.sum(1), d_v @ h2.T, d_v.sum(1), g_logstd]
    flat, stats = np.concatenate([t.reshape(-1) for t in grads]), R.loss_stats(pg_s, vf_s, ratio, logstd, vf_coef, ent_coef)
    return (flat, stats, d_v[0]) if parts else (flat, stats)
