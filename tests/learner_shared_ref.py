"""The oracle and the inputs of the shared-trunk fused-learner tests (rmav_ppo_grad_shared, csrc/rmav_learner_shared.hpp): the
counterpart of learner_ref.py for an ``MlpPolicy(value_network="shared")`` - one 2 x 64 trunk, the mean head ``pi.2`` and the scalar
value head ``vf.0`` on its latent.

* ``oracle``: ``PPO.loss`` on a ``.double()`` copy of the policy on the CPU with autograd -> the flat gradient in the ABI order of
  include/rmav_ppo.h (9 tensors), the four statistics, and the three clearance distances learner_ref.py defines.
* ``restate``: what the kernel computes, by hand in fp64 numpy - ONE forward, the two heads, the summed delta of the trunk - with
  switches for the arithmetic mutants the host test uses: learner_ref's seven and two that cut one head's delta off the trunk.
* ``make_case`` / ``trained_policy``: the inputs the GPU test and the host test share; built as learner_ref's, from the fp64 SHARED
  policy's outputs, with one more mode (``both_clipped``).
* ``margin``: MARGIN for the chains profiles/r23/learner.md rounded it for, the chain-length rule evaluated for a longer one.

SEED was chosen before any GPU run, on the CPU (profiles/r24/learner_shared.md): among seeds 0..7 the one whose one-element tensor
``vf.0.bias`` - the sum of per-sample terms that may cancel - has the mildest worst cancellation sum|d_j| / |sum d_j| over every
(kind, B, statistics) case the GPU test draws."""
import math

import numpy as np
import torch

from learner_ref import BATCHES, CLEAR, CLIP, FLOOR, KINDS, MARGIN, VF_COEF, TableNorm, _excluding, adv_moments, make_norm  # noqa: F401

NAMES = tuple(f"pi.{k}.{w}" for k in range(3) for w in ("weight", "bias")) + ("vf.0.weight", "vf.0.bias", "logstd")
NET = NAMES[:8]   # the eight tensors of the net (everything but logstd)
SEED = 3   # (worst cancellation 77; the other seven: 206 .. 2906)
MODES = ("mixed", "pg_clipped", "vf_clipped", "both_clipped")


def chain(B):
    """the longest run of sequential roundings of a kernel sum: 64 over K, 64 per tile and tile after tile in a thread, then the
    workgroups' partials one after the other"""
    tiles = -(-B // 64)
    return 64 + 64 * -(-tiles // 512) + min(tiles, 512)


def margin(B):
    """The factor of the bound err(kernel) <= margin(B) * max(err(torch fp32), FLOOR).  profiles/r23/learner.md rounds MARGIN = 10 for
    every chain up to the 162 roundings of its largest shape, B = 2125; that holds here unchanged: 10 for every B of BATCHES.  (The
    quotient itself, evaluated with a full tile for the small batches, would be wider there - 21.5 at B = 1 - and is NOT used.)  A
    longer chain gets the quotient the rule rounds: the kernel's chain over the shortest a blocked or pairwise sum can have,
    log2 64 + log2 B: 704 / 21.0 = 33.5 at B = 32 833."""
    return MARGIN if chain(B) <= 162 else max(MARGIN, chain(B) / (6.0 + math.log2(B)))


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


def policy64(kind, seed, norm=None):
    pol = trained_policy(kind, seed, norm).double()
    if norm is not None:
        pol.obs_norm = norm.to(dtype=torch.float64)
    return pol


def make_case(kind, B, seed, norm=None, mode="mixed", clip=CLIP):
    """fp32 CPU inputs of one minibatch for ``trained_policy(kind, seed, norm)``: dict(obs [nS, B], act [nA, B], logp_old, val_old, adv,
    ret [B]).  ``mode``: 'mixed' (ratios over [0.5, 2] with both advantage signs, |v - val_old| on both sides of the clip, both vf
    branches), 'pg_clipped' (every sample's clipped surrogate branch strictly active), 'vf_clipped' (v_clip's branch active everywhere
    with |v - val_old| > clip), 'both_clipped' (both at once: no gradient reaches the net)."""
    assert mode in MODES
    nS, nA = KINDS[kind]
    g = torch.Generator().manual_seed(6000 + 7 * seed + B)
    pol = policy64(kind, seed, norm)
    obs = torch.randn(nS, B, generator=g).float()
    with torch.no_grad():
        mean, v = pol(obs.double())
        act = (mean + torch.exp(pol.logstd)[:, None] * torch.randn(nA, B, generator=g, dtype=torch.float64)).float()
        logp = pol.log_prob(mean, act.double())
    adv = torch.randn(B, generator=g, dtype=torch.float64) * 1.5 + 0.3
    pg_cut, vf_cut = mode in ("pg_clipped", "both_clipped"), mode in ("vf_clipped", "both_clipped")
    if pg_cut:   # ratio well outside the range on the side that clips for the sample's advantage sign
        a_sign = torch.sign(adv - adv.float().mean().double()) if B > 1 else torch.sign(adv)
        up = 1.0 + clip + 0.1 + 0.6 * torch.rand(B, generator=g, dtype=torch.float64)
        down = 1.0 - clip - 0.1 - 0.3 * torch.rand(B, generator=g, dtype=torch.float64)
        ratio = torch.where(a_sign > 0, up, down)
    else:
        ratio = torch.exp(_excluding(g, B, math.log(0.5), math.log(2.0), (math.log(1 - clip), math.log(1 + clip)), 0.02))
        ratio[0] = 1.0 + 0.25 * clip   # sample 0 sits inside both clips, so that a batch of one has a gradient in every tensor
    logp_old = (logp - torch.log(ratio)).float()
    sign = torch.where(torch.rand(B, generator=g) < 0.5, -1.0, 1.0).double()
    if vf_cut:
        d = sign * (clip + 0.05 + 0.35 * torch.rand(B, generator=g, dtype=torch.float64))
    else:
        d = sign * _excluding(g, B, 0.0, 3 * clip, (clip,), 0.05)
        d[0] = sign[0] * 0.5 * clip
    val_old = (v - d).float()
    # ret: a margin m away from the midpoint of v and v_clip; beyond v_clip's side the clipped term is the larger one
    vc = val_old.double() + torch.clamp(v - val_old.double(), -clip, clip)
    m = 0.05 + 0.95 * torch.rand(B, generator=g, dtype=torch.float64)
    side = torch.sign(d) if vf_cut else torch.where(torch.rand(B, generator=g) < 0.5, -1.0, 1.0).double()
    ret = (0.5 * (v + vc) + side * m).float()   # vf_cut: ret on v's side of the midpoint, so v_clip is the farther one
    return dict(obs=obs, act=act, logp_old=logp_old, val_old=val_old, adv=adv.float(), ret=ret)


def flat_grad(pol):
    named = dict(pol.named_parameters())
    return torch.cat([named[n].grad.reshape(-1) for n in NAMES])


def slices(kind):
    """{name: slice of the flat gradient}"""
    nS, nA = KINDS[kind]
    sizes = [64 * nS, 64, 4096, 64, 64 * nA, nA, 64, 1, nA]
    out, o = {}, 0
    for n, s in zip(NAMES, sizes):
        out[n] = slice(o, o + s)
        o += s
    return out


def torch_learner(pol, case, clip=CLIP, vf_coef=VF_COEF, ent_coef=0.0):
    """PPO.loss + backward on the shared-trunk ``pol`` (any dtype / device; the case is moved to it) -> (flat grad, [loss, pg, vf, max
    ratio]) as fp64 numpy.  A single sample (its std is NaN) goes through PPO.loss's expressions with the raw advantage
    (learner_ref.adv_moments)."""
    from gym_reinmav_amd.ppo import PPO

    assert pol.shared
    p0 = next(pol.parameters())
    c = {k: v.to(device=p0.device, dtype=p0.dtype) for k, v in case.items()}
    ppo = PPO(pol, clip=clip, vf_coef=vf_coef, ent_coef=ent_coef)
    pol.zero_grad(set_to_none=True)
    if c["adv"].numel() < 2:
        a = c["adv"]
        mean, v = pol(c["obs"])
        ratio = torch.exp(pol.log_prob(mean, c["act"]) - c["logp_old"])
        pg = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
        v_clip = c["val_old"] + torch.clamp(v - c["val_old"], -clip, clip)
        vf = 0.5 * torch.max((v - c["ret"]) ** 2, (v_clip - c["ret"]) ** 2).mean()
        loss = pg + vf_coef * vf - ent_coef * pol.entropy()
    else:
        loss, pg, vf, ratio = ppo.loss(c["obs"], c["act"], c["logp_old"], c["val_old"], c["adv"], c["ret"])
    loss.backward()
    stats = np.array([float(loss.detach()), float(pg.detach()), float(vf.detach()), float(ratio.detach().max())])
    named = dict(pol.named_parameters())
    for n in NAMES:   # a tensor no gradient reaches (both heads clipped) has none in autograd: the kernel writes its zeros
        if named[n].grad is None:
            named[n].grad = torch.zeros_like(named[n])
    return flat_grad(pol).detach().double().cpu().numpy(), stats


def oracle(kind, seed, case, norm=None, clip=CLIP, vf_coef=VF_COEF, ent_coef=0.0):
    """-> (flat gradient fp64, stats fp64 [4], clearances dict) of PPO.loss on the .double() CPU policy with autograd"""
    pol = policy64(kind, seed, norm)
    grad, stats = torch_learner(pol, case, clip, vf_coef, ent_coef)
    with torch.no_grad():
        c = {k: v.double() for k, v in case.items()}
        mean, v = pol(c["obs"])
        ratio = torch.exp(pol.log_prob(mean, c["act"]) - c["logp_old"])
        d = (v - c["val_old"]).abs()
        vc = c["val_old"] + torch.clamp(v - c["val_old"], -clip, clip)
        gap = ((v - c["ret"]) ** 2 - (vc - c["ret"]) ** 2).abs()[d > clip]
        clear = {"ratio": float(torch.minimum((ratio - (1 - clip)).abs(), (ratio - (1 + clip)).abs()).min()),
                 "vclip": float((d - clip).abs().min()),
                 "vf_terms": float(gap.min()) if gap.numel() else math.inf}
    return grad, stats, clear


# ---- the restatement: what the kernel computes, by hand, in fp64 ---------------------------------------------------------------------
MUTANTS = ("no_inv_b", "no_tanh_prime", "clip_wrong_side", "no_value_clip", "raw_adv", "no_vf_coef", "ent_sign",
           "value_skips_trunk", "policy_skips_trunk")


def params64(pol):
    named = dict(pol.named_parameters())
    return [named[n].detach().double().cpu().numpy().copy() for n in NAMES]


def restate(P, case, norm=None, clip=CLIP, vf_coef=VF_COEF, ent_coef=0.0, mutant=None, parts=False):
    """P: the 9 fp64 arrays in the ABI order -> (flat gradient, stats [loss, pg, vf, max ratio]).  ``parts=True``: also the per-sample
    value delta d_v [B] (the terms of vf.0.bias)."""
    assert mutant is None or mutant in MUTANTS
    W1, b1, W2, b2, W3, b3, wv, bv, logstd = P
    c = {k: v.double().numpy() for k, v in case.items()}
    x = c["obs"]
    if norm is not None:
        x = np.clip((x - norm.mean_f.double().numpy()[:, None]) * norm.rstd_f.double().numpy()[:, None], -norm.clip_f, norm.clip_f)
    B = x.shape[1]
    inv_b = 1.0 if mutant == "no_inv_b" else 1.0 / B
    nA = logstd.size
    # one forward, two heads
    h1 = np.tanh(W1 @ x + b1[:, None])
    h2 = np.tanh(W2 @ h1 + b2[:, None])
    mean = W3 @ h2 + b3[:, None]
    v = (wv @ h2 + bv[:, None])[0]
    # the policy term
    inv_std = np.exp(-logstd)[:, None]
    z = (c["act"] - mean) * inv_std
    logp = -0.5 * (z * z).sum(0) - logstd.sum() - 0.5 * nA * math.log(2 * math.pi)
    ratio = np.exp(logp - c["logp_old"])
    if mutant == "raw_adv":
        a = c["adv"]
    else:
        m = c["adv"].mean() if B > 1 else 0.0
        rstd = 1.0 / (c["adv"].std(ddof=1) + 1e-8) if B > 1 else 1.0
        a = (c["adv"] - m) * rstd
    lo, hi = 1.0 - clip, 1.0 + clip
    t1, t2 = -a * ratio, -a * np.clip(ratio, lo, hi)
    inside = (ratio >= lo) & (ratio <= hi)
    if mutant == "clip_wrong_side":   # min instead of max: the surrogate keeps the gradient where PPO cuts it
        pg_s = np.minimum(t1, t2)
        g_ratio = np.where((t1 < t2) | inside, -a, 0.0)
    else:
        pg_s = np.maximum(t1, t2)
        g_ratio = np.where((t1 > t2) | ((t1 == t2) & inside), -a, np.where(t1 == t2, -0.5 * a, 0.0))
    gl = g_ratio * ratio * inv_b
    d_mean = gl[None, :] * z * inv_std
    g_logstd = (gl[None, :] * (z * z - 1.0)).sum(1) + (ent_coef if mutant == "ent_sign" else -ent_coef)
    # the value term
    dv = v - c["val_old"]
    vc = c["val_old"] + np.clip(dv, -clip, clip)
    u1, u2 = v - c["ret"], vc - c["ret"]
    e1, e2 = u1 * u1, u2 * u2
    ins = (dv >= -clip) & (dv <= clip)
    if mutant == "no_value_clip":
        vf_s, gv = e1, 2.0 * u1
    else:
        vf_s = np.maximum(e1, e2)
        gv = np.where(e1 > e2, 2.0 * u1, np.where(e1 < e2, np.where(ins, 2.0 * u2, 0.0), u1 + np.where(ins, u2, 0.0)))
    d_v = ((1.0 if mutant == "no_vf_coef" else vf_coef) * 0.5 * gv * inv_b)[None, :]
    # the trunk gets the sum of both heads' deltas
    back = (0.0 if mutant == "policy_skips_trunk" else W3.T @ d_mean) + (0.0 if mutant == "value_skips_trunk" else wv.T @ d_v)
    d2 = back * (1.0 if mutant == "no_tanh_prime" else (1.0 - h2 * h2))
    d1 = (W2.T @ d2) * (1.0 - h1 * h1)
    grads = [d1 @ x.T, d1.sum(1), d2 @ h1.T, d2.sum(1), d_mean @ h2.T, d_mean.sum(1), d_v @ h2.T, d_v.sum(1), g_logstd]
    pg, vf = pg_s.mean(), 0.5 * vf_s.mean()
    ent = (logstd + 0.5 * math.log(2 * math.pi * math.e)).sum()
    stats = np.array([pg + vf_coef * vf - ent_coef * ent, pg, vf, ratio.max()])
    flat = np.concatenate([t.reshape(-1) for t in grads])
    return (flat, stats, d_v[0]) if parts else (flat, stats)


def tensor_errors(kind, g, g64):
    """{name: max|g - g64| / max|g64|} per parameter tensor"""
    out = {}
    for n, s in slices(kind).items():
        ref = np.abs(g64[s]).max()
        assert ref > 0, n   # (the exact-zero cases are compared bit for bit, not through this)
        out[n] = float(np.abs(g[s] - g64[s]).max() / ref)
    return out
