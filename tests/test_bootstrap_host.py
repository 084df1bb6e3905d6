"""The bootstrap term of truncated steps, what needs no GPU: ppo.gae(..., boot=b) against a float64 per-env recursion of

    delta_t = r_t + gamma ((1 - done_t) V_{t+1} + boot_t) - V_t ,   A_t = delta_t + gamma lam (1 - done_t) A_{t+1}

with episode boundaries and truncated steps placed by hand.  Tolerance as tests/test_gpu_gae.py: 1e-5 * max(1, |A|max)."""
import inspect

import numpy as np
import torch


def ref_f64(rew, val, done, boot, gamma, lam, scale=1.0):
    T, N = rew.shape
    adv = np.zeros((T, N))
    last = np.zeros(N)
    for t in reversed(range(T)):
        nt = 1.0 - done[t].astype(np.float64)
        delta = scale * rew[t].astype(np.float64) + gamma * (nt * val[t + 1].astype(np.float64) + boot[t].astype(np.float64)) - val[t]
        last = delta + gamma * lam * nt * last
        adv[t] = last
    return adv, adv + val[:T]


def hand_placed(T, N, seed):
    """random rewards / values; terminations and truncations placed by hand: env 0 is truncated on step 0, env 1 on the last step, env 2
    on both and in between, env 3 terminates where env 2 is truncated, env 4 never ends, the rest draw 5 % terminations and 5 %
    truncations per step.  boot = a random value on the truncated steps, 0 elsewhere."""
    rng = np.random.RandomState(seed)
    rew = rng.normal(size=(T, N)).astype(np.float32)
    val = rng.normal(size=(T + 1, N)).astype(np.float32)
    term = rng.uniform(size=(T, N)) < 0.05
    trunc = (rng.uniform(size=(T, N)) < 0.05) & ~term
    term[:, :5] = False
    trunc[:, :5] = False
    trunc[0, 0] = True
    trunc[T - 1, 1] = True
    trunc[[0, T // 2, T - 1], 2] = True
    term[[0, T // 2, T - 1], 3] = True
    done = (term | trunc).astype(np.uint8)
    boot = np.where(trunc, rng.normal(size=(T, N)), 0.0).astype(np.float32)
    return rew, val, done, boot, trunc


def test_torch_gae_with_the_bootstrap_term_matches_the_float64_recursion():
    from gym_reinmav_amd.ppo import gae

    assert "boot" in inspect.signature(gae).parameters
    gamma, lam = 0.99, 0.95
    for T, N in ((1, 8), (7, 63), (33, 257), (64, 1000)):
        rew, val, done, boot, trunc = hand_placed(T, N, T + N)
        assert trunc[0, 0] and trunc[T - 1, 1] and trunc.sum() >= 3
        r, v, d, b = (torch.from_numpy(x) for x in (rew, val, done, boot))
        adv, ret = gae(r, v, d, gamma, lam, boot=b)
        exp_a, exp_r = ref_f64(rew, val, done, boot, gamma, lam)
        tol = 1e-5 * max(1.0, np.abs(exp_a).max())
        assert np.abs(adv.numpy() - exp_a).max() < tol and np.abs(ret.numpy() - exp_r).max() < tol
        # the term matters: without it the truncated steps' targets differ by gamma * boot
        a0, r0 = gae(r, v, d, gamma, lam)
        assert np.abs((ret - r0).numpy()[trunc] - gamma * boot[trunc]).max() < tol
        # boot = None and boot = zeros are the function without the term, exactly
        az, rz = gae(r, v, d, gamma, lam, boot=torch.zeros_like(r))
        an, rn = gae(r, v, d, gamma, lam, boot=None)
        assert torch.equal(az, a0) and torch.equal(rz, r0) and torch.equal(an, a0) and torch.equal(rn, r0)


def test_a_truncated_step_targets_r_plus_gamma_v_final():
    """lam = 1: the return target of a truncated step is exactly r + gamma * boot, whatever follows it"""
    from gym_reinmav_amd.ppo import gae

    T, N, gamma = 12, 16, 0.9
    rng = np.random.RandomState(3)
    rew = torch.from_numpy(rng.normal(size=(T, N)).astype(np.float32))
    val = torch.from_numpy(rng.normal(size=(T + 1, N)).astype(np.float32))
    done = torch.zeros((T, N), dtype=torch.uint8)
    boot = torch.zeros((T, N))
    done[5] = 1
    boot[5] = 2.0
    _, ret = gae(rew, val, done, gamma, 1.0, boot=boot)
    assert torch.allclose(ret[5], rew[5] + gamma * 2.0, atol=1e-6)
    _, ret0 = gae(rew, val, done, gamma, 1.0)
    assert torch.allclose(ret0[5], rew[5], atol=1e-6)
