"""The policy action rule and the evaluation helpers, what needs no GPU: first_episode_stats against a plain Python loop (an env that
never finishes, an env done at t = 0, chunked use against one-shot use), and the argument validation of the Python setters."""
import math

import numpy as np
import pytest


def _loop(rew, done):
    """Per env: add rewards in step order (fp32) up to and including the first done."""
    T, N = rew.shape
    ret, ln, fin = np.zeros(N, np.float32), np.zeros(N, np.int64), np.zeros(N, bool)
    for i in range(N):
        for t in range(T):
            ret[i] = np.float32(ret[i] + rew[t, i])
            ln[i] += 1
            if done[t, i]:
                fin[i] = True
                break
    return ret, ln, fin


def _case(T=37, N=53, seed=0):
    rng = np.random.RandomState(seed)
    rew = rng.normal(size=(T, N)).astype(np.float32)
    done = (rng.uniform(size=(T, N)) < 0.08).astype(np.uint8)
    done[:, 0] = 0          # never finishes
    done[0, 1] = 1          # done at t = 0 ...
    done[5, 1] = 1          # ... and again later: only the first episode counts
    done[:, 2] = 0
    done[T - 1, 2] = 1      # finishes with the last step
    return rew, done


def test_first_episode_stats_equals_the_python_loop(built):
    import torch
    from gym_reinmav_amd.evaluate import first_episode_stats

    rew, done = _case()
    ret, ln, fin = first_episode_stats(torch.from_numpy(rew), torch.from_numpy(done))
    r0, l0, f0 = _loop(rew, done)
    assert ret.dtype == torch.float32 and fin.dtype == torch.bool and ret.shape == ln.shape == fin.shape == (rew.shape[1],)
    assert np.array_equal(ret.numpy(), r0) and np.array_equal(ln.numpy(), l0) and np.array_equal(fin.numpy(), f0)
    assert not f0[0] and l0[0] == rew.shape[0]                     # the env that never finishes: its running values
    assert f0[1] and l0[1] == 1 and r0[1] == rew[0, 1]             # done at t = 0
    assert f0[2] and l0[2] == rew.shape[0]
    assert 3 < f0.sum() < f0.size
    # a bool done array is the same thing
    again = first_episode_stats(torch.from_numpy(rew), torch.from_numpy(done.astype(bool)))
    assert all(torch.equal(a, b) for a, b in zip(again, (ret, ln, fin)))


@pytest.mark.parametrize("chunk", [1, 5, 36, 64])
def test_first_episode_stats_chunk_by_chunk_equals_one_shot(built, chunk):
    import torch
    from gym_reinmav_amd.evaluate import first_episode_stats

    rew, done = (torch.from_numpy(x) for x in _case(seed=3))
    whole = first_episode_stats(rew, done)
    carry = None
    for s in range(0, rew.shape[0], chunk):
        nxt = first_episode_stats(rew[s:s + chunk], done[s:s + chunk], carry)
        if carry is not None:   # the carry is not modified in place
            assert all(a is not b for a, b in zip(nxt, carry))
        carry = nxt
    assert all(torch.equal(a, b) for a, b in zip(carry, whole))


def test_policy_action_rule_arguments(built):
    from gym_reinmav_amd.core import policy_action_rule as rule

    inf = math.inf
    box = lambda: (0.0, 10.0)  # noqa: E731
    assert rule(False, None) == (0, -inf, inf) and rule(False, False) == (0, -inf, inf)
    assert rule(True, True, box) == (1, 0.0, 10.0)
    assert rule(np.bool_(True), (-1, 1)) == (1, -1.0, 1.0) and rule(0, [2.0, 2.0]) == (0, 2.0, 2.0)
    assert rule(False, (-inf, 3.0)) == (0, -inf, 3.0)
    for det, clip in ((2, None), ("yes", None), (None, None), (False, (1.0, 0.0)), (False, (float("nan"), 1.0)), (False, (0.0, float("nan"))),
                      (False, (1.0,)), (False, (1.0, 2.0, 3.0)), (False, "ab"), (False, 3.0)):
        with pytest.raises(ValueError):
            rule(det, clip, box)
    with pytest.raises(ValueError):
        rule(False, True)   # clip=True without an action space


def test_evaluate_policy_needs_a_horizon(built):
    from gym_reinmav_amd.evaluate import evaluate_policy

    class NoLimit:
        max_episode_steps = None

    with pytest.raises(ValueError, match="n_steps"):
        evaluate_policy(None, NoLimit())
    with pytest.raises(ValueError):
        evaluate_policy(None, NoLimit(), n_steps=0)
