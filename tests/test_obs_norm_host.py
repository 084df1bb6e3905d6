"""RunningObsNorm on CPU tensors (the torch float64 form of the update rule the kernels implement) against a NumPy float64
restatement of baselines' RunningMeanStd / VecNormalize (third party; restated from memory, as include/rmav_ppo.h does)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinmav-gym_amd"))


class RefRunningMeanStd:
    """baselines.common.running_mean_std.RunningMeanStd + VecNormalize._obfilt, NumPy float64"""

    def __init__(self, n, epsilon=1e-4):
        self.mean, self.var, self.count = np.zeros(n), np.ones(n), epsilon

    def update(self, x):   # x [B, n]
        x = np.asarray(x, np.float64)
        bm, bv, bc = x.mean(0), x.var(0), x.shape[0]
        d = bm - self.mean
        tot = self.count + bc
        self.mean = self.mean + d * bc / tot
        self.var = (self.var * self.count + bv * bc + d * d * self.count * bc / tot) / tot
        self.count = tot

    def normalise(self, x, clipob=10.0, eps=1e-8):
        return np.clip((np.asarray(x, np.float64) - self.mean) / np.sqrt(self.var + eps), -clipob, clipob)


def check_against_ref(norm_mean, norm_var, norm_count, ref, n_seen):
    """count exact; mean within 4 n 2^-53 relative to max(|mean|, std), var within the same relative to var"""
    tol = 4.0 * n_seen * 2.0 ** -53
    assert norm_count == ref.count, (norm_count, ref.count)
    e_mean = np.abs(norm_mean - ref.mean) / np.maximum(np.abs(ref.mean), np.sqrt(ref.var))
    e_var = np.abs(norm_var - ref.var) / ref.var
    print(f"n={n_seen} mean err {e_mean.max():.3e} var err {e_var.max():.3e} bound {tol:.3e}")
    assert e_mean.max() <= tol and e_var.max() <= tol, (e_mean.max(), e_var.max(), tol)


def _batches(ns, seed=0):
    """Uneven batches, the first of one row.  Conditioned like the envs' observations (per-feature spread 0.4 .. 5, |mean| up to twice
    the spread: the oracle's rollouts have variances >= 0.2 and magnitudes <= 5.3).  The bound above is the rounding of a pairwise
    merge; it does not model the cancellation in (batch mean - running mean) that |mean| >> std would add on top - an error of
    2^-53 |mean| in that difference enters the variance with a factor |mean| / std, for ANY fp64 implementation, the restatement
    included."""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.4, 5.0, ns)
    shift = rng.uniform(-2.0, 2.0, ns) * scale
    return [(rng.standard_normal((b, ns)) * scale + shift).astype(np.float32) for b in (1, 6, 1024, 3969, 15000, 12768)]


@pytest.mark.parametrize("ns", [5, 9, 10, 16])
def test_running_obs_norm_matches_the_numpy_restatement(ns):
    from gym_reinmav_amd.obs_norm import RunningObsNorm

    norm, ref, seen = RunningObsNorm(ns), RefRunningMeanStd(ns), 0
    assert norm.count == 1e-4 and np.array_equal(norm.mean, np.zeros(ns)) and np.array_equal(norm.var, np.ones(ns))
    assert torch.equal(norm.mean_f, torch.zeros(ns)) and torch.equal(norm.rstd_f, torch.ones(ns)) and float(norm.clip_f) == 10.0
    for i, b in enumerate(_batches(ns)):
        if i % 2 == 0:   # feature-major [nS, B], what the rollouts store
            norm.update(torch.from_numpy(b.T.copy()), layout="soa")
        else:
            norm.update(torch.from_numpy(b), layout="aos")
        ref.update(b)
        seen += b.shape[0]
        check_against_ref(norm.mean, norm.var, norm.count, ref, seen)
    # tables: one rounding of the fp64 state
    assert np.array_equal(norm.mean_f.numpy(), norm.mean.astype(np.float32))
    assert np.array_equal(norm.rstd_f.numpy(), (1.0 / np.sqrt(norm.var + 1e-8)).astype(np.float32))
    # normalise: the fp32 expression against the float64 restatement, three roundings
    x = _batches(ns, seed=1)[3]
    z = norm.normalize(torch.from_numpy(x), layout="aos").numpy()
    zr = ref.normalise(x)
    rstd = 1.0 / np.sqrt(ref.var + 1e-8)
    bound = 4 * 2.0 ** -24 * (np.abs(zr) + (np.abs(x) + np.abs(ref.mean)) * rstd)
    assert (np.abs(z - zr) <= bound).all(), float((np.abs(z - zr) / bound).max())
    assert np.abs(z).max() <= 10.0
    zt = norm.normalize(torch.from_numpy(x.T.copy()), layout="soa").numpy()
    assert np.array_equal(zt.T, z)


def test_freeze_state_dict_and_refusals():
    from gym_reinmav_amd.obs_norm import RunningObsNorm
    from gym_reinmav_amd.ppo import MlpPolicy
    from gym_reinmav_amd.vec_env import VecNormalize

    a = RunningObsNorm(10, clip=5.0, eps=1e-6, count0=1e-2)
    for b in _batches(10)[:4]:
        a.update(torch.from_numpy(b), layout="aos")
    sd = a.state_dict()
    b_ = RunningObsNorm(10)
    ptr = b_.data_ptr()
    b_.load_state_dict(sd)
    assert b_.data_ptr() == ptr, "loaded in place: the pointer the kernels hold stays valid"
    assert torch.equal(a.buf, b_.buf) and b_.clip == 5.0 and b_.eps == 1e-6 and b_.count == a.count
    assert np.array_equal(a.mean, b_.mean) and np.array_equal(a.var, b_.var)
    assert torch.equal(a.mean_f, b_.mean_f) and torch.equal(a.rstd_f, b_.rstd_f) and torch.equal(a.clip_f, b_.clip_f)
    nxt = torch.from_numpy(_batches(10)[4])
    a.update(nxt, layout="aos")
    b_.update(nxt, layout="aos")
    assert torch.equal(a.buf, b_.buf)
    b_.freeze = True
    before = b_.buf.clone()
    b_.update(nxt, layout="aos")
    assert torch.equal(b_.buf, before)
    with pytest.raises(ValueError):
        RunningObsNorm(10).load_state_dict(RunningObsNorm(9).state_dict())
    with pytest.raises(ValueError, match="ret"):
        VecNormalize(None, ret=True)
    with pytest.raises(ValueError):
        MlpPolicy(9, 2, obs_norm=RunningObsNorm(10))
    with pytest.raises(ValueError):
        RunningObsNorm(17)


@pytest.mark.parametrize("vn", ["copy", "shared"])
def test_policy_normalises_first_and_keeps_gradients_out_of_the_statistics(vn):
    from gym_reinmav_amd.obs_norm import RunningObsNorm
    from gym_reinmav_amd.ppo import MlpPolicy

    torch.manual_seed(0)
    norm = RunningObsNorm(10, clip=1.0)
    raw = torch.from_numpy(_batches(10)[2].T.copy())
    norm.update(raw, layout="soa")
    plain = MlpPolicy(10, 4, value_network=vn)
    pol = MlpPolicy(10, 4, value_network=vn, obs_norm=norm)
    pol.load_state_dict(plain.state_dict())
    z = torch.clamp((raw - norm.mean_f[:, None]) * norm.rstd_f[:, None], -1.0, 1.0)
    share = float(((z == 1.0) | (z == -1.0)).float().mean())
    assert 0.1 < share < 0.9, share   # the clip binds
    m0, v0 = plain(z)
    m1, v1 = pol(raw)
    assert torch.equal(m0, m1) and torch.equal(v0, v1)
    (m1.sum() + v1.sum()).backward()
    assert all(p.grad is not None for n, p in pol.named_parameters() if n != "logstd") and not norm.buf.requires_grad


def test_ppo_update_absorbs_the_rollout_after_the_last_minibatch():
    """frozen statistics: PPO.update learns with the statistics it was handed and merges obs[:T] afterwards"""
    import types

    from gym_reinmav_amd.obs_norm import RunningObsNorm
    from gym_reinmav_amd.ppo import PPO, MlpPolicy

    NS, NA, T, N = 10, 4, 6, 48
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ro = types.SimpleNamespace(obs=3.0 + 2.0 * r(T + 1, NS, N), act=r(T, NA, N), logp=-4.0 + 0.3 * r(T, N), val=r(T + 1, N), rew=r(T, N),
                               done=(torch.rand(T, N, generator=g) < 0.1).to(torch.uint8), env=None)
    norm, ref = RunningObsNorm(NS), RefRunningMeanStd(NS)
    pol = MlpPolicy(NS, NA, obs_norm=norm)
    seen_tables = []
    orig = norm.normalize
    norm.normalize = lambda *a, **k: (seen_tables.append(norm.mean_f.clone()), orig(*a, **k))[1]
    PPO(pol, epochs=2, minibatches=2).update(ro)
    assert len(seen_tables) == 4 and all(torch.equal(t, torch.zeros(NS)) for t in seen_tables), "statistics moved while learning"
    ref.update(ro.obs[:T].permute(0, 2, 1).reshape(-1, NS).numpy())
    check_against_ref(norm.mean, norm.var, norm.count, ref, T * N)
    assert norm.count == 1e-4 + T * N


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_batch(rank):
    return _batches(10, seed=7 + rank)[2 + rank]   # different sizes and contents per rank


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, os.path.join(ROOT, "reinmav-gym_amd"))
    import torch.distributed as dist

    from gym_reinmav_amd.obs_norm import RunningObsNorm

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    norm = RunningObsNorm(10)
    norm.update(torch.from_numpy(_rank_batch(rank)), layout="aos")
    np.save(os.path.join(out_dir, f"buf_{rank}.npy"), norm.buf.numpy())
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_data_parallel_update_world2(tmp_path):
    """two ranks with different batches end with bit-identical statistics, equal to one process that saw them in rank order"""
    from gym_reinmav_amd.obs_norm import RunningObsNorm

    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    b0, b1 = np.load(tmp_path / "buf_0.npy"), np.load(tmp_path / "buf_1.npy")
    assert np.array_equal(b0, b1)
    one = RunningObsNorm(10)
    for r in range(2):
        one.update(torch.from_numpy(_rank_batch(r)), layout="aos")
    assert np.array_equal(one.buf.numpy(), b0)
    assert one.count == 1e-4 + _rank_batch(0).shape[0] + _rank_batch(1).shape[0]
