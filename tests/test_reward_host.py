"""Tracking reward, the Python layer without a GPU: bad specs are refused before the library is reached, the keyword reaches every
constructor that takes it (BatchedQuadrotor, QuadrotorVecEnv, registration.make, make_sharded, the example's --reward), the defaults
resolve as documented, and the fp64 restatement the GPU tests use (tests/reward_ref.py) is itself checked - against a hand-written
evaluation and against four mutants that must leave the bar.  The library is replaced by a recorder: no handle is ever created."""
import ctypes as C
import os

import numpy as np
import pytest

import reward_ref as R
from util import KINDS, NA, NS, TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fill_params(p, kind):
    """The constants the resolution reads, as rmav_default_params leaves them."""
    p.mass, p.thrust_scale = (0.6 if kind in (0, 1) else 1.0), (2.0 if kind in (0, 1) else 1.0)
    p.g_vec[0], p.g_vec[1], p.g_vec[2] = (0.0, -9.8, 0.0) if kind in (0, 1) else (0.0, 0.0, -9.8)
    p.ref_pos[0], p.ref_pos[1], p.ref_pos[2] = (0.0, 1.0, 0.0) if kind in (0, 1) else (0.0, 0.0, 2.0)


class _Recorder:
    """Stands in for librmav.so: every entry point returns RMAV_OK; rmav_set_reward / rmav_get_reward keep the spec, rmav_create the
    params."""

    def __init__(self):
        self.calls, self.spec, self.on, self.params = [], None, 0, None

    def __getattr__(self, name):
        def f(*a):
            from gym_reinmav_amd import _abi as A

            self.calls.append(name)
            if name == "rmav_default_params":
                _fill_params(a[2]._obj, a[0])
            if name == "rmav_create":
                self.params = A.Params.from_buffer_copy(a[7]._obj)
            if name == "rmav_get_params":
                C.memmove(C.addressof(a[1]._obj), C.addressof(self.params), C.sizeof(A.Params))
            if name == "rmav_set_reward":
                self.on = int(a[1] is not None)
                if a[1] is not None:
                    self.spec = A.RewardSpec.from_buffer_copy(a[1]._obj)
            if name == "rmav_get_reward":
                if self.spec is not None:
                    C.memmove(C.addressof(a[1]._obj), C.addressof(self.spec), C.sizeof(A.RewardSpec))
                a[2]._obj.value = self.on
            if name == "rmav_get_frame_skip":
                a[1]._obj.value = 1
            return 0
        return f


@pytest.fixture
def rec(monkeypatch):
    from gym_reinmav_amd import _abi as A
    from gym_reinmav_amd import core

    r = _Recorder()
    monkeypatch.setattr(A, "lib", lambda: r)
    monkeypatch.setattr(core, "torch", None)
    return r


def _spec_tuple(s):
    return (tuple(s.goal), s.alive, s.w_pos, s.w_vel, s.w_act, tuple(s.act_ref), s.terminal)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(alive=float("nan")), dict(w_pos=float("inf")), dict(terminal=-float("inf")), dict(goal=(0, float("nan"), 1)),
                                dict(act_ref=(1.0, float("inf"))), dict(w_vel=1e39), dict(goal=(1, 2, 3, 4)), dict(goal=(1,)), dict(goal=()),
                                dict(act_ref=(1, 2, 3)), dict(act_ref=(1, 2, 3, 4, 5))])
def test_bad_values_and_lengths_are_value_errors(rec, kw):
    import gym_reinmav_amd as g

    with pytest.raises(ValueError):
        g.TrackingReward(**kw)
    assert rec.calls == []


@pytest.mark.parametrize("kw", [dict(alive="1"), dict(goal="012"), dict(goal=2.0), dict(act_ref="abcd"), dict(w_act=None), dict(w_pos=True),
                                dict(goal=(0, "1", 2)), dict(terminal=[1.0])])
def test_wrong_types_are_type_errors(rec, kw):
    import gym_reinmav_amd as g

    with pytest.raises(TypeError):
        g.TrackingReward(**kw)
    assert rec.calls == []


@pytest.mark.parametrize("bad", ["goal=0,0,2", 1.0, {"goal": (0, 0, 2)}, (0, 0, 2)])
def test_the_keyword_takes_a_tracking_reward_or_none(rec, bad):
    import gym_reinmav_amd as g

    with pytest.raises(TypeError):
        g.BatchedQuadrotor("quad3d", 4, reward=bad)
    assert rec.calls == []


def test_lengths_are_checked_against_the_kind_before_the_library(rec):
    import gym_reinmav_amd as g

    for kind, kw in (("quad3d", dict(goal=(0, 1))), ("quad3d_sl", dict(act_ref=(1, 0))), ("quad3d", dict(goal=(0, 1), act_ref=(1, 0)))):
        with pytest.raises(ValueError):
            g.BatchedQuadrotor(kind, 4, reward=g.TrackingReward(**kw))
    assert rec.calls == []
    env = g.BatchedQuadrotor("quad2d", 4, reward=g.TrackingReward(goal=(0.5, 1), act_ref=(3, 0.5)))
    assert _spec_tuple(rec.spec) == ((0.5, 1.0, 0.0), 0.0, 1.0, 0.0, 0.0, (3.0, 0.5, 0.0, 0.0), 0.0)
    env._h = None


def test_the_setter_validates_and_none_switches_off(rec):
    import gym_reinmav_amd as g

    env = g.BatchedQuadrotor("quad3d", 4)
    assert "rmav_set_reward" not in rec.calls and env.reward is None
    env.reward = g.TrackingReward(goal=(1, 2, 3), alive=0.5, w_pos=2, w_vel=0.25, w_act=0.125, act_ref=(4, 3, 2, 1), terminal=-7)
    assert rec.on == 1 and _spec_tuple(rec.spec) == ((1.0, 2.0, 3.0), 0.5, 2.0, 0.25, 0.125, (4.0, 3.0, 2.0, 1.0), -7.0)
    got = env.reward
    assert (got.goal, got.alive, got.w_pos, got.w_vel, got.w_act, got.act_ref, got.terminal) == _spec_tuple(rec.spec)
    n = rec.calls.count("rmav_set_reward")
    for bad in ("alive=1", 3, g.TrackingReward(goal=(1, 2))):
        with pytest.raises((TypeError, ValueError)):
            env.reward = bad
    assert rec.calls.count("rmav_set_reward") == n and rec.on == 1
    env.reward = None
    assert rec.on == 0 and env.reward is None
    env._h = None


# ---- the keyword -------------------------------------------------------------------------------------------------------------------
def test_the_keyword_reaches_every_constructor(rec):
    import gym_reinmav_amd as g
    from gym_reinmav_amd import distributed, registration
    from gym_reinmav_amd.vec_env import QuadrotorVecEnv

    made = []
    for i, make in enumerate((lambda r: g.BatchedQuadrotor("quad2d", 4, reward=r),
                              lambda r: QuadrotorVecEnv("quadrotor3d-v0", 4, reward=r, numpy_io=True),
                              lambda r: registration.make("quadrotor3d-v0", reward=r),
                              lambda r: registration.make("quadrotor2d-v0", reward=r),
                              lambda r: registration.make("quadrotor2d-slungload-v0", reward=r),
                              lambda r: registration.make("quadrotor3d-slungload-v0", reward=r),
                              lambda r: distributed.make_sharded("quad3d", 8, 0, 2, device=0, reward=r))):
        rec.spec, rec.on = None, 0
        made.append(make(g.TrackingReward(alive=float(i + 1))))
        assert rec.on == 1 and rec.spec.alive == i + 1, i
    assert made[1].env.reward.alive == 7.0 and made[2].reward.alive == 7.0
    with pytest.raises(TypeError):
        registration.make("quadrotor3d-v0", reward="goal=0,0,2")
    with pytest.raises(TypeError):
        QuadrotorVecEnv("quadrotor3d-v0", 4, reward=1.5)
    for m in made:   # (nothing to destroy)
        getattr(m, "env", getattr(m, "_batch", m))._h = None
        if hasattr(m, "_hnd"):
            m._hnd = None


def test_the_examples_parser():
    import subprocess
    import sys

    import gym_reinmav_amd as g

    # the example hands --reward to TrackingReward.parse before it creates an env: a bad spec ends it as a usage error
    ex = os.path.join(ROOT, "examples", "train_ppo2.py")
    bad = subprocess.run([sys.executable, ex, "--num_timesteps", "0", "--reward", "speed=1"], capture_output=True, text=True)
    assert bad.returncode == 2 and "--reward" in bad.stderr and "speed=1" in bad.stderr, (bad.returncode, bad.stderr[-400:])
    r = g.TrackingReward.parse("goal=0,0,2:alive=1:w_pos=1:w_vel=0.1:w_act=0.01:terminal=-10")
    assert (r.goal, r.alive, r.w_pos, r.w_vel, r.w_act, r.act_ref, r.terminal) == ((0.0, 0.0, 2.0), 1.0, 1.0, 0.1, 0.01, None, -10.0)
    assert g.TrackingReward.parse("act_ref=9.8,0,0,0").act_ref == (9.8, 0.0, 0.0, 0.0) and g.TrackingReward.parse("").w_pos == 1.0
    for bad in ("goal", "goal=a,b", "speed=1", "alive=1:alive=2", "alive=1,2", "goal=1,2,3,4", "w_pos=nan"):
        with pytest.raises((TypeError, ValueError)):
            g.TrackingReward.parse(bad)
    with pytest.raises(TypeError):
        g.TrackingReward.parse(None)


# ---- the defaults ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_none_resolves_to_the_set_point_and_the_hover_action(rec, kind):
    import gym_reinmav_amd as g
    from gym_reinmav_amd import _abi as A

    k = A.KIND_BY_NAME[kind]
    p = A.Params()
    _fill_params(p, k)
    p.mass, p.thrust_scale = 0.75, 1.5
    s = g.TrackingReward().spec(k, p)
    assert tuple(s.goal) == tuple(np.float32(x) for x in p.ref_pos)
    hover = np.float32(0.75 * 9.8 / 1.5)
    assert tuple(s.act_ref) == (hover, 0.0, 0.0, 0.0)
    assert (s.alive, s.w_pos, s.w_vel, s.w_act, s.terminal) == (0.0, 1.0, 0.0, 0.0, 0.0)
    # ... through the constructor, from the handle's params
    env = g.BatchedQuadrotor(kind, 4, reward=g.TrackingReward(w_act=0.5))
    pp = rec.params
    assert tuple(rec.spec.goal) == tuple(np.float32(x) for x in pp.ref_pos) and rec.spec.act_ref[0] == np.float32(pp.mass * 9.8 / pp.thrust_scale)
    env._h = None
    p.thrust_scale = 0.0
    with pytest.raises(ValueError):
        g.TrackingReward().spec(k, p)
    with pytest.raises(ValueError):
        g.TrackingReward().spec(A.REINMAV, p)


def test_prototypes():
    from gym_reinmav_amd import _abi as A

    assert A.PROTOTYPES["rmav_set_reward"] == (C.c_int, [C.c_void_p, C.POINTER(A.RewardSpec)])
    assert A.PROTOTYPES["rmav_get_reward"] == (C.c_int, [C.c_void_p, C.POINTER(A.RewardSpec), C.POINTER(C.c_int32)])
    assert [f[0] for f in A.RewardSpec._fields_] == ["goal", "alive", "w_pos", "w_vel", "w_act", "act_ref", "terminal"]


def test_the_collector_refuses_the_actors_without_a_kernel(rec):
    """The fp32 vector-ALU and bf16 actors have no tracking-reward kernel: refused in the constructor, before any launch."""
    import gym_reinmav_amd as g
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    class Policy:   # (the constructor reads .shared and .obs_norm before the refusal, nothing else)
        shared, obs_norm = False, None

    env = g.BatchedQuadrotor("quad3d", 4, reward=g.TrackingReward(act_ref=(9.8, 0, 0, 0)))
    for kw in (dict(bf16_mfma=True), dict(f32_mfma=False)):
        rec.calls.clear()
        with pytest.raises(ValueError, match="tracking-reward"):
            FusedPolicyCollector(env, Policy(), 4, **kw)
        assert not [c for c in rec.calls if "rollout" in c or "pack" in c]
    env._h = None


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _case(kind, n=64, seed=5):
    rng = np.random.RandomState(seed)
    s = rng.uniform(-2, 2, (n, NS[kind])).astype(np.float32)
    u = rng.uniform(-3, 3, (n, NA[kind])).astype(np.float32)
    term = np.arange(n) % 4 == 0
    return s, u, term


@pytest.mark.parametrize("kind", KINDS)
def test_reward_ref_against_a_hand_written_evaluation(kind):
    s, u, term = _case(kind)
    r, M = R.reward_ref(kind, s, u, R.SPEC, term)
    s64, u64 = s.astype(np.float64), u.astype(np.float64)
    g3, a4 = np.float32(R.SPEC["goal"]).astype(np.float64), np.float32(R.SPEC["act_ref"]).astype(np.float64)
    if kind in ("quad2d", "quad2d_sl"):
        d, v = np.linalg.norm(s64[:, 0:2] - g3[:2], axis=1), np.linalg.norm(s64[:, 3:5], axis=1)
        c = np.linalg.norm(u64 - a4[:2], axis=1) ** 2
    elif kind == "quad3d":
        d, v = np.linalg.norm(s64[:, 0:3] - g3, axis=1), np.linalg.norm(s64[:, 7:10], axis=1)
        c = np.linalg.norm(u64 - a4, axis=1) ** 2
    else:
        d, v = np.linalg.norm(s64[:, 10:13] - g3, axis=1), np.linalg.norm(s64[:, 13:16], axis=1)
        c = np.linalg.norm(u64 - a4, axis=1) ** 2
    live = 1.5 - 2.0 * d - 0.25 * v - 0.125 * c
    np.testing.assert_allclose(r[~term], live[~term], rtol=1e-13, atol=1e-13)
    assert (r[term] == -7.0).all() and term.any() and (~term).any()
    np.testing.assert_allclose(M, 1.5 + 2.0 * d + 0.25 * v + 0.125 * c, rtol=1e-13)


def _leaves_the_bar(kind, r_mutant, s, u, term):
    r, M = R.reward_ref(kind, s, u, R.SPEC, term)
    return bool((np.abs(r_mutant - r) > TOL * np.maximum(1.0, M)).any())


def test_mutants_of_the_restatement_leave_the_bar():
    """Each on inputs where it matters: had the kernels made the mistake, the arithmetic test (same bar) would catch it."""
    sp = R.f32(R.SPEC)
    g3, a4 = np.asarray(sp["goal"]), np.asarray(sp["act_ref"])
    live = lambda d, v, c: sp["alive"] - sp["w_pos"] * d - sp["w_vel"] * v - sp["w_act"] * c   # noqa: E731
    # 1. the wrong body for quadrotor3d-slungload: the quadrotor (s[0:3], s[7:10]) instead of the load
    s, u, term = _case("quad3d_sl")
    term[:] = False
    s64, u64 = s.astype(np.float64), u.astype(np.float64)
    c = ((u64 - a4) ** 2).sum(axis=1)
    wrong = live(np.linalg.norm(s64[:, 0:3] - g3, axis=1), np.linalg.norm(s64[:, 7:10], axis=1), c)
    assert _leaves_the_bar("quad3d_sl", wrong, s, u, term)
    # 2. the velocity norm squared
    s, u, term = _case("quad3d")
    term[:] = False
    s64, u64 = s.astype(np.float64), u.astype(np.float64)
    c = ((u64 - a4) ** 2).sum(axis=1)
    wrong = live(np.linalg.norm(s64[:, 0:3] - g3, axis=1), (s64[:, 7:10] ** 2).sum(axis=1), c)
    assert _leaves_the_bar("quad3d", wrong, s, u, term)
    # 3. the unclipped action: the dynamics took clip(u, -0.5, 0.5), the mutant is given u
    clipped = np.clip(u, -0.5, 0.5)
    assert (clipped != u).any()
    wrong, _ = R.reward_ref("quad3d", s, u, R.SPEC, term)
    assert _leaves_the_bar("quad3d", wrong, s, clipped, term)
    # 4. the terminal step given r_live
    term = np.arange(len(s)) % 4 == 0
    wrong, _ = R.reward_ref("quad3d", s, u, R.SPEC, np.zeros(len(s), bool))
    assert _leaves_the_bar("quad3d", wrong, s, u, term)
    # ... and the restatement itself stays inside it
    right, _ = R.reward_ref("quad3d", s, u, R.SPEC, term)
    assert not _leaves_the_bar("quad3d", right, s, u, term)
