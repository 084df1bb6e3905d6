"""Frame skip, the Python layer without a GPU: `frame_skip` is validated before the library is reached, and the keyword reaches every
constructor that takes it - BatchedQuadrotor, QuadrotorVecEnv, registration.make (the gym-shaped classes), make_sharded and the
example's --frame-skip.  The library is replaced by a recorder: no handle is ever created."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Recorder:
    """Stands in for librmav.so: every entry point returns RMAV_OK; rmav_set_frame_skip / rmav_get_frame_skip keep the value."""

    def __init__(self):
        self.calls = []
        self.k = 1

    def __getattr__(self, name):
        def f(*a):
            self.calls.append(name)
            if name == "rmav_set_frame_skip":
                self.k = int(a[1].value if hasattr(a[1], "value") else a[1])
            if name == "rmav_get_frame_skip":
                a[1]._obj.value = self.k
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


@pytest.mark.parametrize("bad", [0, -1, 1025, 2 ** 31])
def test_out_of_range_is_refused_before_the_library(rec, bad):
    import gym_reinmav_amd as g

    with pytest.raises(ValueError):
        g.BatchedQuadrotor("quad3d", 4, frame_skip=bad)
    assert rec.calls == []


@pytest.mark.parametrize("bad", [2.0, 2.5, "2", None, True, np.float32(2)])
def test_non_integers_are_refused_before_the_library(rec, bad):
    import gym_reinmav_amd as g

    with pytest.raises(TypeError):
        g.BatchedQuadrotor("quad3d", 4, frame_skip=bad)
    assert rec.calls == []


def test_the_setter_validates_too(rec):
    import gym_reinmav_amd as g

    env = g.BatchedQuadrotor("quad3d", 4, frame_skip=np.int64(3))
    assert rec.k == 3 and env.frame_skip == 3
    n = rec.calls.count("rmav_set_frame_skip")
    for bad, exc in ((0, ValueError), (1025, ValueError), (1.0, TypeError)):
        with pytest.raises(exc):
            env.frame_skip = bad
    assert rec.calls.count("rmav_set_frame_skip") == n and rec.k == 3
    env.frame_skip = 1
    assert rec.k == 1
    env._h = None


def test_the_default_never_calls_the_setter(rec):
    import gym_reinmav_amd as g

    env = g.BatchedQuadrotor("quad3d", 4)
    assert "rmav_set_frame_skip" not in rec.calls
    env._h = None


def test_the_keyword_reaches_every_constructor(rec, monkeypatch):
    import gym_reinmav_amd as g
    from gym_reinmav_amd import distributed, registration
    from gym_reinmav_amd.vec_env import QuadrotorVecEnv

    made = []
    for make in (lambda: g.BatchedQuadrotor("quad2d", 4, frame_skip=2),
                 lambda: QuadrotorVecEnv("quadrotor3d-v0", 4, frame_skip=3, numpy_io=True),
                 lambda: registration.make("quadrotor3d-v0", frame_skip=4),
                 lambda: registration.make("quadrotor2d-v0", frame_skip=5),
                 lambda: registration.make("quadrotor2d-slungload-v0", frame_skip=6),
                 lambda: registration.make("quadrotor3d-slungload-v0", frame_skip=7),
                 lambda: distributed.make_sharded("quad3d", 8, 0, 2, device=0, frame_skip=8)):
        rec.k = 1
        made.append(make())
        assert rec.k == len(made) + 1, len(made)
    assert made[1].env.frame_skip == rec.k and made[2].frame_skip == rec.k
    with pytest.raises(ValueError):
        registration.make("quadrotor3d-v0", frame_skip=0)
    with pytest.raises(TypeError):
        QuadrotorVecEnv("quadrotor3d-v0", 4, frame_skip=1.5)
    for m in made:   # (nothing to destroy)
        getattr(m, "env", getattr(m, "_batch", m))._h = None
        if hasattr(m, "_hnd"):
            m._hnd = None


def test_the_gym_class_steps_without_step_control_on_such_an_env(rec):
    """rmav_step_control has no frame-skip kernel: the gym-shaped class calls rmav_step, and control() a launch of its own."""
    from gym_reinmav_amd import registration

    env = registration.make("quadrotor3d-v0", frame_skip=2)
    rec.calls.clear()
    env.step(np.zeros(4))
    assert "rmav_step" in rec.calls and "rmav_step_control" not in rec.calls
    env.control()
    assert "rmav_control" in rec.calls
    env.frame_skip = 1
    rec.calls.clear()
    env.step(np.zeros(4))
    assert "rmav_step_control" in rec.calls and "rmav_step" not in rec.calls
    env._batch._h = env._hnd = None


def test_the_example_has_the_flag():
    src = open(os.path.join(ROOT, "examples", "train_ppo2.py")).read()
    assert '"--frame-skip"' in src and src.count("frame_skip=args.frame_skip") == 2


def test_prototypes():
    from gym_reinmav_amd import _abi as A

    assert A.PROTOTYPES["rmav_set_frame_skip"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert A.PROTOTYPES["rmav_get_frame_skip"][1][1] == C.POINTER(C.c_int32)
