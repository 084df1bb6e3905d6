"""fp64 restatement of the tracking reward (rmav_set_reward, include/rmav.h) for the reward tests.  The spec is a dict with the keys of
rmav_reward_spec: goal (3), alive, w_pos, w_vel, w_act, act_ref (4), terminal; the 2-D kinds read goal[0:2] and act_ref[0:2]."""
import numpy as np

# kind -> (position slice, velocity slice) of the tracked body: the one whose distance the reference rewards
BODY = {"quad2d": (slice(0, 2), slice(3, 5)), "quad2d_sl": (slice(0, 2), slice(3, 5)),
        "quad3d": (slice(0, 3), slice(7, 10)), "quad3d_sl": (slice(10, 13), slice(13, 16))}
NA = {"quad2d": 2, "quad2d_sl": 2, "quad3d": 4, "quad3d_sl": 4}

# the spec the GPU tests run
SPEC = dict(goal=(0.3, -0.2, 0.5), alive=1.5, w_pos=2.0, w_vel=0.25, w_act=0.125, act_ref=(0.5, 0.1, -0.1, 0.2), terminal=-7.0)
# ... and the one whose live reward is the reference's -dist
REFERENCE = dict(goal=(0.0, 0.0, 0.0), alive=0.0, w_pos=1.0, w_vel=0.0, w_act=0.0, act_ref=(0.0, 0.0, 0.0, 0.0), terminal=0.25)


def f32(spec):
    """The spec as the kernels hold it: every value rounded to fp32 (returned as fp64 numbers)."""
    return {k: (tuple(float(np.float32(x)) for x in v) if isinstance(v, (tuple, list)) else float(np.float32(v))) for k, v in spec.items()}


def reward_ref(kind, s_post, u, spec, term):
    """s_post [n, nS]: the stored post-step state; u [n, nA]: the action handed to the dynamics; term [n] bool -> (r [n], M [n]) in fp64,
    M = |alive| + w_pos d + w_vel v + w_act c: the magnitude the fp32 roundings of r_live scale with."""
    s_post, u = np.asarray(s_post, np.float64), np.asarray(u, np.float64)
    sp = f32(spec)
    ps, vs = BODY[kind]
    dim, na = ps.stop - ps.start, NA[kind]
    d = np.sqrt(((s_post[:, ps] - np.asarray(sp["goal"][:dim])) ** 2).sum(axis=1))
    v = np.sqrt((s_post[:, vs] ** 2).sum(axis=1))
    c = ((u[:, :na] - np.asarray(sp["act_ref"][:na])) ** 2).sum(axis=1)
    live = sp["alive"] - sp["w_pos"] * d - sp["w_vel"] * v - sp["w_act"] * c
    M = abs(sp["alive"]) + abs(sp["w_pos"]) * d + abs(sp["w_vel"]) * v + abs(sp["w_act"]) * c
    return np.where(np.asarray(term, bool), sp["terminal"], live), M
