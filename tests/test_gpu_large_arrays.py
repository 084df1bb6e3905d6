"""Trajectory addressing at and beyond 4 GiB per array.

Every kernel that writes a trajectory (act / obs / rew / done, time-major) addresses it with raw buffer instructions: 32-bit offsets, range
check off.  Three mechanisms keep that right, and each is run here at the sizes where it matters:
  - the lean / generic switch of the two-wavefront kernels (launch_rollout_kms: F_LEAN while n_steps * nS * pitch < 2^30) - the lean drain's
    32-bit step offsets up to one row short of 2^32, the first launch on the generic side, rows that start beyond 4 GiB;
  - the 64-bit cursors of the one-wavefront kernels (all eight feature families), of the fused = 0 host loop, of the chunk-major slices and of
    the in-kernel actors;
  - the in-step column offset c * 4 * pitch, which is why a column pitch is bounded like num_envs (2^25).

A column pitch can be chosen freely while N stays tiny, so 130 envs put a trajectory row beyond 4 GiB: the launches take microseconds and only
the allocation is large.  Groups A, B, D, E compare rmav_rollout_pitched into caller-allocated arrays with a second fresh handle of the same
configuration rolled out in the plain layout (pitch = N, a few KB - the path the oracle and golden tests pin), bit for bit, on the device.
Every large array is filled with a sentinel bit pattern first; afterwards the number of elements that differ from the sentinel over the WHOLE
array must equal that number inside [..., :N]: a store that wrapped into another column of the caller's allocation is caught, not only an
overrun.  Group C runs real batch sizes without a pitch and compares every element with the same rollout cut into short launches.

Nothing here has a tolerance of its own: rollouts are compared bit for bit, group D reuses the bound of tests/test_gpu_obs_norm.py.
No test holds more than 10 GiB of device memory (the largest are about 9 GB); no large array is copied to the host."""
import ctypes as C

import numpy as np
import pytest

import disturbance_ref as DR
import start_ref as SR
from test_gpu_actuator import INIT, TAUS, commands
from test_gpu_disturbance import ACTORS, dist, policy_of, same, tracking
from test_gpu_obs_norm import _check_moments, _moments, _stats_from_a_rollout
from test_gpu_start_state import start_of
from util import KINDS, NA, NS

pytestmark = pytest.mark.gpu

N = 130                      # two full wavefronts and a ragged one of 2 envs
SEED, BASE = 11, 300
BIG_KINDS = ("quad2d", "quad3d_sl")      # nS = 5 with paired action draws, and the widest state (nS = 16)
SENT = 0x7FC12345            # a quiet NaN with a payload: compared as int32, so that NaN payloads count
SENT_U8 = 0xA5
GIB = 1 << 30
MAX_PITCH = 1 << 25


def pitch_for(dim):
    """the smallest multiple of 64 with 16 * dim * P >= 2^30: 16 steps of a [dim][P] fp32 array reach 4 GiB"""
    return -(-(1 << 26) // (dim * 64)) * 64


P_OBS = {kind: pitch_for(NS[kind]) for kind in KINDS}
P_ACT = {kind: pitch_for(NA[kind]) for kind in KINDS}
assert P_OBS["quad2d"] == 13421824 and P_OBS["quad3d_sl"] == 4194304 and P_ACT["quad2d"] == MAX_PITCH


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gym_reinmav_amd as g

    yield g
    torch.cuda.empty_cache()   # the module's multi-GB blocks go back to the device when it ends


@pytest.fixture(autouse=True)
def room(G):
    """A test may skip only when the device has less than 12 GiB left (blocks the caching allocator holds unused count as free)."""
    import torch

    def free():
        return torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()

    if free() < 12 * GIB:
        torch.cuda.empty_cache()
    if free() < 12 * GIB:
        pytest.skip(f"torch.cuda.mem_get_info() reports {torch.cuda.mem_get_info()[0] / GIB:.1f} GiB free: these tests need 12 GiB")


# ---- helpers -----------------------------------------------------------------------------------------------------------------------------------
def bits(x):
    import torch

    return x.view(torch.int32) if x.dtype == torch.float32 else x


def same_bits(a, b, what):
    import torch

    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert torch.equal(bits(a), bits(b)), what


def filled(shape, u8=False):
    import torch

    if u8:
        return torch.full(shape, SENT_U8, dtype=torch.uint8, device="cuda")
    return torch.full(shape, SENT, dtype=torch.int32, device="cuda").view(torch.float32)


def written(arr):
    """Elements of arr [T, ...] whose bits differ from the sentinel: over the whole array - one time row at a time, so that no temporary
    exceeds 1 GiB - and inside [..., :N].  -> two device scalars"""
    import torch

    b = bits(arr)
    sent = SENT_U8 if arr.dtype == torch.uint8 else SENT
    whole = torch.zeros((), dtype=torch.int64, device=arr.device)
    for t in range(b.shape[0]):
        whole += (b[t] != sent).sum()
    return whole, (b[..., :N] != sent).sum()


def sentinel_problems(arrays):
    """The sentinel count of every array: as many elements differ from the sentinel over the whole array as inside [..., :N] (nothing
    was stored into the padding, by an overrun or by a wrapped column or step offset), and inside [..., :N] all of them do (every element
    was stored: no output has the sentinel's bits - a NaN with a payload, 0xA5 for a done byte).  -> a list of complaints"""
    import torch

    counts = {key: written(v) + (v[..., :N].numel(),) for key, v in arrays.items() if v is not None}
    torch.cuda.synchronize()
    out = []
    for key, (whole, view, full) in counts.items():
        if int(whole) != int(view):
            out.append(f"sentinel count, {key}: {int(whole)} elements differ from the sentinel, {int(view)} of them inside [..., :N]")
        if int(view) != full:
            out.append(f"sentinel count, {key}: {full - int(view)} of {full} elements of [..., :N] were never stored")
    return out


def same_handles(env, ref, what):
    same(env.get_state(), ref.get_state(), what + ": state")
    same(env.get_reset_counts(), ref.get_reset_counts(), what + ": reset counts")
    same(env.get_sbd(), ref.get_sbd(), what + ": steps beyond done")
    assert env.episode_totals() == ref.episode_totals(), what
    assert env.step_count == ref.step_count, what
    if env.actuator is not None:
        same(env.actuator_state(), ref.actuator_state(), what + ": actuator state")


def handle(G, kind, n=N, tune=None, **kw):
    env = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE, auto_reset=True, track_episodes=True, **kw)
    if tune:
        env.set_tuning(**tune)
    return env


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def pitched_run(G, kind, mode, T, P, features=None, tune=None, fused=True, obs_out=True, keep=False):
    """One rmav_rollout_pitched launch of T steps at column pitch P into sentinel-filled arrays, against the same handle configuration in the
    plain layout: values, handle state, and the sentinel count.  keep=True: -> (env, obs) for a test that goes on with the large array."""
    import torch
    from gym_reinmav_amd import _abi as A

    features = features or (lambda: {})
    nS, nA = NS[kind], NA[kind]
    buffer = mode == "buffer"
    acts = None
    if buffer:   # commands that end episodes inside the launch
        acts = torch.from_numpy(np.ascontiguousarray(commands(kind, N, T).transpose(0, 2, 1))).cuda()
    want = ("actions", "rew", "done") + (("obs",) if obs_out else ())
    ref_env = handle(G, kind, tune=tune, **features())
    ref = ref_env.rollout(T, mode=mode, actions=acts, layout="soa", fused=fused, want=want, device_out=True)
    env = handle(G, kind, tune=tune, **features())
    big = {"a_in": None, "actions": None, "obs": filled((T, nS, P)) if obs_out else None, "rew": filled((T, P)),
           "done": filled((T, P), u8=True)}
    if buffer:
        big["a_in"] = filled((T, nA, P))
        big["a_in"][..., :N] = acts
    else:
        big["actions"] = filled((T, nA, P))
    A.check(env._lib.rmav_rollout_pitched(env._h, T, {"buffer": A.ACT_BUFFER, "random": A.ACT_RANDOM, "controller": A.ACT_CONTROLLER}[mode],
                                          ptr(big["a_in"]), ptr(big["actions"]), ptr(big["obs"]), ptr(big["rew"]), ptr(big["done"]), P,
                                          1 if fused else 0))
    torch.cuda.synchronize()
    what = f"{kind} {mode} T={T} P={P}"
    problems = []   # (both checks are always made, so that a failure shows what each of them saw)
    for key in want:
        src = big["a_in"] if (key == "actions" and buffer) else big[key]
        assert src[..., :N].shape == ref[key].shape and src.dtype == ref[key].dtype, key
        if not torch.equal(bits(src[..., :N]), bits(ref[key])):
            rows = (bits(src[..., :N]) != bits(ref[key])).flatten(1).any(1).nonzero().flatten().tolist()
            problems.append(f"values, {key}: steps {rows} differ from the plain layout")
    problems += sentinel_problems(big)
    assert not problems, (what, problems)
    same_handles(env, ref_env, what)
    if buffer:
        assert bool(ref["done"].any()), "the commands end episodes inside the launch"
    ref_env.close()
    if keep:
        return env, big["obs"]
    env.close()
    return None


# ---- A. the lean / generic switch of the two-wavefront kernels, and the one-wavefront kernels of a handle without features ----------------------
# T = 15: lean, the last obs row ends just under 2^32 and the scalar step offset crosses 2^31; T = 16: the first launch on the generic side;
# T = 20: rows 16 - 19 start beyond 4 GiB
@pytest.mark.parametrize("T", (15, 16, 20))
@pytest.mark.parametrize("mode", ("random", "buffer", "controller"))
@pytest.mark.parametrize("kind", BIG_KINDS)
def test_two_wavefront_rollouts_around_the_switch(G, kind, mode, T):
    P = P_OBS[kind]
    assert (T * NS[kind] * P < GIB) == (T == 15) and 15 * NS[kind] * P * 4 > 1 << 31
    pitched_run(G, kind, mode, T, P)


@pytest.mark.parametrize("kind", BIG_KINDS)
def test_an_odd_pitch_beyond_4_gib(G, kind):
    """P + 1: the dword store paths (a pitch that is no multiple of 4 misaligns the 16-byte stores)"""
    pitched_run(G, kind, "random", 20, P_OBS[kind] + 1)


@pytest.mark.parametrize("store_policy", (0, 1, 2))
@pytest.mark.parametrize("kind", BIG_KINDS)
def test_one_wavefront_rollouts_beyond_4_gib(G, kind, store_policy):
    pitched_run(G, kind, "random", 20, P_OBS[kind], tune=dict(split=0, store_policy=store_policy))


@pytest.mark.parametrize("kind", BIG_KINDS)
def test_single_step_launches_with_host_side_step_pointers_beyond_4_gib(G, kind):
    pitched_run(G, kind, "buffer", 20, P_OBS[kind], fused=False)


@pytest.mark.parametrize("kind", BIG_KINDS)
def test_caller_actions_read_beyond_4_gib(G, kind):
    """no observations: the action array is the wide one, and act_in itself is read beyond 4 GiB"""
    P = P_ACT[kind]
    assert 16 * NA[kind] * P >= GIB and P <= MAX_PITCH
    pitched_run(G, kind, "buffer", 20, P, obs_out=False)


# ---- B. every feature family: separate instantiations of the one-wavefront body ------------------------------------------------------------------
FAMILIES = {
    "tl": lambda G, kind: dict(max_episode_steps=5),
    "dr": lambda G, kind: dict(randomize={"mass": (0.8, 1.2)}),
    "fs": lambda G, kind: dict(frame_skip=3),
    "rw": lambda G, kind: dict(reward=tracking(G)),
    "ds": lambda G, kind: dict(disturbance=dist(G, DR.SPEC)),
    "sn": lambda G, kind: dict(sensor_noise=G.SensorNoise(0.25)),
    "al": lambda G, kind: dict(actuator=G.Actuator(TAUS[NA[kind]], init=INIT[NA[kind]])),
    "ss": lambda G, kind: dict(start_state=start_of(G, SR.ranges(kind))),
}


@pytest.mark.parametrize("mode", ("random", "buffer"))
@pytest.mark.parametrize("family", tuple(FAMILIES))
@pytest.mark.parametrize("kind", BIG_KINDS)
def test_every_feature_family_beyond_4_gib(G, kind, family, mode):
    pitched_run(G, kind, mode, 20, P_OBS[kind], features=lambda: FAMILIES[family](G, kind))


# ---- C. real batch sizes, no pitch: every element of a > 4 GiB array against the same rollout in short launches ----------------------------------
C_KIND, C_N, C_T, C_PIECE = "quad3d_sl", 65536, 1040, 130
WANT = ("actions", "obs", "rew", "done")


def pieces(T, step):
    return [(t0, min(T, t0 + step)) for t0 in range(0, T, step)]


def same_totals(env, ref, what):
    """launches of different lengths: the counts exactly (return_sum is a sum of per-launch partial sums, grouped differently)"""
    a, b = env.episode_totals(), ref.episode_totals()
    assert a["episodes"] == b["episodes"] > 0 and a["length_sum"] == b["length_sum"], (what, a, b)
    same(env.get_state(), ref.get_state(), what + ": state")
    same(env.get_reset_counts(), ref.get_reset_counts(), what + ": reset counts")
    same(env.get_sbd(), ref.get_sbd(), what + ": steps beyond done")


@pytest.mark.parametrize("split", (1, 0))
@pytest.mark.parametrize("layout", ("soa", "aos"))
def test_a_real_batch_beyond_4_gib_equals_short_launches(G, layout, split):
    """65 536 quadrotor3d-slungload envs x 1040 steps: obs is 4.36 GB, feature-major [T, nS, N] and batch-major [T, N, nS] (there the row
    pointer dst_step + li * nS and the bounded per-wavefront descriptors); the reference is the same handle in 8 launches of 130 steps
    (tests/test_gpu_parity.py pins that launches of different lengths join bit for bit)."""
    import torch

    env = handle(G, C_KIND, C_N, tune=dict(split=split))
    tr = env.rollout(C_T, mode="random", layout=layout, want=WANT, device_out=True)
    assert tr["obs"].numel() * 4 > 4 * GIB
    ref_env = handle(G, C_KIND, C_N)
    for t0, t1 in pieces(C_T, C_PIECE):
        ref = ref_env.rollout(t1 - t0, mode="random", layout="soa", want=WANT, device_out=True)
        for key in WANT:
            got = tr[key][t0:t1]
            if layout == "aos" and key in ("actions", "obs"):
                got = got.permute(0, 2, 1)
            same_bits(got, ref[key], f"{layout} split={split} steps [{t0}, {t1}): {key}")
        del ref
    torch.cuda.synchronize()
    same_totals(env, ref_env, f"{layout} split={split}")
    env.close()
    ref_env.close()


def test_chunk_major_regions_beyond_4_gib_equal_short_launches(G):
    """70 000 envs in chunks of 32 768, 700 steps: three regions of 1.47 GB each in one 4.4 GB obs array (slice_args: the third chunk's base
    is 2.9 GB in, its rows cross 4 GiB at step 648)"""
    import torch

    n, chunk, T = 70000, 32768, 700
    env = handle(G, C_KIND, n)
    tr = env.rollout_chunked(T, mode="random", chunk=chunk, want=WANT)
    assert tr["obs"].shape == (3, T, NS[C_KIND], chunk) and tr["obs"].numel() * 4 > 4 * GIB
    ref_env = handle(G, C_KIND, n)
    for t0, t1 in pieces(T, 100):
        ref = ref_env.rollout(t1 - t0, mode="random", layout="soa", want=WANT, device_out=True)
        for key in WANT:
            same_bits(env.unchunk(tr[key][:, t0:t1]), ref[key], f"chunk-major steps [{t0}, {t1}): {key}")
        del ref
    torch.cuda.synchronize()
    same_totals(env, ref_env, "chunk-major")
    env.close()
    ref_env.close()


@pytest.mark.parametrize("actor", ACTORS)
def test_policy_rollouts_beyond_4_gib_by_replay(G, actor):
    """The three in-kernel actors at 65 536 envs x 1040 steps (obs 4.36 GB): the stored obs / rew / done are those of the stored (clipped)
    actions replayed in buffer mode on a second handle, 130 steps at a time; logp / val / act of the first 130 steps are those of a
    130-step launch from the same start."""
    import torch
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    env = handle(G, C_KIND, C_N)
    lo, hi = float(env.params.act_lo), float(env.params.act_hi)      # what clip_actions=True clips to
    col = FusedPolicyCollector(env, policy_of(env, actor, False), C_T, f16_mfma=(actor == "f16"), clip_actions=True)
    col.collect()
    assert col.obs.numel() * 4 > 4 * GIB
    twin = handle(G, C_KIND, C_N)
    same_bits(col.obs[0], twin.get_state(layout="soa", device_out=True), "the start")
    for t0, t1 in pieces(C_T, C_PIECE):
        u = torch.clamp(col.act[t0:t1], lo, hi).contiguous()
        tr = twin.rollout(t1 - t0, mode="buffer", actions=u, layout="soa", want=("obs", "rew", "done"), device_out=True)
        same_bits(tr["obs"], col.obs[1 + t0:1 + t1], f"{actor} steps [{t0}, {t1}): obs")
        same_bits(tr["rew"], col.rew[t0:t1], f"{actor} steps [{t0}, {t1}): rew")
        same_bits(tr["done"], col.done[t0:t1], f"{actor} steps [{t0}, {t1}): done")
        del tr, u
    torch.cuda.synchronize()
    assert bool(col.done.any())
    same(env.get_state(), twin.get_state(), "final state")
    same(env.get_reset_counts(), twin.get_reset_counts(), "reset counts")
    twin.close()
    short_env = handle(G, C_KIND, C_N)
    short = FusedPolicyCollector(short_env, policy_of(short_env, actor, False), C_PIECE, f16_mfma=(actor == "f16"), clip_actions=True)
    short.collect()
    torch.cuda.synchronize()
    for key in ("logp", "val", "act", "rew", "done"):
        same_bits(getattr(col, key)[:C_PIECE], getattr(short, key)[:C_PIECE], f"{actor}: {key} of the first {C_PIECE} steps")
    same_bits(col.obs[:C_PIECE + 1], short.obs, f"{actor}: obs of the first {C_PIECE} steps")
    short_env.close()
    env.close()


# ---- D. the normaliser launches on a large array -------------------------------------------------------------------------------------------------
def test_obs_moments_and_normalize_on_a_pitched_array_beyond_4_gib(G):
    import torch
    from gym_reinmav_amd import _abi as A

    kind, T = "quad3d_sl", 20
    P, ns = P_OBS[kind], NS[kind]
    env, obs = pitched_run(G, kind, "random", T, P, keep=True)
    x = obs[..., :N].contiguous().cpu().numpy()                     # [T, nS, N]: 166 KB
    # the padding holds NaN sentinels: one element of it read and the moments are NaN
    _check_moments(_moments(G, env, obs, A.SOA, T, P), np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(-1, ns), ns)
    clip = 1.0
    norm = _stats_from_a_rollout(G, env, clip=clip)
    torch.cuda.synchronize()
    mean_f, rstd_f = norm.mean_f.cpu().numpy()[:ns], norm.rstd_f.cpu().numpy()[:ns]
    assert mean_f.dtype == np.float32 and rstd_f.dtype == np.float32
    # the documented order in fp32: subtract, multiply, clamp
    want = np.clip((x - mean_f[None, :, None]) * rstd_f[None, :, None], np.float32(-clip), np.float32(clip))
    assert want.dtype == np.float32 and 0.0 < float((np.abs(want) == clip).mean()) < 1.0, "the clip binds somewhere, not everywhere"
    A.check(A.lib().rmav_obs_normalize(env._h, C.c_void_p(norm.data_ptr()), ptr(obs), ptr(obs), A.SOA, T, P))
    torch.cuda.synchronize()
    same(obs[..., :N].contiguous(), want, "normalised in place")
    assert not sentinel_problems({"obs": obs}), "the padding stays at the sentinel"
    env.close()


# ---- E. the pitch bound --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_pitch_beyond_the_bound_is_refused(G, kind):
    """c * 4 * pitch is added in 32 bits (c < nS <= 16): a pitch beyond 2^25 - where, for nS = 16 from 2^26 / 15 on, component c of every env
    would land in another column of the same step - is RMAV_ERR_INVALID before anything is launched."""
    import torch
    from gym_reinmav_amd import _abi as A

    env = handle(G, kind)
    state = env.get_state()
    for pitch in (MAX_PITCH + 64, (1 << 30) - 1):
        # first without any output: a library that did not refuse would have nothing to store
        assert env._lib.rmav_rollout_pitched(env._h, 2, A.ACT_RANDOM, None, None, None, None, None, pitch, 1) == A.ERR_INVALID, pitch
        assert b"2^25" in env._lib.rmav_last_error()
        tiny = filled((2, NS[kind], 192))
        for fused in (1, 0):
            assert env._lib.rmav_rollout_pitched(env._h, 2, A.ACT_RANDOM, None, None, ptr(tiny), None, None, pitch, fused) == A.ERR_INVALID
            assert b"2^25" in env._lib.rmav_last_error()
        torch.cuda.synchronize()
        assert bool((bits(tiny) == SENT).all())
    assert env.step_count == 0
    same(env.get_state(), state, "a refused call leaves the handle alone")
    env.close()


def test_a_chunk_wider_than_the_batch_beyond_the_bound_is_refused(G):
    """rmav_rollout_chunked turns chunk_envs > N into a column pitch: the same bound"""
    import torch
    from gym_reinmav_amd import _abi as A

    env = handle(G, "quad3d_sl")
    assert env._lib.rmav_rollout_chunked(env._h, 2, A.ACT_RANDOM, None, None, None, None, None, MAX_PITCH + 64) == A.ERR_INVALID
    assert b"2^25" in env._lib.rmav_last_error()
    tiny = filled((2, 16, 192))
    assert env._lib.rmav_rollout_chunked(env._h, 2, A.ACT_RANDOM, None, None, ptr(tiny), None, None, MAX_PITCH + 64) == A.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((bits(tiny) == SENT).all()) and env.step_count == 0
    env.close()


@pytest.mark.parametrize("T", (3, 1))
def test_the_last_accepted_pitch_works(G, T):
    """pitch = 2^25, nS = 16: in-step offsets up to 15 * 2^27, one step = 2^31 bytes - T = 3 on the two-wavefront kernel (generic drain, row 2
    starts at 4 GiB), T = 1 on the single-step kernel"""
    pitched_run(G, "quad3d_sl", "random", T, MAX_PITCH)
