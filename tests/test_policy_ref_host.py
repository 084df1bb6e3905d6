"""oracle/policy_ref.py without a GPU: the restatement holds the operands the packer stores, says what the fp32 torch policy says at
the old tolerances, and its bound is tight enough to see six arithmetic mutants - on exactly the inputs tests/test_gpu_policy_exact.py
launches (the builders of those inputs live here and are imported there)."""
import functools

import numpy as np
import pytest

import policy_ref as R
from test_gpu_ppo import ACTOR_TOL
from util import random_cases

SHAPES = (("quad2d", 131), ("quad3d", 65), ("quad3d_sl", 300), ("reinmav", 64), ("quad3d", 1))
ACTORS = ("fp32", "fp32_mfma", "bf16", "bf16_1w", "f16", "f16_shared")
QUANTISED = ("bf16", "bf16_1w", "f16", "f16_shared")
HUGE_ENVS = (3, 40, -1)          # (the last env of the launch), where they exist
SAT = 40.0                       # magnitude of the one non-zero per row of a saturating layer


def cases_of(actor, kind):
    """The cases of section 3 of the issue an actor runs on a kind."""
    out = ["dense", "dense_wide", "layer3", "layer2"]
    if actor in QUANTISED:
        out.append("huge")
    if actor in ("f16", "f16_shared", "fp32_mfma") and kind != "reinmav":   # the *_nrm kernels: the four quadrotor kinds
        out.append("norm")
    return out


def dims(kind):
    from gym_reinmav_amd import _abi as A

    k = A.KIND_BY_NAME[kind]
    return A.STATE_DIM[k], A.ACTION_DIM[k]


# seeds moved until test_input_conditions held (the issue: change the seeds, not the fractions): one env, or 64 alike, make a narrow
# sample of max|y|, and the f16 bound is ~1/4 of the accepted error where max|y| is ordinary
SEED_SHIFT = {("reinmav", 64, "dense"): 1, ("quad3d", 1, "dense"): 290, ("quad3d", 1, "dense_wide"): 10}


def _seed(kind, n, case):
    return 100000 * SEED_SHIFT.get((kind, n, case), 0) + 1000 * ("quad2d", "quad3d", "quad3d_sl", "reinmav").index(kind) + 10 * ("dense", "dense_wide", "layer3", "layer2", "huge", "norm").index(case) + (n % 7)


def _one_per_row(rng, rows, cols):
    """[rows, cols] with ONE non-zero of magnitude SAT and random sign per row, every column used."""
    W = np.zeros((rows, cols), np.float32)
    W[np.arange(rows), (np.arange(rows) + rng.randint(cols)) % cols] = SAT * rng.choice([-1.0, 1.0], rows)
    return W


def make_policy(actor, kind, n, case, logstd=0.0):
    """The CPU MlpPolicy of a case (the GPU test moves it to the device): default init + 0.3 randn, action head x 20, biases in +-0.3;
    dense_wide: hidden weights x 4; layer3 / layer2: the layers in front replaced by saturating one-non-zero-per-row matrices."""
    import torch
    from gym_reinmav_amd.ppo import MlpPolicy

    nS, nA = dims(kind)
    seed = _seed(kind, n, case)
    torch.manual_seed(seed)
    rng = np.random.RandomState(seed)
    shared = actor == "f16_shared"
    pol = MlpPolicy(nS, nA, init_logstd=float(logstd), value_network="shared" if shared else "copy")
    with torch.no_grad():
        for net in (pol.pi, pol.vf):
            for lin in net:
                lin.weight.add_(torch.randn_like(lin.weight) * 0.3)
                lin.bias.uniform_(-0.3, 0.3)
        pol.pi[2].weight.mul_(20.0)
        trunks = (pol.pi,) if shared else (pol.pi, pol.vf)
        for net in trunks:
            if case == "dense_wide":
                net[0].weight.mul_(4.0)
                net[1].weight.mul_(4.0)
            if case in ("layer3", "layer2"):
                net[0].weight.copy_(torch.from_numpy(_one_per_row(rng, 64, nS)))
            if case == "layer3":
                net[1].weight.copy_(torch.from_numpy(_one_per_row(rng, 64, 64)))
        if case in ("layer3", "layer2"):   # dense weights bounded away from 0: none becomes an f16-subnormal operand (|-2 w| >= 2^-14)
            for lin in list(pol.pi) + list(pol.vf):
                w = lin.weight
                w.copy_(torch.where((w != 0) & (w.abs() < 1e-3), torch.where(w < 0, -1e-3, 1e-3).to(w.dtype), w))
    return pol


def make_states(kind, n, case):
    """[n, nS] fp32 start states of a case (`env.set_state`)."""
    nS, _ = dims(kind)
    seed = _seed(kind, n, case)
    if case in ("layer3", "layer2"):
        # +-1, the sign of component c = bit c of a 16-bit hash of the env index (the plain index would give env e and env e + 32
        # the same 5-component state: the lane-exchange mutant needs them different)
        e = np.arange(n, dtype=np.uint64)
        word = ((e * np.uint64(0x9E3779B1)) >> np.uint64(13)) & np.uint64(0xFFFF)
        bits = (word[:, None] >> np.arange(nS, dtype=np.uint64)[None, :]) & np.uint64(1)
        return (1.0 - 2.0 * bits.astype(np.float64)).astype(np.float32)
    wide = case in ("dense_wide", "norm")
    if kind == "reinmav":
        sc = np.where(np.arange(n) % 2 == 0, 1.0, 3.0 if wide else 1.0)[:, None]
        s = (np.random.RandomState(seed).uniform(-1, 1, (n, nS)) * sc).astype(np.float32)
    else:
        s = random_cases(kind, n, seed, wide=wide)[0]
    if case == "norm":             # up to +-6: behind statistics of mean ~0.4 and deviation ~1.7, clip = 2 binds on a part of the envs
        s = s * np.float32(2.0)
    if case == "huge":
        for e in sorted({i % n for i in HUGE_ENVS if -n <= i < n}):
            s[e, 0] = 3e4          # k x > 65504
            s[e, nS - 1] = 1e30
    return s


def huge_envs(n):
    return sorted({i % n for i in HUGE_ENVS if -n <= i < n})


def make_norm_tables(kind, n):
    """Host twin of the statistics the GPU test builds for the `norm` case is NOT possible (the tables come from a device update);
    the host tests use tables of the same character: means ~0.4, standard deviations ~1.7, clip 2."""
    nS, _ = dims(kind)
    rng = np.random.RandomState(_seed(kind, n, "norm"))
    mean = np.zeros(16, np.float32)
    rstd = np.ones(16, np.float32)
    mean[:nS] = 0.4 + 0.05 * rng.randn(nS)
    rstd[:nS] = 1.0 / (1.7 + 0.05 * rng.randn(nS))
    return mean, rstd, np.float32(2.0)


def nets_of(pol):
    """The fp32 parameters of an MlpPolicy as the arrays oracle/policy_ref.py takes."""
    g = lambda net: [a for lin in net for a in (lin.weight.detach().cpu().numpy(), lin.bias.detach().cpu().numpy())]  # noqa: E731
    return {"pi": g(pol.pi), "vf": g(pol.vf)}


def family(actor):
    return "bf16" if actor.startswith("bf16") else "fp32" if actor.startswith("fp32") else actor


@functools.lru_cache(maxsize=None)
def case_inputs(fam, kind, n, case):
    """(policy, nets, states [n, nS], norm tables or None) of a configuration, built once."""
    pol = make_policy(fam, kind, n, case)
    return pol, nets_of(pol), make_states(kind, n, case), (make_norm_tables(kind, n) if case == "norm" else None)


@functools.lru_cache(maxsize=None)
def reference(fam, kind, n, case):
    _, nets, s, norm = case_inputs(fam, kind, n, case)
    return R.ACTORS[fam](nets, s.T, norm=norm)


def outside(res_mut, res):
    """Per env: some output row of the mutated restatement is outside the reference's bound (a NaN is outside)."""
    return (~(np.abs(res_mut.y - res.y) <= res.bound)).any(1)


# ---- the restatement against the packer ---------------------------------------------------------------------------------------------
def _unpack(buf, fmt16):
    """pack()'s fragment area of one net -> (A1 [64, 16], A2 [64, 64], A3 [32, 64]) read back through _rowmap; buf: 16-bit words."""
    import torch
    from gym_reinmav_amd.ppo import _rowmap

    v = buf.view(fmt16).double().numpy().reshape(-1, 64, 8)       # [fragment][lane][j]
    A1, A2, A3 = np.full((64, 16), np.nan), np.full((64, 64), np.nan), np.full((32, 64), np.nan)
    for lane in range(64):
        m, h = lane & 31, lane >> 5
        for j in range(8):
            for Mt in range(2):
                A1[32 * Mt + m, 8 * h + j] = v[Mt, lane, j]
                for s in range(4):
                    A2[32 * Mt + m, _rowmap(s, h, j)] = v[2 + 4 * Mt + s, lane, j]
            for s in range(4):
                A3[m, _rowmap(s, h, j)] = v[10 + s, lane, j]
    assert not (np.isnan(A1).any() or np.isnan(A2).any() or np.isnan(A3).any())   # the map reaches every element once
    return A1, A2, A3


@pytest.mark.parametrize("actor", ["bf16", "f16", "f16_shared"])
@pytest.mark.parametrize("kind", ["quad2d", "quad3d_sl"])   # the smallest and the largest state (nS = 5, 16)
def test_reference_operands_equal_the_packed_buffer(actor, kind):
    """The quantised weights the restatement multiplies by and its unscaled biases are, bit for bit, what _PolicyPacker.pack() stores
    (bf16 / f16 rounding, the f16 actor's -2k / -2 scales, the zero padding, the stacked heads of the shared trunk)."""
    import torch
    from gym_reinmav_amd.ppo import _PolicyPacker

    pol, nets, _, _ = case_inputs(actor, kind, 65, "dense")
    nS, nA = dims(kind)
    buf = _PolicyPacker(pol, nS, actor).pack()
    fmt16 = torch.bfloat16 if actor == "bf16" else torch.float16
    ops = R.packed_operands(actor, nets)
    n_frag, n_bias = 14 * 256, 160
    for i, name in enumerate(["pi"] if actor == "f16_shared" else ["pi", "vf"]):
        base = i * (n_frag + n_bias)
        A1, A2, A3 = _unpack(buf[base:base + n_frag].contiguous().view(torch.int16), fmt16)
        bias = buf[base + n_frag:base + n_frag + n_bias].numpy()
        r1, r2, r3, b1, b2, b3 = ops[name]
        rows = list(range(nA)) + [4] if actor == "f16_shared" else list(range(r3.shape[0]))
        exp3, expb3 = np.zeros((32, 64)), np.zeros(32, np.float32)
        exp3[rows], expb3[rows] = r3, b3
        assert np.array_equal(A1, r1) and np.array_equal(A2, r2) and np.array_equal(A3, exp3), (actor, name)
        assert np.array_equal(bias[:64], b1) and np.array_equal(bias[64:128], b2) and np.array_equal(bias[128:], expb3), (actor, name)
    assert (r1[:, nS:] == 0).all() and np.abs(r1[:, :nS]).min() > 0


# ---- the restatement against the fp32 torch policy -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,kind,n,case", [(f, k, n, c) for f in ("fp32", "bf16", "f16", "f16_shared") for k, n in SHAPES
                                             for c in ("dense", "norm") if c in cases_of(f, k) or (c == "norm" and f == "fp32" and k != "reinmav")])
def test_reference_agrees_with_the_torch_policy(fam, kind, n, case):
    """The new reference says what the old tests say: quantised families inside ACTOR_TOL * max(1, max|y|) of the fp32 torch policy,
    the unquantised one inside 2e-5 * max(1, max|y|)."""
    import copy

    import torch

    pol, _, s, norm = case_inputs(fam, kind, n, case)
    x = torch.from_numpy(np.ascontiguousarray(R.normalise(s.T, norm)))
    with torch.no_grad():
        mean, val = copy.deepcopy(pol).double()(x.double())
    res = reference(fam, kind, n, case)
    tol = 2e-5 if fam == "fp32" else ACTOR_TOL[fam]
    em = np.abs(res.mean - mean.numpy().T).max()
    ev = np.abs(res.value - val.numpy()).max()
    sm, sv = max(1.0, float(mean.abs().max())), max(1.0, float(val.abs().max()))
    print(f"{fam} {kind} {n} {case}: mean err {em:.3g} (tol {tol * sm:.3g}), value err {ev:.3g} (tol {tol * sv:.3g})")
    assert em < tol * sm and ev < tol * sv


# ---- conditions on the inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["bf16", "f16", "f16_shared"])
@pytest.mark.parametrize("kind,n", SHAPES)
def test_input_conditions(fam, kind, n):
    """Staged cases.  layer3: every env has zero undecided activations and zero f16-subnormal operands - the bound is accumulation +
    fold only.  layer2: the same for the operands of the layer under test (the first hidden layer's activations, the subnormal
    operands of layers 1 and 2); the SECOND hidden layer's activations are ordinary values there - they have to be, a saturated one
    would hide layer 2's sum - so they may be undecided, and the bound accounts for them.
    Dense cases: the bound's median over envs is at most 1/10 (bf16) / 1/3 (f16) of what ACTOR_TOL accepts, for the mean rows and for
    the value - so the GPU comparison cannot pass by being loose."""
    res = reference(fam, kind, n, "layer3")
    assert res.undecided.max() == 0 and res.subnormal.max() == 0, (int(res.undecided.max()), int(res.subnormal.max()))
    assert res.bound.max() < 1e-4 * np.abs(res.y).max()
    res = reference(fam, kind, n, "layer2")
    assert res.undecided_l1.max() == 0 and res.subnormal_l12.max() == 0, (int(res.undecided_l1.max()), int(res.subnormal_l12.max()))
    for case in ("layer3", "layer2"):
        res = reference(fam, kind, n, case)
        print(f"{fam} {kind} {n} {case}: bound median {np.median(res.bound):.3g} max {res.bound.max():.3g}, max|y| {np.abs(res.y).max():.3g}, "
              f"envs with undecided activations {float((res.undecided.max(1) > 0).mean()):.2f}")
        assert np.isfinite(res.bound).all()
    frac = 10.0 if fam == "bf16" else 3.0
    for case in ("dense", "dense_wide"):
        res = reference(fam, kind, n, case)
        for what, y, b in (("mean", res.mean, res.bound[:, :-1]), ("value", res.value[:, None], res.bound[:, -1:])):
            accepted = ACTOR_TOL[fam] * max(1.0, float(np.abs(y).max()))
            med = float(np.median(b.max(1)))
            print(f"{fam} {kind} {n} {case} {what}: median bound {med:.3g} = 1/{accepted / med:.0f} of the accepted {accepted:.3g}; "
                  f"envs with undecided activations {float((res.undecided.max(1) > 0).mean()):.2f}")
            assert med <= accepted / frac, (case, what, med, accepted)


# ---- mutants ----------------------------------------------------------------------------------------------------------------------------
# (mutant, families it is a mutation of, cases it is applied in).  Where a mutant cannot be seen, and why:
#   act_trunc      bf16 only (f16 hands r on, rounded by the same instruction).  Not in layer3: the operands of the output layer are
#                  exactly +-1 there, which truncation leaves, and layer 2 stays saturated with +-2.875 in place of +-2.890625.
#   input_rne      f16 only; dense_wide only.  In the staged cases layer 1 saturates whatever the input's last bit is, and on the
#                  default-scale dense case it stays inside the worst-case bound on ~99 % of the envs (the issue's prototype).
#   fold_unrounded f16 only; the staged cases and dense_wide - not the default-scale dense case, for the same reason.  It shifts an
#                  output row of every env by the same ~1e-4, about the size of the bound where layer 3's operands are not exact:
#                  with n = 1 there is one env to exceed it on, so there it is applied in layer3 only.
#   sat_inf        f16 only, the huge case (the only one with |k x| > 65504).
#   zero_slot      layer3: a slot of the SECOND hidden fragment; every other case: one of the first.  Not f16 with n = 1 in the huge
#                  and the staged cases: the one env's unit is saturated, and the f16 operand of a unit saturated at tanh = +1 IS 0.
#   swap_lanes     needs envs 48..63 of a wavefront: not n = 1.  In layer3 the exchanged fragment is the second one.
def _mutants(fam, kind, n, case):
    f16 = fam.startswith("f16")
    out = []
    if fam == "bf16" and case != "layer3":
        out.append("act_trunc")
    if f16 and case == "dense_wide":
        out.append("input_rne")
    if f16 and (case == "layer3" or (case in ("layer2", "dense_wide") and n > 1)):
        out.append("fold_unrounded")
    if f16 and case == "huge":
        out.append("sat_inf")
    layer = 2 if case == "layer3" else 1
    if not (f16 and n == 1 and case in ("huge", "layer3", "layer2")):
        out.append(("zero_slot", (layer, R.rowmap(3, 1, 5))))
    if n >= 64:
        out.append(("swap_lanes", layer))
    return out


@pytest.mark.parametrize("fam", ["bf16", "f16", "f16_shared"])
@pytest.mark.parametrize("kind,n", SHAPES)
@pytest.mark.parametrize("case", ["dense", "dense_wide", "layer3", "layer2", "huge"])
def test_every_mutant_leaves_the_bound(fam, kind, n, case):
    _, nets, s, norm = case_inputs(fam, kind, n, case)
    res = reference(fam, kind, n, case)
    for mut in _mutants(fam, kind, n, case):
        bad = outside(R.ACTORS[fam](nets, s.T, norm=norm, mutant=mut), res)
        print(f"{fam} {kind} {n} {case} {mut}: outside the bound on {int(bad.sum())} of {n} envs")
        assert bad.any(), mut
        if R._name(mut) == "sat_inf":   # ... and exactly there: the saturated envs
            assert set(np.nonzero(bad)[0]) == set(huge_envs(n))


def test_huge_states_saturate_in_the_reference():
    """The huge case as the restatement sees it: f16 operands 65504, outputs finite, the other envs untouched by their neighbours."""
    for fam in ("bf16", "f16", "f16_shared"):
        res = reference(fam, "quad3d", 65, "huge")
        assert np.isfinite(res.y).all()
        s = make_states("quad3d", 65, "huge")
        assert (s[huge_envs(65), 0] == np.float32(3e4)).all() and huge_envs(65) == [3, 40, 64]
    assert R.quantise(np.float64(np.float32(3e4) * R.K32), R.F16, "rtz", saturate=True) == 65504.0
