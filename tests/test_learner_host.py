"""The fused learner (rmav_ppo_grad), what can be checked without a GPU: the hand-written fp64 restatement of its arithmetic
(learner_ref.restate) agrees with central differences and with the autograd oracle; each arithmetic mutant of the restatement lands at
least a decade outside the bound the GPU test uses, on the GPU test's own inputs - so that bound has teeth; the inputs the GPU test
draws keep the three clearance distances; and PPO(fused_learner=True) refuses what it does not compute."""
import numpy as np
import pytest
import torch

import learner_ref as R

SEED = 0


def _loss64(P, case, norm, ent_coef):
    return R.restate(P, case, norm, ent_coef=ent_coef)[1][0]


@pytest.mark.parametrize("kind", sorted(R.KINDS))
@pytest.mark.parametrize("with_norm", [False, True])
def test_restatement_agrees_with_central_differences_and_autograd(kind, with_norm):
    norm = R.make_norm(kind, SEED) if with_norm else None
    case = R.make_case(kind, 65, SEED, norm)
    P = R.params64(R.trained_policy(kind, SEED, norm))
    g, stats = R.restate(P, case, norm, ent_coef=0.01)
    g64, s64, clear = R.oracle(kind, SEED, case, norm, ent_coef=0.01)
    assert min(clear.values()) >= R.CLEAR, clear
    np.testing.assert_allclose(stats, s64, rtol=1e-12, atol=1e-13)
    assert max(R.tensor_errors(kind, g, g64).values()) < 1e-11
    # central differences on a handful of entries of every tensor (fp64, h = 1e-6: truncation ~1e-12, rounding ~1e-10 of the loss)
    rng = np.random.default_rng(5)
    o = 0
    for k, p in enumerate(P):
        for e in rng.choice(p.size, size=min(4, p.size), replace=False):
            h = 1e-6
            flat = p.reshape(-1)
            keep = flat[e]
            flat[e] = keep + h
            up = _loss64(P, case, norm, 0.01)
            flat[e] = keep - h
            dn = _loss64(P, case, norm, 0.01)
            flat[e] = keep
            fd = (up - dn) / (2 * h)
            assert abs(fd - g[o + e]) <= 1e-8 + 1e-6 * abs(g[o + e]), (R.NAMES[k], int(e), fd, g[o + e])
        o += p.size
    assert o == g.size


@pytest.mark.parametrize("kind,B", [("quad2d", 33), ("quad3d", 130), ("quad3d_sl", 2125), ("reinmav", 65)])
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_land_a_decade_outside_the_gpu_bound(kind, B, mutant):
    """The GPU test's bound is MARGIN * max(err of the torch fp32 learner, FLOOR) per tensor; here the fp32 learner runs on the CPU
    (the same expressions, the same precision) and stands for it."""
    ent = 0.01
    case = R.make_case(kind, B, SEED)
    g64, _, clear = R.oracle(kind, SEED, case, ent_coef=ent)
    assert min(clear.values()) >= R.CLEAR, clear
    g32, _ = R.torch_learner(R.trained_policy(kind, SEED), case, ent_coef=ent)
    e32 = R.tensor_errors(kind, g32, g64)
    bound = {n: R.MARGIN * max(e, R.FLOOR) for n, e in e32.items()}
    assert max(bound.values()) < 1e-4, bound   # the bound itself is of the order of fp32 rounding
    P = R.params64(R.trained_policy(kind, SEED))
    clean = R.tensor_errors(kind, R.restate(P, case, ent_coef=ent)[0], g64)
    assert all(clean[n] <= bound[n] for n in bound)
    em = R.tensor_errors(kind, R.restate(P, case, ent_coef=ent, mutant=mutant)[0], g64)
    worst = max(em[n] / bound[n] for n in bound)
    assert worst >= 10.0, (mutant, worst, em)


def test_the_margin_of_the_walks_is_the_chain_rule_evaluated():
    """one rule for both learners (learner_shared_ref re-exports it): MARGIN up to the 162 roundings of B = 2125, the quotient beyond"""
    import learner_ref
    import learner_shared_ref

    assert learner_shared_ref.margin is learner_ref.margin and learner_shared_ref.chain is learner_ref.chain
    assert [R.margin(B) for B in R.BATCHES] == [R.MARGIN] * len(R.BATCHES)
    assert [R.chain(B) for _, B, *_ in R.WALKS] == [64 + 128 + 512, 64 + 192 + 512, 64 + 256 + 512]
    assert [round(R.margin(B), 1) for _, B, *_ in R.WALKS] == [33.5, 34.9, 36.2]


@pytest.mark.parametrize("kind,B,with_norm,use_idx,ent", R.WALKS)
def test_the_walks_keep_their_clearances(kind, B, with_norm, use_idx, ent):
    """the batches at which a workgroup walks several tiles: the same three distances, and the tile counts the GPU test names"""
    tiles = -(-B // 64)
    assert (tiles, B % 64) in ((514, 1), (1026, 1), (2048, 0)) and -(-tiles // 512) in (2, 3, 4)
    norm = R.make_norm(kind, SEED) if with_norm else None
    case = R.make_case(kind, B, SEED, norm)
    _, _, clear = R.oracle(kind, SEED, case, norm, ent_coef=ent)
    assert min(clear.values()) >= R.CLEAR, clear
    assert case["adv"].min() < 0 < case["adv"].max()


@pytest.mark.parametrize("B", R.HYPER_BATCHES)
@pytest.mark.parametrize("kind", R.HYPER_KINDS)
@pytest.mark.parametrize("clip,vf_coef,ent", R.HYPERS)
def test_a_kept_default_lands_outside_the_gpu_bound(kind, B, clip, vf_coef, ent):
    """The GPU test's other hyper-parameters: the batch drawn for the case's clip keeps its clearances, the clean restatement is
    inside margin(B) * max(err of the fp32 learner, FLOOR), and a restatement that keeps clip = 0.2 or vf_coef = 0.5 - a literal
    somewhere between the binding and the kernel - lands more than a decade outside it."""
    assert clip != R.CLIP and vf_coef != R.VF_COEF
    case = R.make_case(kind, B, SEED, clip=clip)
    g64, s64, clear = R.oracle(kind, SEED, case, clip=clip, vf_coef=vf_coef, ent_coef=ent)
    assert min(clear.values()) >= R.CLEAR, clear
    g32, _ = R.torch_learner(R.trained_policy(kind, SEED), case, clip=clip, vf_coef=vf_coef, ent_coef=ent)
    bound = {n: R.margin(B) * max(e, R.FLOOR) for n, e in R.tensor_errors(kind, g32, g64).items()}
    P = R.params64(R.trained_policy(kind, SEED))
    g, stats = R.restate(P, case, clip=clip, vf_coef=vf_coef, ent_coef=ent)
    clean = R.tensor_errors(kind, g, g64)
    assert all(clean[n] <= bound[n] for n in bound)
    np.testing.assert_allclose(stats, s64, rtol=1e-12, atol=1e-13)
    for kept in (dict(clip=R.CLIP, vf_coef=vf_coef), dict(clip=clip, vf_coef=R.VF_COEF)):
        em = R.tensor_errors(kind, R.restate(P, case, ent_coef=ent, **kept)[0], g64)
        worst = max(em[n] / bound[n] for n in bound)
        assert worst >= 10.0, (kept, worst, em)


@pytest.mark.parametrize("kind", sorted(R.KINDS))
def test_the_gpu_inputs_keep_their_clearances(kind):
    """every (B, statistics) case the GPU test runs: ratios away from 1 +- clip, |v - val_old| away from clip, the two vf terms apart"""
    for B in R.BATCHES:
        for with_norm in (False, True):
            norm = R.make_norm(kind, SEED) if with_norm else None
            case = R.make_case(kind, B, SEED, norm)
            _, _, clear = R.oracle(kind, SEED, case, norm)
            assert min(clear.values()) >= R.CLEAR, (B, with_norm, clear)
            if B >= 64:   # both sides of both clips, both advantage signs
                P = R.params64(R.trained_policy(kind, SEED, norm))
                _, stats = R.restate(P, case, norm)
                assert stats[3] > 1.2 and case["adv"].min() < 0 < case["adv"].max()


def test_exact_cases_in_the_restatement():
    """the batches the GPU test uses for its bitwise zeros: the clipped branches kill the policy / the value gradient exactly"""
    kind = "quad3d"
    sl = R.slices(kind)
    P = R.params64(R.trained_policy(kind, SEED))
    g, _ = R.restate(P, R.make_case(kind, 130, SEED, mode="pg_clipped"), ent_coef=0.01)
    assert not g[:sl["vf.0.weight"].start].any() and np.abs(g[sl["vf.0.weight"]]).max() > 0
    np.testing.assert_array_equal(g[sl["logstd"]], -0.01)
    g, _ = R.restate(P, R.make_case(kind, 130, SEED, mode="vf_clipped"))
    assert not g[sl["vf.0.weight"].start:sl["logstd"].start].any() and np.abs(g[sl["pi.0.weight"]]).max() > 0


def test_fused_learner_refusals_that_need_no_gpu():
    from gym_reinmav_amd.ppo import PPO, MlpPolicy

    with pytest.raises(ValueError, match='value_network="shared"'):
        PPO(MlpPolicy(10, 4, value_network="shared"), fused_learner=True)
    with pytest.raises(ValueError, match="hidden=32"):
        PPO(MlpPolicy(10, 4, hidden=32), fused_learner=True)
    with pytest.raises(ValueError, match="CPU tensors"):
        PPO(MlpPolicy(10, 4), fused_learner=True)
    ppo = PPO(MlpPolicy(10, 4))   # the default is the torch path
    assert ppo.fused_learner is False

    class Ro:   # a collector without an env handle
        pass

    T, N = 2, 8
    ro = Ro()
    ro.rew, ro.done = torch.zeros(T, N), torch.zeros(T, N, dtype=torch.uint8)
    ro.val, ro.logp = torch.zeros(T + 1, N), torch.zeros(T, N)
    ro.obs, ro.act = torch.zeros(T + 1, 10, N), torch.zeros(T, 4, N)
    ppo.fused_learner = True   # (past the constructor's checks: the collector's is made in update)
    with pytest.raises(ValueError, match="env handle"):
        ppo.update(ro)
