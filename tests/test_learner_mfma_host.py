"""The shared-trunk learner on the fp32 matrix cores (rmav_ppo_grad_shared_mfma), what can be checked without a GPU: the chain of
sequential roundings counted from the kernel's geometry and the margin derived from it have the documented values; each arithmetic
mutant of learner_shared_ref's restatement lands at least a decade outside the bound the GPU test uses, on the GPU test's own inputs,
at every batch size it runs; those inputs keep the three clearance distances; and PPO(matrix_learner=True) refuses what it does not
compute."""
import math

import pytest

import learner_mfma_ref as M
from learner_mfma_ref import R

SEED = R.SEED
KIND_OF = dict(zip(M.BATCHES, ("quad3d", "quad2d", "quad2d_sl", "quad3d", "quad3d_sl", "reinmav", "quad3d", "quad3d_sl")))
# At B = 1 four mutants ARE the kernel's arithmetic: 1 / B = 1; a single sample's advantage is passed raw (learner_ref.adv_moments);
# and make_case puts sample 0 inside both clips (so that a batch of one has a gradient in every tensor), where neither clip acts
IDENTITIES = {(1, "no_inv_b"), (1, "raw_adv"), (1, "clip_wrong_side"), (1, "no_value_clip")}


def test_the_chain_is_counted_from_the_geometry():
    assert (M.TILE, M.STEP, M.GROUPS) == (32, 128, 256)
    assert [M.steps(B) for B in M.BATCHES] == [1, 1, 1, 1, 1, 1, 2, 17]
    assert [M.groups(B) for B in (1, 128, 129, 32768, 32769, 1 << 20)] == [1, 1, 2, 256, 256, 256]
    # 64 over K + 32 per tile and tile after tile + the 4 wavefronts + the workgroups' partials
    assert [M.chain_mfma(B) for B in M.BATCHES] == [101, 101, 101, 101, 101, 101, 102, 117]
    assert [B for _, B, *_ in M.WALKS] == [32769, 65665, 98304]
    assert [M.chain_mfma(B) for _, B, *_ in M.WALKS] == [64 + 64 + 4 + 256, 64 + 96 + 4 + 256, 64 + 96 + 4 + 256]
    assert M.chain_mfma(1040) == 64 + 32 + 4 + 9 and M.chain_mfma(524288) == 64 + 32 * 16 + 4 + 256


def test_the_margin_is_the_chain_rule_evaluated():
    import learner_ref

    assert M.MARGIN is learner_ref.MARGIN and M.FLOOR is learner_ref.FLOOR
    assert [M.margin_mfma(B) for B in M.BATCHES] == [M.MARGIN] * len(M.BATCHES)
    assert M.margin_mfma(1040) == M.MARGIN
    assert [round(M.margin_mfma(B), 1) for _, B, *_ in M.WALKS] == [18.5, 19.1, 18.6]
    for _, B, *_ in M.WALKS:   # never wider than max(MARGIN, chain / (6 + log2 B))
        assert M.margin_mfma(B) == max(M.MARGIN, M.chain_mfma(B) / (6.0 + math.log2(B)))
    for B in M.BATCHES:
        assert M.margin_mfma(B) <= max(M.MARGIN, M.chain_mfma(B) / (6.0 + math.log2(B)))


@pytest.mark.parametrize("B", M.BATCHES)
def test_mutants_land_a_decade_outside_the_gpu_bound(B):
    """The GPU test's bound is margin_mfma(B) * max(err of the torch fp32 learner, FLOOR) per tensor; here the fp32 learner runs on the
    CPU (the same expressions, the same precision) and stands for it.  One kind per batch size, every kind at least once."""
    kind, ent = KIND_OF[B], 0.01
    case = R.make_case(kind, B, SEED)
    g64, _, clear = R.oracle(kind, SEED, case, ent_coef=ent)
    assert min(clear.values()) >= R.CLEAR, clear
    g32, _ = R.torch_learner(R.trained_policy(kind, SEED), case, ent_coef=ent)
    e32 = R.tensor_errors(kind, g32, g64)
    bound = {n: M.margin_mfma(B) * max(e, M.FLOOR) for n, e in e32.items()}
    assert max(bound.values()) < 1e-4, bound   # the bound itself is of the order of fp32 rounding
    P = R.params64(R.trained_policy(kind, SEED))
    clean = R.tensor_errors(kind, R.restate(P, case, ent_coef=ent)[0], g64)
    assert all(clean[n] <= bound[n] for n in bound)
    for mutant in R.MUTANTS:
        em = R.tensor_errors(kind, R.restate(P, case, ent_coef=ent, mutant=mutant)[0], g64)
        worst = max(em[n] / bound[n] for n in bound)
        if (B, mutant) in IDENTITIES:
            assert worst <= 1.0, (mutant, worst)
        else:
            assert worst >= 10.0, (B, mutant, worst, em)


@pytest.mark.parametrize("kind", sorted(R.KINDS))
def test_the_gpu_inputs_keep_their_clearances(kind):
    """every (B, statistics) case the GPU test runs: ratios away from 1 +- clip, |v - val_old| away from clip, the two vf terms apart"""
    for B in M.BATCHES:
        for with_norm in (False, True):
            norm = R.make_norm(kind, SEED) if with_norm else None
            case = R.make_case(kind, B, SEED, norm)
            _, _, clear = R.oracle(kind, SEED, case, norm)
            assert min(clear.values()) >= R.CLEAR, (B, with_norm, clear)
            if B >= 127:   # both sides of both clips, both advantage signs
                P = R.params64(R.trained_policy(kind, SEED, norm))
                _, stats = R.restate(P, case, norm)
                assert stats[3] > 1.2 and case["adv"].min() < 0 < case["adv"].max()


@pytest.mark.parametrize("kind,B,with_norm,use_idx,ent", M.WALKS)
def test_the_walks_keep_their_clearances(kind, B, with_norm, use_idx, ent):
    norm = R.make_norm(kind, SEED) if with_norm else None
    case = R.make_case(kind, B, SEED, norm)
    _, _, clear = R.oracle(kind, SEED, case, norm, ent_coef=ent)
    assert min(clear.values()) >= R.CLEAR, clear
    assert case["adv"].min() < 0 < case["adv"].max()


def test_matrix_learner_refuses_what_it_does_not_compute():
    from gym_reinmav_amd.ppo import PPO, MlpPolicy

    with pytest.raises(ValueError, match="matrix_learner=True needs fused_learner=True"):
        PPO(MlpPolicy(10, 4, value_network="shared"), matrix_learner=True)
    with pytest.raises(ValueError, match="matrix_learner=True computes an MlpPolicy"):
        PPO(MlpPolicy(10, 4), fused_learner=True, matrix_learner=True)
    with pytest.raises(ValueError, match="hidden=32"):
        PPO(MlpPolicy(10, 4, hidden=32, value_network="shared"), fused_learner=True, matrix_learner=True)
    with pytest.raises(ValueError, match="CPU tensors"):   # the architecture passes; the fused learner's own device check refuses
        PPO(MlpPolicy(10, 4, value_network="shared"), fused_learner=True, matrix_learner=True, fused_optimizer=True)
    ppo = PPO(MlpPolicy(10, 4, value_network="shared"))   # the default: the torch path, no matrix learner
    assert ppo.matrix_learner is False and ppo.fused_learner is False and ppo._fused is None
