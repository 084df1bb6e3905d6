"""The policy action rule, what can be checked without a GPU: the two entry points are declared, exported and bound; the kernels that
take the rule - every *_nrm / *_dr policy kernel - keep the budgets of test_obs_norm_build.py / test_domain_rand_build.py (`make asm`);
and the rule added no kernel: every family keeps its size."""
import buildinfo as B

NEW = {"rmav_set_policy_action_rule": ("int", 4), "rmav_get_policy_action_rule": ("int", 4)}
ONE = ("_ZN4rmav13k_rollout_nrmILi", "_ZN4rmav16k_rollout_nrm_drILi")
PAIRS = ("_ZN4rmav18k_rollout_pair_nrmILi", "_ZN4rmav25k_rollout_pair_shared_nrmILi",
         "_ZN4rmav17k_rollout_pair_drILi", "_ZN4rmav24k_rollout_pair_shared_drILi")


def test_action_rule_entry_points_are_declared_exported_and_bound(built):
    B.assert_entry_points(NEW)


def test_kernels_that_take_the_rule_keep_their_budgets():
    """No scratch, no spills, at most 256 VGPR + AGPR; the pair actors at two wavefronts per SIMD or more; no LDS permutes and no
    compiler-packed fp32 in any of them; and every one of them does take the rule (ActRuleArgs is in its signature)."""
    one, pairs = B.family(*ONE), B.family(*PAIRS)
    assert len(one) == 16 and len(pairs) == 32, (len(one), len(pairs))
    for n, u in {**one, **pairs}.items():
        assert B.clean(u) and u["vgpr"] + u["agpr"] <= 256, (n, u)
        assert "ActRuleArgs" in n, n
    for n, u in pairs.items():
        assert u["occ"] >= 2, (n, u)
    B.assert_matrix_core_clean(r"_ZN4rmav(13k_rollout_nrm|16k_rollout_nrm_dr|18k_rollout_pair_nrm|25k_rollout_pair_shared_nrm|"
                               r"17k_rollout_pair_dr|24k_rollout_pair_shared_dr)ILi", 48)


def test_the_rule_added_no_kernel():
    """Every family of the census has the members it had, and no other kernel signature mentions the rule."""
    seen = B.family(*B.FAMILIES)
    taking = {n for n in B.usage() if "ActRuleArgs" in n}
    assert taking == set(B.family(*ONE, *PAIRS)), sorted(taking ^ set(B.family(*ONE, *PAIRS)))
    assert taking <= set(seen)
