// rmav_ladder.hpp - the feature ladder, host side ("The feature ladder").  The features a handle switches on are rungs of ONE
// ladder: the kernels of a rung take the arguments of every rung below it as well, so a handle runs the kernels of the highest rung it has
// switched on.  This header is the one place that knows the order: the rungs, rung_of, and one table row per rung with the words its
// messages use and the launchers of its unit.  rmav_abi.hip and rmav_ppo_abi.hip route through the table; the rung units take the enum (and
// their noun) from here, through rmav_rung_launch.hpp / rmav_policy_rung.hpp.
#pragma once

#include "rmav_handle.hpp"

// in ladder order (the kernel headers' guard fragments count the same way: RMAV_RUNG in rmav_rollout_rung.inc / rmav_pair_rung.inc)
enum Rung : int { RUNG_NONE = 0, RUNG_RANGE, RUNG_SKIP, RUNG_REWARD, RUNG_DISTURB, RUNG_SENSOR, RUNG_ACTUATOR, RUNG_START, RUNG_TERM, RUNG_COUNT };

// THE precedence of the handle's switches: the highest rung that is on (eight flag tests, nothing else)
RMAV_INTERNAL inline Rung rung_of(const rmav_env_s *h) {
    if (h->term_on) return RUNG_TERM;
    if (h->start_on) return RUNG_START;
    if (h->actuator_on) return RUNG_ACTUATOR;
    if (h->sensor_on) return RUNG_SENSOR;
    if (h->disturb_on) return RUNG_DISTURB;
    if (h->reward_on) return RUNG_REWARD;
    if (h->frame_skip > 1) return RUNG_SKIP;
    if (h->range_mask) return RUNG_RANGE;
    return RUNG_NONE;
}

struct RungRow {
    const char *noun;     // "no <noun> kernel for action mode %d"; what need_variants says the fp32 vector-ALU and bf16 actors lack
    const char *handle;   // "<handle> runs the normalised kernels"
    const char *who;      // the phrase need_variants is given
    // one launch of the rung's fused rollout / single step on the handle's stream (rmav_handle.hpp has the arguments).  st: the rungs above the
    // tracking reward have one store policy and ignore it.  ctrl: the ranged step has a form that ends with control() ...
    int (*rollout)(rmav_handle h, int mode, int st, const rmav::RolloutArgs &a);
    int (*step)(rmav_handle h, const rmav::RolloutArgs &a, bool ctrl, int bs, const rmav::FinalArgs &fa);
    bool control_behind;   // ... the steps from the tracking reward up are followed by k_control; rollout_impl refuses control() with a frame skip
    // the policy-in-kernel rollout: the rungs up to the disturbance are variants of rmav_policy_abi.hip's kernels
    int (*policy)(rmav_handle h, int kmode, const rmav::RolloutArgs &a, const rmav::BootArgs *bt, const rmav::NormArgs *nm);
};

constexpr RungRow kLadder[RUNG_COUNT] = {
    {nullptr, nullptr, nullptr, nullptr, nullptr, false, rmav_launch_policy_rollout},
    {"ranged", "a handle with a parameter range", "a handle with a parameter range", rmav_launch_ranged_rollout, rmav_launch_ranged_step, false,
     rmav_launch_policy_rollout},
    {"frame-skip", "a handle with a frame skip", "a handle with a frame skip (rmav_set_frame_skip)", rmav_launch_skip_rollout, rmav_launch_skip_step, false,
     rmav_launch_policy_rollout},
    {"tracking-reward", "a handle with a tracking reward", "a handle with a tracking reward (rmav_set_reward)", rmav_launch_reward_rollout, rmav_launch_reward_step,
     true, rmav_launch_policy_rollout},
    {"disturbed", "a handle with a disturbance", "a handle with a disturbance (rmav_set_disturbance)", rmav_launch_disturb_rollout, rmav_launch_disturb_step, true,
     rmav_launch_policy_rollout},
    {"sensor-noise", "a handle with sensor noise", "a handle with sensor noise (rmav_set_sensor_noise)", rmav_launch_sensor_rollout, rmav_launch_sensor_step, true,
     rmav_launch_sensor_policy_rollout},
    {"actuator-lag", "a handle with actuator lag", "a handle with actuator lag (rmav_set_actuator)", rmav_launch_actuator_rollout, rmav_launch_actuator_step, true,
     rmav_launch_actuator_policy_rollout},
    {"start-state", "a handle with a start-state spec", "a handle with a start-state spec (rmav_set_start_state)", rmav_launch_start_rollout, rmav_launch_start_step,
     true, rmav_launch_start_policy_rollout},
    {"termination", "a handle with a termination spec", "a handle with a termination spec (rmav_set_termination)", rmav_launch_term_rollout, rmav_launch_term_step,
     true, rmav_launch_term_policy_rollout},
};
