// rmav_rung_launch.hpp - what the eight rung units (rmav_range_abi.hip ... rmav_term_abi.hip) share: the trailing argument list of a rung's
// kernels and the two launchers.  A unit names its kernels in a struct
//     struct Kernels {
//         template <int K, int MODE, int ST, bool TL, bool RW> static auto rollout() { return k_rollout_xx<...>; }
//         template <int K, bool CTRL, bool TL, bool RW> static auto step() { return k_step_xx<...>; }
//     };
// which drops the parameters its kernels do not have, and forwards its two rmav_launch_* functions to the launchers below.  A launcher
// resolves only the parameters the rung's kernels take, so a unit instantiates the kernels it names for the values they exist for.
#pragma once

#include <tuple>

#include "rmav_ladder.hpp"

// a run-time flag as std::bool_constant: f is a generic lambda
template <typename F> inline void dispatch_bool(bool v, F &&f) {
    if (v) f(std::true_type{});
    else f(std::false_type{});
}

// What the kernels of rung R take behind tl (the steps: behind tl, fa), in order: dr, fs, rw, ds, sn, al, ss, tc, cut off at R.  Every rung's
// list is that of a rung below it with its own slots appended; a slot that follows changes its provider where the rung above has to stand in
// for a feature the handle may not have:
//   ds  the handle's disturbance at its own rung, disturb_or_calm above (the all-zero spec without one)
//   al  actuator_args at its own rung, start_actuator_args above (zeros and no array without one)
//   ss  start_args at its own rung, term_start_args above (the identity coefficients without one)
// t0: the step counter of the launch's first step (RolloutArgs::t0).
template <Rung R> RMAV_INTERNAL inline auto rung_tail(const rmav_env_s *h, uint64_t t0) {
    static_assert(R >= RUNG_RANGE && R <= RUNG_TERM, "a rung of the ladder");
    if constexpr (R == RUNG_RANGE) return std::make_tuple(range_args(h));
    else if constexpr (R == RUNG_SKIP) return std::tuple_cat(rung_tail<RUNG_RANGE>(h, t0), std::make_tuple(skip_args(h)));
    else if constexpr (R == RUNG_REWARD) return std::tuple_cat(rung_tail<RUNG_SKIP>(h, t0), std::make_tuple(reward_args(h)));
    else if constexpr (R == RUNG_DISTURB) return std::tuple_cat(rung_tail<RUNG_REWARD>(h, t0), std::make_tuple(disturb_args(h, t0)));
    else if constexpr (R == RUNG_SENSOR) return std::tuple_cat(rung_tail<RUNG_REWARD>(h, t0), std::make_tuple(disturb_or_calm(h, t0), sensor_args(h)));
    else if constexpr (R == RUNG_ACTUATOR) return std::tuple_cat(rung_tail<RUNG_SENSOR>(h, t0), std::make_tuple(actuator_args(h)));
    else if constexpr (R == RUNG_START) return std::tuple_cat(rung_tail<RUNG_SENSOR>(h, t0), std::make_tuple(start_actuator_args(h), start_args(h)));
    else return std::tuple_cat(rung_tail<RUNG_SENSOR>(h, t0), std::make_tuple(start_actuator_args(h), term_start_args(h), term_args(h)));
}

// The rungs up to the tracking reward have kernels <K, MODE, ST, TL> for three store policies (batch-major obs through the per-lane stores:
// there is no LDS-transposing kernel, ST_AOS_LDS runs the write-through one) and take the reward - if they take one - unconditionally; the
// rungs above have one store policy and the handle's reward choice as a template parameter, <K, MODE, TL, RW>.
template <Rung R> constexpr bool kRungByStore = R <= RUNG_REWARD;

// ONE launch of the rung's fused rollout over the envs a names (mode = ACT_BUFFER | ACT_RANDOM | ACT_CONTROLLER, st = a store policy).  The
// caller checks hipGetLastError.
template <Rung R, typename KN, int K, int MODE> RMAV_INTERNAL inline int launch_rung_rollout_km(rmav_handle h, int st, const rmav::RolloutArgs &a) {
    using namespace rmav;
    const KindParams<K> kp = kind_params<K>(h);
    const int64_t count = a.slice_count ? (int64_t)a.slice_count : h->n;
    const dim3 grid((unsigned)((count + block_size(h) - 1) / block_size(h))), block(block_size(h));
    const TimeLimitArgs tl = tl_args(h);
    std::apply(
        [&](const auto &...tail) {
            auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, h->stream, a, kp.p, kp.pc, tl, tail...); };
            dispatch_bool(h->time_limit > 0, [&](auto limited) {
                constexpr bool TL = decltype(limited)::value;
                if constexpr (kRungByStore<R>)
                    dispatch_store<ST_WRITE_THROUGH, ST_DEFAULT, ST_STREAM>(st, [&](auto s) { launch(KN::template rollout<K, MODE, decltype(s)::value, TL, false>()); });
                else
                    dispatch_bool(h->reward_on != 0, [&](auto rw) { launch(KN::template rollout<K, MODE, ST_DEFAULT, TL, decltype(rw)::value>()); });
            });
        },
        rung_tail<R>(h, a.t0));
    return RMAV_OK;
}
template <Rung R, typename KN> RMAV_INTERNAL inline int launch_rung_rollout(rmav_handle h, int mode, int st, const rmav::RolloutArgs &a) {
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        switch (mode) {
        case rmav::ACT_BUFFER: return launch_rung_rollout_km<R, KN, K, rmav::ACT_BUFFER>(h, st, a);
        case rmav::ACT_RANDOM: return launch_rung_rollout_km<R, KN, K, rmav::ACT_RANDOM>(h, st, a);
        case rmav::ACT_CONTROLLER: return launch_rung_rollout_km<R, KN, K, rmav::ACT_CONTROLLER>(h, st, a);
        }
        return rmav_fail(RMAV_ERR_INVALID, "no %s kernel for action mode %d", kLadder[R].noun, mode);
    });
}

// The rung's single step at bs threads per workgroup; fa = what rmav_step_final wants (NULL pointers otherwise).  ctrl: the ranged kernel has
// a form that ends with control(), the other rungs ignore it.  The caller checks hipGetLastError.
template <Rung R, typename KN> RMAV_INTERNAL inline int launch_rung_step(rmav_handle h, const rmav::RolloutArgs &a, bool ctrl, int bs, const rmav::FinalArgs &fa) {
    using namespace rmav;
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        const KindParams<K> kp = kind_params<K>(h);
        const dim3 grid((unsigned)((h->n + bs - 1) / bs));
        const TimeLimitArgs tl = tl_args(h);
        std::apply(
            [&](const auto &...tail) {
                // k_step's preloaded leading arguments (StepHot in rmav_kernels.hpp), then the argument block
                auto launch = [&](auto kernel) {
                    hipLaunchKernelGGL(kernel, grid, dim3(bs), 0, h->stream, a.state, a.n, a.act_in, a.pitch, (uint32_t)bs, a.flags, a.ep_ret, a.rec, a, kp.p, kp.pc, tl,
                                       fa, tail...);
                };
                dispatch_bool(h->time_limit > 0, [&](auto limited) {
                    constexpr bool TL = decltype(limited)::value;
                    if constexpr (R == RUNG_RANGE) dispatch_bool(ctrl, [&](auto c) { launch(KN::template step<K, decltype(c)::value, TL, false>()); });
                    else if constexpr (kRungByStore<R>) launch(KN::template step<K, false, TL, false>());
                    else dispatch_bool(h->reward_on != 0, [&](auto rw) { launch(KN::template step<K, false, TL, decltype(rw)::value>()); });
                });
            },
            rung_tail<R>(h, a.t0));
        return (int)RMAV_OK;
    });
}
