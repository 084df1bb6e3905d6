// rmav_skip_abi.hip - the launches of a handle with a frame skip (rmav_set_frame_skip; include/rmav.h): the single-step kernels k_step_fs
// and the one-wavefront fused rollouts k_rollout_fs.  A translation unit of its own, as rmav_range_abi.hip and for its reason;
// rmav_abi.hip decides what a call launches and comes here only for the launch itself.  The frame-skip policy rollouts are in
// rmav_policy_abi.hip.
#include "rmav_handle.hpp"

using namespace rmav;

namespace {

template <int K, int MODE> int launch_km(rmav_handle h, int st, const RolloutArgs &a) {
    const KindParams<K> kp = kind_params<K>(h);
    const int64_t count = a.slice_count ? (int64_t)a.slice_count : h->n;
    const dim3 grid((unsigned)((count + block_size(h) - 1) / block_size(h))), block(block_size(h));
    const TimeLimitArgs tl = tl_args(h);
    const RangeArgs dr = range_args(h);
    const FrameSkipArgs fs = skip_args(h);
    // (the ranged kernels' store policies: batch-major obs through the per-lane stores, ST_AOS_LDS runs the write-through kernel)
    return dispatch_store<ST_WRITE_THROUGH, ST_DEFAULT, ST_STREAM>(st, [&](auto s) {
        constexpr int ST = decltype(s)::value;
        if (h->time_limit > 0) hipLaunchKernelGGL((k_rollout_fs<K, MODE, ST, true>), grid, block, 0, h->stream, a, kp.p, kp.pc, tl, dr, fs);
        else hipLaunchKernelGGL((k_rollout_fs<K, MODE, ST, false>), grid, block, 0, h->stream, a, kp.p, kp.pc, tl, dr, fs);
        return (int)RMAV_OK;
    });
}

template <int K> void launch_step(rmav_handle h, const RolloutArgs &a, int bs, const FinalArgs &fa) {
    const KindParams<K> kp = kind_params<K>(h);
    const dim3 grid((unsigned)((h->n + bs - 1) / bs));
    const TimeLimitArgs tl = tl_args(h);
    const RangeArgs dr = range_args(h);
    const FrameSkipArgs fs = skip_args(h);
    // k_step's preloaded leading arguments (StepHot in rmav_kernels.hpp), then the argument block
    if (h->time_limit > 0)
        hipLaunchKernelGGL((k_step_fs<K, true>), grid, dim3(bs), 0, h->stream, a.state, a.n, a.act_in, a.pitch, (uint32_t)bs, a.flags, a.ep_ret, a.rec, a,
                           kp.p, kp.pc, tl, fa, dr, fs);
    else
        hipLaunchKernelGGL((k_step_fs<K, false>), grid, dim3(bs), 0, h->stream, a.state, a.n, a.act_in, a.pitch, (uint32_t)bs, a.flags, a.ep_ret, a.rec, a,
                           kp.p, kp.pc, tl, fa, dr, fs);
}

}  // namespace

int rmav_launch_skip_rollout(rmav_handle h, int mode, int st, const RolloutArgs &a) {
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        switch (mode) {
        case ACT_BUFFER: return launch_km<K, ACT_BUFFER>(h, st, a);
        case ACT_RANDOM: return launch_km<K, ACT_RANDOM>(h, st, a);
        case ACT_CONTROLLER: return launch_km<K, ACT_CONTROLLER>(h, st, a);
        }
        return rmav_fail(RMAV_ERR_INVALID, "no frame-skip kernel for action mode %d", mode);
    });
}

int rmav_launch_skip_step(rmav_handle h, const RolloutArgs &a, int bs, const FinalArgs &fa) {
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) {
        launch_step<decltype(k)::value>(h, a, bs, fa);
        return (int)RMAV_OK;
    });
}
