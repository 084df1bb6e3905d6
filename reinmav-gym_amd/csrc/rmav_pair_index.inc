// rmav_pair_index.inc - which wavefront of which pair a thread is, and the env its lane works on: the first statements after the type
// aliases of both pair bodies (rmav_pair_body.inc, rmav_pair_shared_body.inc), shared textually as the bodies themselves are.
//   expects:  the kernel argument a (RolloutArgs: n, n_steps, flags); F_TRACK, F_AUTO_RESET
//   defines:  G (pairs per workgroup), wave, helper (the pair's second wavefront: the critic / wavefront B), pair, lane, h (the
//             half-wave), gi, n, valid, li (a lane past the end of the batch is a clone of env n - 1), col, off (bytes between the
//             components of an SoA block; this lane's byte offset inside one), T, track, auto_reset - all const
//   modifies: nothing
//   barriers: none (in front of the weight staging and its two barriers)
    const uint32_t G = blockDim.x >> 7;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool helper = wave >= G;
    const uint32_t pair = helper ? wave - G : wave, lane = threadIdx.x & 63u, h = lane >> 5;
    const uint32_t gi = (blockIdx.x * G + pair) * 64u + lane;
    const int64_t n = a.n;
    const bool valid = gi < (uint64_t)n;
    const uint32_t li = valid ? gi : (uint32_t)n - 1u;
    const uint32_t col = (uint32_t)n * 4u, off = li * 4u;
    const int32_t T = a.n_steps;
    const bool track = (a.flags & F_TRACK) != 0, auto_reset = (a.flags & F_AUTO_RESET) != 0;
