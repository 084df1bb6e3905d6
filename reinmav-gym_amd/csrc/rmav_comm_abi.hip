// rmav_comm_abi.hip - the C ABI of include/rmav_comm.h: the RCCL loader, the communicator, and the overlapped all-gather of the
// per-env episode statistics (the protocol between a handle's armed rollout launch and the communicator's stream).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <new>

#include <dlfcn.h>

#include "rmav_handle.hpp"
#include "rmav_exchange.hpp"

using namespace rmav;

// =================================================================================================
extern "C" {

// ---- the path's one collective, behind the C ABI: RCCL all-gather of per-env episode statistics ---------------
namespace {
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;      // optional (rmav_comm_info)
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;   // optional
};
// resolved on first use: librmav.so has no link-time dependency on RCCL, and a process that already loaded
// librccl.so.1 (torch does) shares that copy
char g_rccl_path[1024] = "";   // rmav_comm_use_library
bool g_rccl_tried = false;
RcclApi *rccl() {
    static RcclApi api;
    if (!g_rccl_tried) {
        g_rccl_tried = true;
        if (g_rccl_path[0]) {
            api.lib = dlopen(g_rccl_path, RTLD_NOW | RTLD_LOCAL);
        } else {
            for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
                api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
                if (api.lib) break;
            }
        }
        if (api.lib) {
            api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.lib, "ncclGetUniqueId");
            api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.lib, "ncclCommInitRank");
            api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
            api.AllGather = (decltype(api.AllGather))dlsym(api.lib, "ncclAllGather");
            api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
            api.CommCount = (decltype(api.CommCount))dlsym(api.lib, "ncclCommCount");
            api.CommUserRank = (decltype(api.CommUserRank))dlsym(api.lib, "ncclCommUserRank");
            if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllGather) api.lib = nullptr;
        }
    }
    return api.lib ? &api : nullptr;
}
constexpr uint32_t kCommMagic = 0x524d4143u;  // 'RMAC'
#define RCCL_TRY(expr)                                                                             \
    do {                                                                                           \
        ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess)                                                                     \
            return rmav_fail(RMAV_ERR_HIP, "%s failed: %s", #expr, R->GetErrorString ? R->GetErrorString(r_) : "RCCL error"); \
    } while (0)
}  // namespace

int rmav_comm_use_library(const char *path) {
    if (g_rccl_tried) return rmav_fail(RMAV_ERR_INVALID, "the collective library has already been loaded: call this before any other rmav_comm_* function");
    if (!path || !path[0] || strlen(path) >= sizeof(g_rccl_path)) return rmav_fail(RMAV_ERR_INVALID, "path is NULL, empty or too long");
    snprintf(g_rccl_path, sizeof(g_rccl_path), "%s", path);
    return RMAV_OK;
}

int rmav_comm_unique_id(void *id_out) {
    if (!id_out) return rmav_fail(RMAV_ERR_INVALID, "id_out is NULL");
    RcclApi *R = rccl();
    if (!R) return rmav_fail(RMAV_ERR_NO_DEVICE, "librccl.so.1 could not be loaded");
    ncclUniqueId id;
    RCCL_TRY(R->GetUniqueId(&id));
    static_assert(sizeof(id) == RMAV_COMM_ID_BYTES, "RCCL unique id size");
    memcpy(id_out, &id, sizeof(id));
    return RMAV_OK;
}

int rmav_comm_create(rmav_comm *out, const void *id, int rank, int world, int device) {
    if (!out) return rmav_fail(RMAV_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!id || world <= 0 || rank < 0 || rank >= world) return rmav_fail(RMAV_ERR_INVALID, "need id and 0 <= rank < world");
    const int ndev = rmav_device_count();
    if (ndev <= 0) return rmav_fail(RMAV_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return rmav_fail(RMAV_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
    RcclApi *R = rccl();
    if (!R) return rmav_fail(RMAV_ERR_NO_DEVICE, "librccl.so.1 could not be loaded");
    DeviceGuard guard(device);
    if (!guard.ok) return rmav_fail(RMAV_ERR_HIP, "hipSetDevice(%d) failed", device);
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    rmav_comm c = new (std::nothrow) rmav_comm_s();
    if (!c) return rmav_fail(RMAV_ERR_ALLOC, "host allocation failed");
    memset(c, 0, sizeof(*c));
    c->magic = kCommMagic;
    c->rank = rank;
    c->world = world;
    c->device = device;
    ncclResult_t r = R->CommInitRank(&c->comm, world, uid, rank);
    if (r != ncclSuccess) {
        delete c;
        return rmav_fail(RMAV_ERR_HIP, "ncclCommInitRank failed: %s", R->GetErrorString ? R->GetErrorString(r) : "RCCL error");
    }
    // A high-priority stream: HIP multiplexes all streams of one priority onto a few hardware queues (GPU_MAX_HW_QUEUES,
    // 4 by default) round-robin, and a process that also runs torch has dozens - when the communicator's stream lands on
    // the compute stream's hardware queue their packets serialise (measured: a 131 072-env rollout 85 -> 108 us with the
    // default mapping, 189 us with GPU_MAX_HW_QUEUES=8, 93 us with 2).  Priority levels have queues of their own.
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    hipError_t e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_hi);
    c->depth = kExchangeDepth;
    for (int k = 0; k < kExchangeDepth && e == hipSuccess; ++k) {
        // device-scope release: these events only order streams of this GPU
        const unsigned evf = hipEventDisableTiming | hipEventReleaseToDevice;
        e = hipEventCreateWithFlags(&c->ready[k], evf);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->done[k], evf);
    }
    // the words k_wait_arrivals writes when it gives up on an armed launch (pinned host memory: the host reads them for free)
    if (e == hipSuccess) e = hipHostMalloc((void **)&c->timeout_seq, kExchangeDepth * sizeof(uint32_t), hipHostMallocMapped);
    if (e == hipSuccess) {
        memset(c->timeout_seq, 0, kExchangeDepth * sizeof(uint32_t));
        e = hipHostGetDevicePointer((void **)&c->timeout_seq_dev, c->timeout_seq, 0);
    }
    if (e == hipSuccess) e = hipMalloc((void **)&c->started, sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(c->started, 0, sizeof(uint32_t));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)rmav_comm_destroy(c);
        return rmav_fail(RMAV_ERR_HIP, "stream / event creation for the communicator failed: %s", hipGetErrorString(e));
    }
    // Hand-over from the compute stream to the communicator's stream without an event: hipEventRecord puts a barrier
    // packet into the COMPUTE stream (~8 us in front of the next rollout launch, measured); a one-thread kernel that
    // publishes the post number in a signal word, and hipStreamWaitValue32 on the communicator's stream, cost the
    // compute stream one tiny launch (hipStreamWriteValue32 in its place: +3 us per post, measured).  Falls back to the event when the device cannot wait on memory.
    int can_wait = 0;
    (void)hipDeviceGetAttribute(&can_wait, hipDeviceAttributeCanUseStreamWaitValue, device);
    if (can_wait) {
        if (hipExtMallocWithFlags((void **)&c->flag, 8, hipMallocSignalMemory) != hipSuccess) {
            (void)hipGetLastError();
            c->flag = nullptr;
        } else {
            (void)hipMemset(c->flag, 0, 8);
        }
    }
    *out = c;
    return RMAV_OK;
}

int rmav_comm_destroy(rmav_comm c) {
    if (!c || c->magic != kCommMagic) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_comm");
    DeviceGuard guard(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    RcclApi *R = rccl();
    if (R && c->comm) (void)R->CommDestroy(c->comm);
    for (int k = 0; k < kExchangeDepth; ++k) {
        if (c->ready[k]) (void)hipEventDestroy(c->ready[k]);
        if (c->done[k]) (void)hipEventDestroy(c->done[k]);
        if (c->send[k]) (void)hipFree(c->send[k]);
        if (c->recv[k]) (void)hipFree(c->recv[k]);
    }
    if (c->flag) (void)hipFree(c->flag);
    if (c->arrive) (void)hipFree(c->arrive);
    if (c->timeout_seq) (void)hipHostFree(c->timeout_seq);
    if (c->started) (void)hipFree(c->started);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->armed_by && c->armed_by->magic == kMagic && c->armed_by->xchg.comm == c) {
        // a handle still points at this communicator: disarm it, or its next rollout would dereference freed memory
        c->armed_by->xchg.armed = c->armed_by->xchg.fired = false;
        c->armed_by->xchg.comm = nullptr;
    }
    c->magic = 0;
    delete c;
    return RMAV_OK;
}

int rmav_comm_info(rmav_comm c, int *rank_out, int *world_out, int *lib_rank_out, int *lib_world_out) {
    if (!c || c->magic != kCommMagic) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_comm");
    if (rank_out) *rank_out = c->rank;
    if (world_out) *world_out = c->world;
    RcclApi *R = rccl();
    int lr = -1, lw = -1;
    if (R && R->CommUserRank && R->CommUserRank(c->comm, &lr) != ncclSuccess) lr = -1;
    if (R && R->CommCount && R->CommCount(c->comm, &lw) != ncclSuccess) lw = -1;
    if (lib_rank_out) *lib_rank_out = lr;
    if (lib_world_out) *lib_world_out = lw;
    return RMAV_OK;
}

int rmav_comm_warmup(rmav_comm c, double timeout_s) {
    if (!c || c->magic != kCommMagic) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_comm");
    RcclApi *R = rccl();
    if (!R) return rmav_fail(RMAV_ERR_NO_DEVICE, "librccl.so.1 could not be loaded");
    DeviceGuard guard(c->device);
    int32_t *buf = nullptr;   // [1 + world]: this rank's word, then the gathered words
    HIP_TRY(hipMalloc((void **)&buf, sizeof(int32_t) * (size_t)(1 + c->world)));
    hipEvent_t ev = nullptr;
    hipError_t e = hipMemsetAsync(buf, 0, sizeof(int32_t) * (size_t)(1 + c->world), c->stream);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    int rc = RMAV_OK;
    if (e != hipSuccess) {
        rc = rmav_fail(RMAV_ERR_HIP, "rmav_comm_warmup: %s", hipGetErrorString(e));
    } else {
        // RCCL connects its transports inside the first collective's enqueue (a host-side exchange with the peers): this is the
        // call that may block when a peer is gone, and it touches no handle's stream
        const ncclResult_t r = R->AllGather(buf, buf + 1, 1, ncclInt32, c->comm, c->stream);
        if (r != ncclSuccess) rc = rmav_fail(RMAV_ERR_HIP, "ncclAllGather failed: %s", R->GetErrorString ? R->GetErrorString(r) : "RCCL error");
    }
    if (rc == RMAV_OK && hipEventRecord(ev, c->stream) != hipSuccess) rc = rmav_fail(RMAV_ERR_HIP, "hipEventRecord failed");
    if (rc == RMAV_OK) {
        timespec t0;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (;;) {
            const hipError_t q = hipEventQuery(ev);
            if (q == hipSuccess) break;
            (void)hipGetLastError();
            if (q != hipErrorNotReady) { rc = rmav_fail(RMAV_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(q)); break; }
            timespec t1;
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if (timeout_s >= 0 && (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec) > timeout_s) {
                rc = rmav_fail(RMAV_ERR_TIMEOUT, "the warm-up collective did not complete within %.3f s", timeout_s);
                break;
            }
            timespec nap = {0, 50000};
            nanosleep(&nap, nullptr);
        }
    }
    // (on a time-out the collective may still be in flight: the buffer and the event are left to the process, not freed under it)
    if (rc != RMAV_ERR_TIMEOUT) {
        if (ev) (void)hipEventDestroy(ev);
        (void)hipFree(buf);
    }
    return rc;
}

namespace {
// shard of rank c->rank out of n_total, checked against the handle
int check_shard(rmav_handle h, rmav_comm c, int64_t n_total, int64_t *cmax_out) {
    if (!c || c->magic != kCommMagic) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_comm");
    if (!(h->flags & RMAV_F_TRACK_EPISODES))
        return rmav_fail(RMAV_ERR_INVALID, "handle was created without RMAV_F_TRACK_EPISODES");
    if (c->device != h->device) return rmav_fail(RMAV_ERR_INVALID, "communicator and handle live on different devices");
    const int64_t W = c->world, base = n_total / W, rem = n_total % W;
    if (n_total <= 0 || base == 0) return rmav_fail(RMAV_ERR_INVALID, "n_total must be >= the number of ranks");
    const int64_t count = base + (c->rank < rem ? 1 : 0), start = c->rank * base + (c->rank < rem ? c->rank : rem);
    if (h->n != count || (int64_t)h->env_base != start)
        return rmav_fail(RMAV_ERR_INVALID, "rank %d of %d must own envs [%lld, %lld) of %lld; the handle owns [%llu, %llu)", c->rank,
                    c->world, (long long)start, (long long)(start + count), (long long)n_total,
                    (unsigned long long)h->env_base, (unsigned long long)(h->env_base + (uint64_t)h->n));
    *cmax_out = base + (rem ? 1 : 0);
    return RMAV_OK;
}
}  // namespace

namespace {
// Common front of _arm and _post: shard check, buffers, and the buffer pair of the next post (host-side back pressure).
int exchange_slot(rmav_handle h, rmav_comm c, int64_t n_total, int64_t *cmax_out, int *slot_out) {
    int64_t cmax = 0;
    if (int rc = check_shard(h, c, n_total, &cmax)) return rc;
    RcclApi *R = rccl();
    if (!R) return rmav_fail(RMAV_ERR_NO_DEVICE, "librccl.so.1 could not be loaded");
    if (cmax > c->cmax) {   // (re)allocate the buffer pairs
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        for (int k = 0; k < c->depth; ++k) {
            if (c->send[k]) (void)hipFree(c->send[k]);
            if (c->recv[k]) (void)hipFree(c->recv[k]);
            c->send[k] = c->recv[k] = nullptr;
            c->used[k] = false;
            if (hipMalloc((void **)&c->send[k], (size_t)(2 * cmax) * sizeof(int32_t)) != hipSuccess ||
                hipMalloc((void **)&c->recv[k], (size_t)(2 * cmax) * sizeof(int32_t) * (size_t)c->world) != hipSuccess) {
                (void)hipGetLastError();
                c->cmax = 0;
                return rmav_fail(RMAV_ERR_ALLOC, "device allocation for the exchange buffers failed");
            }
            // an armed launch writes only this rank's envs: the padding up to cmax stays zero from here on
            HIP_TRY(hipMemsetAsync(c->send[k], 0, (size_t)(2 * cmax) * sizeof(int32_t), c->stream));
        }
        if (c->arrive) (void)hipFree(c->arrive);
        c->arrive = nullptr;
        const size_t words = (size_t)((cmax + 31) / 32);
        if (hipMalloc((void **)&c->arrive, words * sizeof(uint32_t)) != hipSuccess) {
            (void)hipGetLastError();
            c->cmax = 0;
            return rmav_fail(RMAV_ERR_ALLOC, "device allocation for the exchange buffers failed");
        }
        HIP_TRY(hipMemsetAsync(c->arrive, 0, words * sizeof(uint32_t), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->cmax = cmax;
    }
    const int k = c->posts % c->depth;
    // The gather that last used this buffer pair (`depth` posts ago) must have finished before the pack overwrites its
    // send half.  In a GPU-bound loop the host runs far ahead of the device, so with two pairs that gather has usually not
    // even started when the host gets here, and a device-side wait (hipStreamWaitEvent = a barrier packet in the COMPUTE
    // stream) was inserted in front of nearly every pack: +8 us per rollout, measured.  So the HOST waits instead - back
    // pressure that bounds its lead to `depth` rollouts (>= 0.5 ms of queued GPU work at depth 8) and puts nothing into
    // the compute stream.
    if (c->used[k] && hipEventQuery(c->done[k]) != hipSuccess) {
        (void)hipGetLastError();
        HIP_TRY(hipEventSynchronize(c->done[k]));
    }
    *cmax_out = cmax;
    *slot_out = k;
    return RMAV_OK;
}
}  // namespace

int rmav_allgather_stats(rmav_handle h, rmav_comm c, int64_t n_total, float *returns_out, int32_t *lengths_out) {
    if (!returns_out || !lengths_out) return rmav_fail(RMAV_ERR_INVALID, "returns_out / lengths_out are required (device pointers)");
    if (int rc = rmav_allgather_stats_post(h, c, n_total)) return rc;
    return rmav_allgather_stats_result(h, c, n_total, returns_out, lengths_out);
}

int rmav_allgather_stats_post(rmav_handle h, rmav_comm c, int64_t n_total) {
    CHECK_HANDLE(h);
    int64_t cmax = 0;
    int k = 0;
    RcclApi *R = rccl();
    const bool armed = h->xchg.armed;
    if (armed && h->xchg.comm != c) return rmav_fail(RMAV_ERR_INVALID, "the handle's armed exchange belongs to another communicator");
    if (armed) {   // allocated and back-pressured when it was armed
        if (!R) return rmav_fail(RMAV_ERR_NO_DEVICE, "librccl.so.1 could not be loaded");
        if (int rc = check_shard(h, c, n_total, &cmax)) return rc;
        if (cmax != h->xchg.cmax) return rmav_fail(RMAV_ERR_INVALID, "n_total differs from the armed exchange's");
        cmax = h->xchg.cmax;
        k = h->xchg.slot;
        h->xchg.armed = false;
        h->xchg.comm = nullptr;
        c->armed_by = nullptr;
    } else if (int rc = exchange_slot(h, c, n_total, &cmax, &k)) {
        return rc;
    }
    // (the gather that last used this buffer pair has finished - exchange_slot waited for it - so its time-out word is history)
    c->timeout_seq[k] = 0;
    c->slot_seq[k] = (uint32_t)(c->posts + 1);
    c->armed_slot[k] = armed && h->xchg.fired && !h->xchg.stale;
    if (c->armed_slot[k]) {
        // the rollout launch itself wrote the snapshot and its wavefronts' arrival words: nothing enters the compute stream.
        // The wait is bounded (k_wait_arrivals: 2 s from the moment the armed launch begins): past that the waiter poisons this
        // rank's payload, notes the post number in the pair's time-out word and lets the gather go ahead - the peers get their
        // collective either way, and only THIS post reports RMAV_ERR_TIMEOUT.
        hipLaunchKernelGGL(k_wait_arrivals, dim3(1), dim3(256), 0, c->stream, (const uint32_t *)c->arrive, h->xchg.expected,
                           h->xchg.seq, h->xchg.no_start ? (const uint32_t *)nullptr : (const uint32_t *)c->started, kArrivalWaitTicks,
                           kArrivalTotalTicks, c->timeout_seq_dev + k, c->send[k], cmax);
        HIP_TRY(hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_pack_stats, dim3((unsigned)((cmax + 255) / 256)), dim3(256), 0, h->stream,
                           (const float *)h->last_ret, (const EnvRec *)h->rec, h->n, cmax, c->send[k]);
        HIP_TRY(hipGetLastError());
        if (c->flag) {
            const uint32_t seq = (uint32_t)(c->posts + 1);
            hipLaunchKernelGGL(k_signal, dim3(1), dim3(1), 0, h->stream, c->flag, seq);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamWaitValue32(c->stream, c->flag, seq, hipStreamWaitValueGte, 0xFFFFFFFFu));
        } else {
            HIP_TRY(hipEventRecord(c->ready[k], h->stream));
            HIP_TRY(hipStreamWaitEvent(c->stream, c->ready[k], 0));
        }
    }
    RCCL_TRY(R->AllGather(c->send[k], c->recv[k], (size_t)(2 * cmax), ncclInt32, c->comm, c->stream));
    HIP_TRY(hipEventRecord(c->done[k], c->stream));
    c->used[k] = true;
    c->posts += 1;
    return RMAV_OK;
}

int rmav_allgather_stats_arm(rmav_handle h, rmav_comm c, int64_t n_total) {
    CHECK_HANDLE(h);
    if (h->xchg.armed) return rmav_fail(RMAV_ERR_INVALID, "an exchange is already armed on this handle: post it first");
    if (c && c->magic == kCommMagic && c->armed_by && c->armed_by != h)
        return rmav_fail(RMAV_ERR_INVALID, "this communicator is armed by another handle: post that exchange first");
    int64_t cmax = 0;
    int k = 0;
    if (int rc = exchange_slot(h, c, n_total, &cmax, &k)) return rc;
    h->xchg.armed = true;
    h->xchg.fired = false;
    h->xchg.stale = false;
    h->xchg.comm = c;
    c->armed_by = h;
    h->xchg.slot = k;
    h->xchg.cmax = cmax;
    h->xchg.seq = (uint32_t)(c->posts + 1);
    h->xchg.expected = 0;
    return RMAV_OK;
}

int rmav_allgather_stats_result(rmav_handle h, rmav_comm c, int64_t n_total, float *returns_out, int32_t *lengths_out) {
    CHECK_HANDLE(h);
    int64_t cmax = 0;
    if (int rc = check_shard(h, c, n_total, &cmax)) return rc;
    if (!returns_out || !lengths_out) return rmav_fail(RMAV_ERR_INVALID, "returns_out / lengths_out are required (device pointers)");
    if (c->posts == 0 || cmax != c->cmax) return rmav_fail(RMAV_ERR_INVALID, "no exchange of this size has been posted");
    const int k = (c->posts - 1) % c->depth;
    // (known only if the waiter has already run; rmav_allgather_stats_wait knows for certain.  Either way the payload of a
    // timed-out post is poisoned - return NaN, length -1 for this rank's envs - on every rank.)
    if (c->armed_slot[k] && c->timeout_seq[k] == c->slot_seq[k])
        return rmav_fail(RMAV_ERR_TIMEOUT, "the armed rollout launch of this exchange did not complete within 2 s of starting");
    HIP_TRY(hipStreamWaitEvent(h->stream, c->done[k], 0));
    hipLaunchKernelGGL(k_unpack_stats, dim3((unsigned)((n_total + 255) / 256)), dim3(256), 0, h->stream,
                       (const int32_t *)c->recv[k], n_total, (int32_t)c->world, cmax, returns_out, lengths_out);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int rmav_allgather_stats_wait(rmav_comm c, double timeout_s) {
    if (!c || c->magic != kCommMagic) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_comm");
    if (c->posts == 0) return RMAV_OK;
    DeviceGuard guard(c->device);
    const int k = (c->posts - 1) % c->depth;
    timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (;;) {
        const hipError_t e = hipEventQuery(c->done[k]);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) return rmav_fail(RMAV_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        timespec t1;
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if (timeout_s >= 0 && (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec) > timeout_s)
            return rmav_fail(RMAV_ERR_TIMEOUT, "the posted exchange did not complete within %.3f s", timeout_s);
        timespec nap = {0, 50000};
        nanosleep(&nap, nullptr);
    }
    if (c->armed_slot[k] && c->timeout_seq[k] == c->slot_seq[k])
        return rmav_fail(RMAV_ERR_TIMEOUT, "the armed rollout launch of this exchange did not complete within 2 s of starting");
    return RMAV_OK;
}

int rmav_pack_stats(rmav_handle h, int64_t cmax, int32_t *send_out) {
    CHECK_HANDLE(h);
    if (!(h->flags & RMAV_F_TRACK_EPISODES))
        return rmav_fail(RMAV_ERR_INVALID, "handle was created without RMAV_F_TRACK_EPISODES");
    if (!send_out || cmax < h->n) return rmav_fail(RMAV_ERR_INVALID, "send_out is NULL or cmax < num_envs");
    hipLaunchKernelGGL(k_pack_stats, dim3((unsigned)((cmax + 255) / 256)), dim3(256), 0, h->stream,
                       (const float *)h->last_ret, (const EnvRec *)h->rec, h->n, cmax, send_out);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

}  // extern "C"
