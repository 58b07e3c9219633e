// part.hip — multi-GPU engine: 1-D vertex-range partition of the slots over the GPUs of one node
// (one process per GPU), frontier exchange with RCCL over xGMI.
//
// Rank p owns slots [p*B, p*B + n_local), B = ceil(N / world): their node words and their
// `_usedBy` rows (entries keep the GLOBAL dependant slot). Every rank also holds a replica of all
// N versions (versions never change during a wave), so the rank that traverses an edge to a
// remote slot checks the tag against the version itself and forwards only matching targets. A
// per-wave "sent" bitmap forwards each remote target at most once per wave: a node's first visit
// in a wave is the only one that can change it (Computed.cs:164-191 — later visits find it
// Invalidated, or the flag already set), so dropping the repeats is exact.
//
// Per level (run_part_wave, wave.hip): all-reduce of the level's frontier and its edges (push vs
// pull, termination); a push level expands locally (k_level<true>), all-gathers the per-owner
// counts, moves the targets by grouped send/recv and the owners apply them (k_apply_recv); a pull
// level all-gathers the frontier bitmap and every rank pulls its own slots.
//
// The bytes move behind PartComm, which has three transports: RcclComm (one process per GPU, RCCL over
// xGMI), HostComm (one process per rank, every collective an all-gather the host supplies) and
// LocalComm (an in-process group of P graphs driven by P host threads, device copies between their
// buffers). A transport knows five things: a few words of every rank on every host (gather_words), the
// per-level sum of device words (allreduce_sum), the in-place sum of a device u32 array (allreduce_u32),
// fixed-size stream-ordered moves (allgather_dev, alltoall_dev) and device byte ranges with per-peer
// counts (alltoallv). The wave's and the loads' protocols (part_exchange, part_allgather_front,
// part_allgatherv, ...) are written once above them, so all three transports run the same
// run_part_wave and the in-process tests execute exactly the level sequence a multi-GPU run does.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <dlfcn.h>
#include <sched.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "fgi_internal.h"

namespace fgi {

// What a transport must know (every rank calls these in the same order). Ranges of length 0 are legal
// everywhere and move nothing.
constexpr uint64_t kPairUnknown = ~0ull;   // alltoallv: the caller does not know the other ranks' pair sizes
struct PartComm {
    virtual ~PartComm() {}
    // words (<= kPartRedMax) u64 of every rank into all[world][words] on every host; src is device memory
    // (final once the stream has run this far) or host memory. Returns with `all` filled: the stream has
    // run up to here if src is on the device. `what` names the collective in a timeout's message.
    virtual fgi_status gather_words(fgi_graph* g, const unsigned long long* src, bool src_dev, uint32_t words, uint64_t* all,
                                    const char* what) = 0;
    // sum of `count` device u64 over all ranks, returned on the host (the stream has run up to here):
    // the words of every rank gathered on the host and summed there, unless the transport sums on the device
    virtual fgi_status allreduce_sum(fgi_graph* g, const unsigned long long* dev_val, uint64_t* out, uint32_t count) {
        uint64_t all[8 * kPartRedMax];
        FGI_TRY(gather_words(g, dev_val, true, count, all, "all-reduce (wave counters)"));
        for (uint32_t i = 0; i < count; ++i) {
            out[i] = 0;
            for (uint32_t q = 0; q < (uint32_t)g->world; ++q) out[i] += all[(size_t)q * count + i];
        }
        return FGI_OK;
    }
    // the element-wise sum of a device u32 array over all ranks, in place (synchronises)
    virtual fgi_status allreduce_u32(fgi_graph* g, uint32_t* dev, uint64_t n) = 0;
    // Fixed size, stream-ordered (the next kernels on the stream see dst; the host need not wait):
    // every rank's src[0, bytes) into dst[q * bytes, + bytes) / src[q * bytes, + bytes) to rank q, which
    // finds it at its dst[this rank * bytes, + bytes)
    virtual fgi_status allgather_dev(fgi_graph* g, const void* src, void* dst, uint64_t bytes) = 0;
    virtual fgi_status alltoall_dev(fgi_graph* g, const void* src, void* dst, uint64_t bytes) = 0;
    // Device byte ranges with per-peer counts: src + soff[q] (sbytes[q] bytes) goes to rank q, which finds it
    // at its dst + roff[this rank]; rbytes[q] bytes arrive from rank q. src and dst do not overlap.
    // max_pair_bytes: the largest range of any pair of ranks if the caller knows it (from all-gathered
    // counts), kPairUnknown if not. wait: return with the data in place and src free to reuse; otherwise
    // the result is stream-ordered (and src is reused only by later work on the stream).
    virtual fgi_status alltoallv(fgi_graph* g, const void* src, const uint64_t* soff, const uint64_t* sbytes, void* dst,
                                 const uint64_t* roff, const uint64_t* rbytes, uint64_t max_pair_bytes, bool wait,
                                 const char* what) = 0;
    // src[0, bytes[rank]) of every rank, concatenated in rank order at dst (bytes: [world], known to all);
    // returns with the data in place. Through alltoallv (allgatherv_pairs) unless the transport has a shorter way.
    virtual fgi_status allgatherv(fgi_graph* g, const void* src, const uint64_t* bytes, void* dst);
};

static fgi_status allgatherv_pairs(fgi_graph* g, PartComm& c, const void* src, const uint64_t* bytes, void* dst) {
    uint64_t soff[8], sb[8], roff[8], at = 0, mx = 0;
    for (uint32_t q = 0; q < (uint32_t)g->world; ++q) {
        soff[q] = 0;
        sb[q] = bytes[g->rank];
        roff[q] = at;
        at += bytes[q];
        mx = std::max(mx, bytes[q]);
    }
    return c.alltoallv(g, src, soff, sb, dst, roff, bytes, mx, true, "variable-size all-gather of a sharded load");
}
fgi_status PartComm::allgatherv(fgi_graph* g, const void* src, const uint64_t* bytes, void* dst) {
    return allgatherv_pairs(g, *this, src, bytes, dst);
}

struct PartState {
    PartView v{};
    ncclComm_t comm = nullptr;
    std::unique_ptr<PartComm> ops;
    // gather_words over RCCL: [1 + world][kPartRedMax], this rank's words (when they come from the host)
    // and everyone's; on the device and pinned on the host
    unsigned long long* gw = nullptr;
    unsigned long long* gw_host = nullptr;
    unsigned long long* scalar = nullptr;      // device scratch for all-reduce
    unsigned long long* scalar_host = nullptr;
    // In-store: the dependency entries of the owned slots, as loaded (dependant local << 32 | used
    // global, tag). The owners of the `used` ends hold these entries in their rows; the owner of the
    // dependant keeps its own copy so it can rebuild its pull lists (part_rebuild_lists) without an
    // exchange whenever its node versions change.
    uint64_t* in_keys = nullptr;
    uint64_t* in_tags = nullptr;
    uint64_t in_n = 0, in_cap = 0;
    uint32_t* weight = nullptr;                // [n_global] live dependencies per slot (list order)
    // delta frontier exchange (part_allgather_front): this rank's changed bitmap words since the last
    // exchange, and the other ranks' received ones (global word index << 32 | word)
    uint64_t* dbuf = nullptr;                  // [block / 32]
    uint64_t* rbuf = nullptr;                  // [(world - 1) * block / 32]
    unsigned long long* dcnt = nullptr;        // device count of dbuf
    uint64_t front_full = 0, front_delta = 0;  // exchanges of each kind (statistics)
    uint64_t front_bytes = 0;                  // bytes received by this rank's frontier exchanges
    // planned waves (run_part_wave): the targets a push level forwards move in fixed-size buckets,
    // a2a_C words per peer (count, then up to a2a_C - 1 ids); what does not fit waits in send_buf
    // (a2a_cur: the next id to pack per owner) for the next push level
    uint32_t a2a_C = 0;                        // words per peer in use (<= a2a_cap; FGI_OPT_PART_BUCKET)
    uint32_t a2a_cap = 0;                      // words per peer allocated
    uint32_t* a2a_send = nullptr;              // [world][a2a_C]
    uint32_t* a2a_recv = nullptr;              // [world][a2a_C]
    unsigned long long* a2a_cur = nullptr;     // [world]
    unsigned long long* red = nullptr;         // [kPartRedMax] device all-reduce buffer (planned waves)
    unsigned long long* red_host = nullptr;
    // partitioned prune: the current-node bits of the owned slots (W64 words, padded per rank) and
    // every rank's, all-gathered (allocated on first use)
    uint64_t cur_w64 = 0;
    unsigned long long* cur_local = nullptr;
    unsigned long long* cur_all = nullptr;
    std::vector<uint32_t> u32_host[2];         // allreduce_u32's host copies (in-process groups: LocalComm::meet)
    uint32_t* roots_codes = nullptr;           // fgi_part_invalidate's roots as codes (partition codes)
    uint64_t roots_cap = 0;
};

static PartState* ps(fgi_graph* g) { return reinterpret_cast<PartState*>(g->part); }

// ---- the RCCL the engine binds to ----------------------------------------------------------------
// libfgi does not link librccl: a process that loaded another librccl with the same soname first
// (torch's bundled copy) would otherwise bind the engine's collectives to that one. The entry points
// are resolved from /opt/rocm's librccl (the one the engine is built against, FGI_RCCL_LIBRARY
// overrides the path), opened RTLD_LOCAL, once per process: every collective below goes through
// this table.
struct RcclApi {
    void* lib = nullptr;
    std::string path;
    decltype(&ncclGetVersion) GetVersion = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitRankConfig) CommInitRankConfig = nullptr;
    decltype(&ncclCommGetAsyncError) CommGetAsyncError = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclAllToAll) AllToAll = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    std::string err;
};

static const RcclApi& rccl() {
    static const RcclApi api = [] {
        RcclApi a;
        const char* env = getenv("FGI_RCCL_LIBRARY");
        a.path = env && *env ? env : "/opt/rocm/lib/librccl.so.1";
        a.lib = dlopen(a.path.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!a.lib) {
            const char* e = dlerror();
            a.err = e ? e : "dlopen failed";
            return a;
        }
        bool ok = true;
        auto sym = [&](auto& fn, const char* name) {
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(a.lib, name));
            if (!fn) {
                ok = false;
                a.err = std::string("missing ") + name;
            }
        };
        sym(a.GetVersion, "ncclGetVersion");
        sym(a.GetUniqueId, "ncclGetUniqueId");
        sym(a.CommInitRank, "ncclCommInitRank");
        sym(a.CommInitRankConfig, "ncclCommInitRankConfig");
        sym(a.CommGetAsyncError, "ncclCommGetAsyncError");
        sym(a.CommAbort, "ncclCommAbort");
        sym(a.CommDestroy, "ncclCommDestroy");
        sym(a.GetErrorString, "ncclGetErrorString");
        sym(a.AllReduce, "ncclAllReduce");
        sym(a.AllGather, "ncclAllGather");
        sym(a.AllToAll, "ncclAllToAll");
        sym(a.Send, "ncclSend");
        sym(a.Recv, "ncclRecv");
        sym(a.GroupStart, "ncclGroupStart");
        sym(a.GroupEnd, "ncclGroupEnd");
        if (!ok) {
            dlclose(a.lib);
            a.lib = nullptr;
        }
        return a;
    }();
    return api;
}

static bool rccl_ok() { return rccl().lib != nullptr; }

// c: [W][W + 2] all-gathered counts (targets sent by q to r, then q's next-level F, T)
static void sum_counts(const uint64_t* c, uint32_t W, uint64_t* glob) {
    const uint32_t S = W + 2;
    glob[0] = glob[1] = glob[2] = 0;
    for (uint32_t q = 0; q < W; ++q) {
        glob[0] += c[(size_t)q * S + W];
        glob[1] += c[(size_t)q * S + W + 1];
        for (uint32_t r = 0; r < W; ++r)
            if (r != q) glob[2] += c[(size_t)q * S + r];
    }
}

fgi_status part_destroy(fgi_graph* g) {
    PartState* p = ps(g);
    if (!p) return FGI_OK;
    p->ops.reset();
    if (p->comm) rccl().CommDestroy(p->comm);
    hipFree(p->v.ver_all);
    hipFree(p->v.sent_bm);
    hipFree(p->v.send_buf);
    hipFree(p->v.recv_buf);
    hipFree(p->v.send_cnt);
    hipFree(p->gw);
    hipFree(p->scalar);
    hipFree(p->v.front_global);
    hipFree(p->v.scratch_u64);
    hipFree(p->in_keys);
    hipFree(p->in_tags);
    hipFree(p->weight);
    hipFree(p->dbuf);
    hipFree(p->rbuf);
    hipFree(p->dcnt);
    hipFree(p->a2a_send);
    hipFree(p->a2a_recv);
    hipFree(p->a2a_cur);
    hipFree(p->red);
    hipFree(p->cur_local);
    hipFree(p->cur_all);
    hipFree(p->roots_codes);
    if (p->red_host) hipHostFree(p->red_host);
    if (p->gw_host) hipHostFree(p->gw_host);
    if (p->scalar_host) hipHostFree(p->scalar_host);
    delete p;
    g->part = nullptr;
    hipFree(g->pg_gc);
    hipFree(g->pg_ig);
    g->pg_gc = g->pg_ig = nullptr;
    g->pg_gc_h.clear();
    g->pg_ig_h.clear();
    g->lbl_perm = false;
    g->pg_hash = 0;
    return FGI_OK;
}

bool part_view(fgi_graph* g, PartView* v) {
    PartState* p = ps(g);
    if (!p) return false;
    *v = p->v;
    return true;
}

// ---- bounded waits on the RCCL path (fail fast, never hang) ------------------------------------------
// A rank whose peer never joins a collective would otherwise wait forever: in ncclCommInitRank, in a
// grouped send/recv's connection setup, or on its stream behind a collective kernel. The communicator
// is non-blocking (ncclConfig_t.blocking = 0): every RCCL call that reports ncclInProgress is polled
// through ncclCommGetAsyncError, and every host wait behind a collective polls the stream, each for at
// most FGI_WAIT_TIMEOUT_S seconds (default 300; FGI_RCCL_INIT_TIMEOUT_S, default 120, for the
// communicator's creation). On timeout the communicator is aborted (its kernels leave), the graph is
// marked failed and the call returns FGI_EDEVICE naming the rank and the collective.
static double wait_limit_s(const char* var, double dflt) {
    const char* e = getenv(var);
    return e && *e ? atof(e) : dflt;
}
static double comm_limit_s() { return wait_limit_s("FGI_WAIT_TIMEOUT_S", 300.0); }

static fgi_status comm_fail(fgi_graph* g, const char* what, double limit_s) {
    PartState* p = ps(g);
    if (p && p->comm && rccl().CommAbort) {
        rccl().CommAbort(p->comm);
        p->comm = nullptr;
    }
    g->failed = true;
    return set_err(g, FGI_EDEVICE, "rank %d of %d: %s did not complete within %.0f s (a peer missing or stuck); "
                                   "the communicator was aborted", g->rank, g->world, what, limit_s);
}

// an RCCL call's result: ncclInProgress (non-blocking communicator) is waited out, bounded
static fgi_status nccl_settle(fgi_graph* g, ncclComm_t comm, ncclResult_t r, const char* what, double limit_s) {
    if (r == ncclInProgress && comm && rccl().CommGetAsyncError) {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint64_t k = 0; r == ncclInProgress; ++k) {
            if (rccl().CommGetAsyncError(comm, &r) != ncclSuccess) break;
            if (r != ncclInProgress) break;
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s)
                return comm_fail(g, what, limit_s);
            if (k > 1024) sched_yield();
        }
    }
    if (r == ncclSuccess) return FGI_OK;
    g->failed = true;
    return set_err(g, FGI_EDEVICE, "rank %d of %d: %s: %s", g->rank, g->world, what, rccl().GetErrorString(r));
}
#define FGI_NCCL(g, call)                                                                                  \
    do {                                                                                                   \
        ncclResult_t _r = (call);                                                                          \
        if (_r != ncclSuccess)                                                                             \
            FGI_TRY(nccl_settle((g), ps(g) ? ps(g)->comm : nullptr, _r, #call, comm_limit_s()));           \
    } while (0)

// the host's wait behind this rank's collectives: the stream polled, bounded
static fgi_status comm_sync(fgi_graph* g, hipStream_t s, const char* what) {
    const double limit_s = comm_limit_s();
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t k = 0;; ++k) {
        const hipError_t e = hipStreamQuery(s);
        if (e == hipSuccess) return FGI_OK;
        if (e != hipErrorNotReady) return hip_check(g, e, what);
        if ((k & 255) == 0 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s)
            return comm_fail(g, what, limit_s);
        if (k < 4096) __builtin_ia32_pause();
        else sched_yield();
    }
}

// ---- RCCL (one process per GPU) ----------------------------------------------------------------
// At world size 1 nothing moves through RCCL (device copies instead) unless FGI_OPT_PART_COLLECTIVES
// forces it. Only gather_words, allreduce_sum, allreduce_u32 and alltoallv(wait) make the host wait.
struct RcclComm final : PartComm {
    static bool through_rccl(fgi_graph* g) { return ps(g)->v.world > 1 || g->opt_part_coll; }

    fgi_status gather_words(fgi_graph* g, const unsigned long long* src, bool src_dev, uint32_t words, uint64_t* all,
                            const char* what) override {
        PartState* p = ps(g);
        const uint32_t W = p->v.world;
        hipStream_t s = g->stream;
        if (!src_dev && !through_rccl(g)) {   // one rank, host words: nothing to move
            std::memcpy(all, src, 8ull * words);
            return FGI_OK;
        }
        unsigned long long* every = p->gw_host + kPartRedMax;   // [W][words]
        if (!src_dev) {
            std::memcpy(p->gw_host, src, 8ull * words);
            FGI_HIP(g, hipMemcpyAsync(p->gw, p->gw_host, 8ull * words, hipMemcpyHostToDevice, s));
            src = p->gw;
        }
        if (through_rccl(g)) {
            FGI_NCCL(g, rccl().AllGather(src, p->gw + kPartRedMax, words, ncclUint64, p->comm, s));
            src = p->gw + kPartRedMax;
        }
        FGI_HIP(g, hipMemcpyAsync(every, src, (size_t)W * words * 8, hipMemcpyDeviceToHost, s));
        FGI_TRY(comm_sync(g, s, what));
        for (size_t i = 0; i < (size_t)W * words; ++i) all[i] = every[i];
        return FGI_OK;
    }
    // summed on the device, into the words the host spins on
    fgi_status allreduce_sum(fgi_graph* g, const unsigned long long* dev_val, uint64_t* out, uint32_t count) override {
        PartState* p = ps(g);
        hipStream_t s = g->stream;
        const bool big = count > 4;
        unsigned long long* dst = big ? p->red : p->scalar;
        unsigned long long* host = big ? p->red_host : p->scalar_host;
        const unsigned long long* src = dev_val;   // one rank: the sum is the value
        if (through_rccl(g)) {
            FGI_NCCL(g, rccl().AllReduce(dev_val, dst, count, ncclUint64, ncclSum, p->comm, s));
            src = dst;
        }
#if FGI_SPIN_WAIT
        (void)host;
        // the host spins instead of a stream sync (publish_wait is bounded by FGI_WAIT_TIMEOUT_S too)
        if (publish_wait(g, s, src, count, g->red_pub) != FGI_OK)
            return comm_fail(g, "all-reduce (wave counters)", comm_limit_s());
        for (uint32_t i = 0; i < count; ++i) out[i] = g->red_pub[i];
#else
        FGI_HIP(g, hipMemcpyAsync(host, src, 8 * count, hipMemcpyDeviceToHost, s));
        FGI_TRY(comm_sync(g, s, "all-reduce (wave counters)"));
        for (uint32_t i = 0; i < count; ++i) out[i] = host[i];
#endif
        return FGI_OK;
    }
    fgi_status allreduce_u32(fgi_graph* g, uint32_t* dev, uint64_t n) override {
        if (n && through_rccl(g))
            FGI_NCCL(g, rccl().AllReduce(dev, dev, n, ncclUint32, ncclSum, ps(g)->comm, g->stream));
        return comm_sync(g, g->stream, "all-reduce (u32)");
    }
    fgi_status allgather_dev(fgi_graph* g, const void* src, void* dst, uint64_t bytes) override {
        if (through_rccl(g))
            FGI_NCCL(g, rccl().AllGather(src, dst, bytes, ncclUint8, ps(g)->comm, g->stream));
        else if (bytes)
            FGI_HIP(g, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, g->stream));
        return FGI_OK;
    }
    fgi_status alltoall_dev(fgi_graph* g, const void* src, void* dst, uint64_t bytes) override {
        if (through_rccl(g))
            FGI_NCCL(g, rccl().AllToAll(src, dst, bytes, ncclUint8, ps(g)->comm, g->stream));
        else if (bytes)
            FGI_HIP(g, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, g->stream));
        return FGI_OK;
    }
    // the engine's one grouped send/recv: every variable-size exchange (a push level's targets, the delta
    // frontier lists, the sharded loads) comes through here
    fgi_status alltoallv(fgi_graph* g, const void* src, const uint64_t* soff, const uint64_t* sbytes, void* dst,
                         const uint64_t* roff, const uint64_t* rbytes, uint64_t, bool wait, const char* what) override {
        PartState* p = ps(g);
        const uint32_t W = p->v.world;
        const char* s8 = static_cast<const char*>(src);
        char* d8 = static_cast<char*>(dst);
        if (!through_rccl(g)) {
            if (rbytes[0])
                FGI_HIP(g, hipMemcpyAsync(d8 + roff[0], s8 + soff[0], rbytes[0], hipMemcpyDeviceToDevice, g->stream));
        } else {
            FGI_NCCL(g, rccl().GroupStart());
            for (uint32_t q = 0; q < W; ++q) {
                if (sbytes[q]) FGI_NCCL(g, rccl().Send(s8 + soff[q], sbytes[q], ncclUint8, (int)q, p->comm, g->stream));
                if (rbytes[q]) FGI_NCCL(g, rccl().Recv(d8 + roff[q], rbytes[q], ncclUint8, (int)q, p->comm, g->stream));
            }
            FGI_NCCL(g, rccl().GroupEnd());
        }
        return wait ? comm_sync(g, g->stream, what) : FGI_OK;
    }
};

// ---- host collectives (one process per rank, the host's own transport) -------------------------------
// Every collective reduces to one primitive the caller supplies (fgi_part_init_host): an all-gather of
// equal-size host buffers, e.g. torch.distributed over gloo. The ranks then need not sit on distinct
// GPUs (RCCL refuses two ranks on one device), so the planned and host-driven waves, the mutations and
// the prune of run_part_wave execute across real process boundaries on any box. Each collective
// synchronises the rank's stream, moves its part through host memory and copies the result back:
// correct, not fast (the stream-ordered primitives are synchronous here).
struct HostComm final : PartComm {
    fgi_allgather_fn fn;
    void* ctx;
    std::vector<uint8_t> sbuf, rbuf;
    HostComm(fgi_allgather_fn f, void* c) : fn(f), ctx(c) {}

    // all-gather `bytes` from sbuf into rbuf (world * bytes)
    fgi_status gather(fgi_graph* g, uint64_t bytes) {
        const uint32_t W = ps(g)->v.world;
        rbuf.resize((size_t)W * bytes + 1);
        if (sbuf.size() < bytes) sbuf.resize(bytes);
        const int rc = fn(ctx, sbuf.data(), bytes, rbuf.data());
        if (rc == 0) return FGI_OK;
        g->failed = true;   // a collective of the wave's protocol is missing on this rank: its state is undefined
        return set_err(g, FGI_EDEVICE, "rank %d of %d: host all-gather of %llu bytes failed (%d; a peer missing?)", g->rank,
                       g->world, (unsigned long long)bytes, rc);
    }
    // device -> sbuf (synchronises the stream: the device words are final)
    fgi_status stage(fgi_graph* g, const void* dev, uint64_t bytes, uint64_t at = 0) {
        if (sbuf.size() < at + bytes) sbuf.resize(at + bytes);
        if (bytes) FGI_HIP(g, hipMemcpyAsync(sbuf.data() + at, dev, bytes, hipMemcpyDeviceToHost, g->stream));
        FGI_HIP(g, hipStreamSynchronize(g->stream));
        return FGI_OK;
    }
    fgi_status upload(fgi_graph* g, void* dev, const void* host, uint64_t bytes) {
        if (bytes) FGI_HIP(g, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, g->stream));
        FGI_HIP(g, hipStreamSynchronize(g->stream));   // the host buffer is reused by the next collective
        return FGI_OK;
    }

    fgi_status gather_words(fgi_graph* g, const unsigned long long* src, bool src_dev, uint32_t words, uint64_t* all,
                            const char*) override {
        if (src_dev) {
            FGI_TRY(stage(g, src, 8ull * words));
        } else {
            if (sbuf.size() < 8ull * words) sbuf.resize(8ull * words);
            std::memcpy(sbuf.data(), src, 8ull * words);
        }
        FGI_TRY(gather(g, 8ull * words));
        std::memcpy(all, rbuf.data(), (size_t)ps(g)->v.world * words * 8);
        return FGI_OK;
    }
    fgi_status allreduce_u32(fgi_graph* g, uint32_t* dev, uint64_t n) override {
        const uint32_t W = ps(g)->v.world;
        FGI_TRY(stage(g, dev, n * 4));
        FGI_TRY(gather(g, n * 4));
        std::vector<uint32_t> sum(n, 0);
        for (uint32_t q = 0; q < W; ++q) {
            const uint32_t* v = reinterpret_cast<const uint32_t*>(rbuf.data() + (size_t)q * n * 4);
            for (uint64_t i = 0; i < n; ++i) sum[i] += v[i];
        }
        return upload(g, dev, sum.data(), n * 4);
    }
    fgi_status allgather_dev(fgi_graph* g, const void* src, void* dst, uint64_t bytes) override {
        FGI_TRY(stage(g, src, bytes));
        FGI_TRY(gather(g, bytes));
        return upload(g, dst, rbuf.data(), (uint64_t)ps(g)->v.world * bytes);
    }
    fgi_status alltoall_dev(fgi_graph* g, const void* src, void* dst, uint64_t bytes) override {
        const uint32_t W = ps(g)->v.world, R = ps(g)->v.rank;
        FGI_TRY(stage(g, src, (uint64_t)W * bytes));
        FGI_TRY(gather(g, (uint64_t)W * bytes));
        std::vector<uint8_t> in((size_t)W * bytes);
        for (uint32_t q = 0; q < W; ++q)
            std::memcpy(in.data() + (size_t)q * bytes, rbuf.data() + ((size_t)q * W + R) * bytes, bytes);
        return upload(g, dst, in.data(), (uint64_t)W * bytes);
    }
    // one all-gather of [max] padded bytes per rank: a world-th of what alltoallv would move
    fgi_status allgatherv(fgi_graph* g, const void* src, const uint64_t* bytes, void* dst) override {
        const uint32_t W = ps(g)->v.world, R = ps(g)->v.rank;
        uint64_t mx = 0;
        for (uint32_t q = 0; q < W; ++q) mx = std::max(mx, bytes[q]);
        FGI_HIP(g, hipStreamSynchronize(g->stream));
        if (!mx) return FGI_OK;
        sbuf.assign(mx, 0);
        FGI_TRY(stage(g, src, bytes[R]));
        FGI_TRY(gather(g, mx));
        uint64_t at = 0;
        for (uint32_t q = 0; q < W; ++q) {
            if (bytes[q])
                FGI_HIP(g, hipMemcpyAsync(static_cast<char*>(dst) + at, rbuf.data() + (size_t)q * mx, bytes[q],
                                          hipMemcpyHostToDevice, g->stream));
            at += bytes[q];
        }
        FGI_HIP(g, hipStreamSynchronize(g->stream));
        return FGI_OK;
    }
    // one all-gather of [world][max] padded bytes; the largest range of any pair first (one word per rank)
    // where the caller does not know it. Always waits.
    fgi_status alltoallv(fgi_graph* g, const void* src, const uint64_t* soff, const uint64_t* sbytes, void* dst,
                         const uint64_t* roff, const uint64_t* rbytes, uint64_t max_pair_bytes, bool,
                         const char* what) override {
        const uint32_t W = ps(g)->v.world, R = ps(g)->v.rank;
        uint64_t mx = max_pair_bytes;
        if (mx == kPairUnknown) {
            unsigned long long mine = 0;
            uint64_t all[8];
            for (uint32_t q = 0; q < W; ++q) mine = std::max<unsigned long long>(mine, sbytes[q]);
            FGI_TRY(gather_words(g, &mine, false, 1, all, what));
            mx = 0;
            for (uint32_t q = 0; q < W; ++q) mx = std::max(mx, all[q]);
        }
        FGI_HIP(g, hipStreamSynchronize(g->stream));
        if (!mx) return FGI_OK;
        sbuf.assign((size_t)W * mx, 0);
        for (uint32_t q = 0; q < W; ++q)
            if (sbytes[q])
                FGI_HIP(g, hipMemcpyAsync(sbuf.data() + (size_t)q * mx, static_cast<const char*>(src) + soff[q], sbytes[q],
                                          hipMemcpyDeviceToHost, g->stream));
        FGI_HIP(g, hipStreamSynchronize(g->stream));
        FGI_TRY(gather(g, (uint64_t)W * mx));
        for (uint32_t q = 0; q < W; ++q)
            if (rbytes[q])
                FGI_HIP(g, hipMemcpyAsync(static_cast<char*>(dst) + roff[q], rbuf.data() + ((size_t)q * W + R) * mx, rbytes[q],
                                          hipMemcpyHostToDevice, g->stream));
        FGI_HIP(g, hipStreamSynchronize(g->stream));
        return FGI_OK;
    }
};

// ---- in-process group (P graphs, one host thread per rank) ---------------------------------------
// The ranks meet at a generation barrier; a rank that fails marks the group failed and releases
// the others, whose collectives then return FGI_EDEVICE instead of waiting forever.
struct LocalGroup {
    std::vector<fgi_graph*> gs;
    std::mutex mu;
    std::condition_variable cv;
    uint32_t arrived = 0;
    uint64_t gen = 0;
    bool failed = false;
    std::vector<uint64_t> vals;   // [2][P][kPartRedMax] gather_words' contributions (LocalComm::meet)
    // device exchanges (LocalComm::exchange_dev): rank r records ready[r] when its source is final and
    // done[r] when its copies from the others are queued; the others' streams wait on them. xsrc, xoff:
    // rank r's source and its [P] byte offsets per destination
    std::vector<hipEvent_t> ready, done;
    std::vector<const char*> xsrc;
    std::vector<uint64_t> xoff;

    explicit LocalGroup(std::vector<fgi_graph*> g) : gs(std::move(g)) {
        xsrc.assign(gs.size(), nullptr);
        xoff.assign(gs.size() * gs.size(), 0);
        vals.assign(2 * gs.size() * kPartRedMax, 0);
        ready.assign(gs.size(), nullptr);
        done.assign(gs.size(), nullptr);
        for (size_t r = 0; r < gs.size(); ++r) {
            hipSetDevice(gs[r]->device);
            hipEventCreateWithFlags(&ready[r], hipEventDisableTiming);
            hipEventCreateWithFlags(&done[r], hipEventDisableTiming);
        }
    }
    ~LocalGroup() {
        for (hipEvent_t e : ready)
            if (e) hipEventDestroy(e);
        for (hipEvent_t e : done)
            if (e) hipEventDestroy(e);
    }
    bool arrive() {
        std::unique_lock<std::mutex> lk(mu);
        if (failed) return false;
        const uint64_t my = gen;
        if (++arrived == gs.size()) {
            arrived = 0;
            ++gen;
            cv.notify_all();
            return true;
        }
        cv.wait(lk, [&] { return gen != my || failed; });
        // a barrier every rank reached has completed, also for a rank that wakes after a peer left the call
        // with an error of its own behind that barrier (a refused shard: every rank returns FGI_EINVAL)
        return gen != my;
    }
    void fail() {
        std::lock_guard<std::mutex> lk(mu);
        failed = true;
        cv.notify_all();
    }
    void reset() {   // gen stays: LocalComm::meet takes its slots from it
        std::lock_guard<std::mutex> lk(mu);
        failed = false;
        arrived = 0;
    }
};

// Every collective is one of the two exchanges below; they alone meet the group's barrier. A rank that
// leaves one with an error of its own fails the group in its driver (local_run), which releases the rest.
struct LocalComm final : PartComm {
    std::shared_ptr<LocalGroup> grp;
    uint32_t rank;
    LocalComm(std::shared_ptr<LocalGroup> g, uint32_t r) : grp(std::move(g)), rank(r) {}

    fgi_status peer_failed(fgi_graph* g) { return set_err(g, FGI_EDEVICE, "another rank of the in-process group failed"); }

    // Host memory, synchronous: publish(slot) leaves this rank's data in its slot, read(slot) finds every
    // rank's there. One barrier: slot is the parity of the group's generation, the same on every rank
    // between two barriers, so the next exchange writes the other slot, and a rank comes to write this one
    // again only behind that exchange's barrier, which every rank reaches after its reads here.
    // This rests on two things. Every rank meets every barrier of the group, the same number of times and in
    // the same order (the collectives' contract; exchange_dev's two barriers leave the parity as it was, for
    // every rank alike). And LocalGroup::gen only ever counts completed barriers: reset() after a failed call
    // must leave it alone, since the ranks of a failed call may have left at different barriers and gen is
    // the one count they still share.
    template <class P, class R>
    fgi_status meet(fgi_graph* g, P publish, R read) {
        uint32_t slot = 0;
        {
            std::lock_guard<std::mutex> lk(grp->mu);
            slot = (uint32_t)(grp->gen & 1);
        }
        FGI_TRY(publish(slot));
        if (!grp->arrive()) return peer_failed(g);
        read(slot);
        return FGI_OK;
    }
    // Device memory: this rank publishes its source (and offsets into it, nullable); behind the first
    // barrier every source is final and `copies` runs; behind the second every rank's copies out of it are
    // done, so no source is overwritten early (and the host publishes its next source only then).
    // Stream-ordered, no host wait: the rank marks its source ready on its stream before the first barrier
    // (a host-thread barrier, no device synchronisation) and its copies done before the second; each stream
    // waits for the others' marks. host_waits: the host waits for its stream before each barrier instead,
    // and returns with the data in place.
    template <class F>
    fgi_status exchange_dev(fgi_graph* g, const void* src, const uint64_t* soff, bool host_waits, F copies) {
        const size_t W = grp->gs.size();
        grp->xsrc[rank] = static_cast<const char*>(src);
        for (size_t q = 0; q < W; ++q) grp->xoff[rank * W + q] = soff ? soff[q] : 0;
        // what this rank's stream holds so far is final for the others behind the barrier: the host has
        // waited for it, or it is marked and the others' streams wait for the mark
        auto settle = [&](std::vector<hipEvent_t>& marks) -> fgi_status {
            if (host_waits) {
                FGI_HIP(g, hipStreamSynchronize(g->stream));
                return grp->arrive() ? FGI_OK : peer_failed(g);
            }
            FGI_HIP(g, hipEventRecord(marks[rank], g->stream));
            if (!grp->arrive()) return peer_failed(g);
            for (size_t q = 0; q < W; ++q)
                if (q != rank) FGI_HIP(g, hipStreamWaitEvent(g->stream, marks[q], 0));
            return FGI_OK;
        };
        FGI_TRY(settle(grp->ready));   // every source is final
        FGI_TRY(copies());
        return settle(grp->done);      // every rank's copies out of this rank's source are done
    }

    fgi_status gather_words(fgi_graph* g, const unsigned long long* src, bool src_dev, uint32_t words, uint64_t* all,
                            const char*) override {
        const size_t W = grp->gs.size();
        if (src_dev) {
#if FGI_SPIN_WAIT
            FGI_TRY(publish_wait(g, g->stream, src, words, g->red_pub));
            src = g->red_pub;
#else
            unsigned long long* host = words > 4 ? ps(g)->red_host : ps(g)->scalar_host;
            FGI_HIP(g, hipMemcpyAsync(host, src, 8 * words, hipMemcpyDeviceToHost, g->stream));
            FGI_HIP(g, hipStreamSynchronize(g->stream));
            src = host;
#endif
        }
        return meet(
            g,
            [&](uint32_t slot) -> fgi_status {
                for (uint32_t i = 0; i < words; ++i) grp->vals[(slot * W + rank) * kPartRedMax + i] = src[i];
                return FGI_OK;
            },
            [&](uint32_t slot) {
                for (size_t q = 0; q < W; ++q)
                    for (uint32_t i = 0; i < words; ++i) all[q * words + i] = grp->vals[(slot * W + q) * kPartRedMax + i];
            });
    }
    // host-side sum: every rank copies its array out, adds up everyone's and copies the sum in
    fgi_status allreduce_u32(fgi_graph* g, uint32_t* dev, uint64_t n) override {
        std::vector<uint32_t> sum(n, 0);
        FGI_TRY(meet(
            g,
            [&](uint32_t slot) -> fgi_status {
                std::vector<uint32_t>& h = ps(g)->u32_host[slot];
                h.resize(n);
                if (n) FGI_HIP(g, hipMemcpyAsync(h.data(), dev, n * 4, hipMemcpyDeviceToHost, g->stream));
                FGI_HIP(g, hipStreamSynchronize(g->stream));
                return FGI_OK;
            },
            [&](uint32_t slot) {
                for (size_t q = 0; q < grp->gs.size(); ++q) {
                    const std::vector<uint32_t>& h = ps(grp->gs[q])->u32_host[slot];
                    for (uint64_t i = 0; i < n; ++i) sum[i] += h[i];
                }
            }));
        if (n) FGI_HIP(g, hipMemcpyAsync(dev, sum.data(), n * 4, hipMemcpyHostToDevice, g->stream));
        FGI_HIP(g, hipStreamSynchronize(g->stream));
        return FGI_OK;
    }
    fgi_status allgather_dev(fgi_graph* g, const void* src, void* dst, uint64_t bytes) override {
        return exchange_dev(g, src, nullptr, false, [&]() -> fgi_status {
            for (size_t q = 0; q < grp->gs.size(); ++q)
                FGI_HIP(g, hipMemcpyAsync(static_cast<char*>(dst) + q * bytes, grp->xsrc[q], bytes, hipMemcpyDefault, g->stream));
            return FGI_OK;
        });
    }
    fgi_status alltoall_dev(fgi_graph* g, const void* src, void* dst, uint64_t bytes) override {
        return exchange_dev(g, src, nullptr, false, [&]() -> fgi_status {
            for (size_t q = 0; q < grp->gs.size(); ++q)
                FGI_HIP(g, hipMemcpyAsync(static_cast<char*>(dst) + q * bytes, grp->xsrc[q] + rank * bytes, bytes,
                                          hipMemcpyDefault, g->stream));
            return FGI_OK;
        });
    }
    fgi_status alltoallv(fgi_graph* g, const void* src, const uint64_t* soff, const uint64_t*, void* dst, const uint64_t* roff,
                         const uint64_t* rbytes, uint64_t, bool, const char*) override {
        // Always the host-waiting form: its callers' hosts have just waited for the counts, and at 8 ranks the
        // marks' 2 x 7 stream waits per rank cost a host-driven level more than the two short waits do
        // (profiles/part_transport_ab.txt).
        const size_t W = grp->gs.size();
        return exchange_dev(g, src, soff, true, [&]() -> fgi_status {
            for (size_t q = 0; q < W; ++q)
                if (rbytes[q])
                    FGI_HIP(g, hipMemcpyAsync(static_cast<char*>(dst) + roff[q], grp->xsrc[q] + grp->xoff[q * W + rank],
                                              rbytes[q], hipMemcpyDefault, g->stream));
            return FGI_OK;
        });
    }
};

// ---- the protocols, once, above the transport -----------------------------------------------------
// This level's forwarded targets: send_buf[q] (send_cnt[q] entries) to owner q; the targets received from
// every other rank are concatenated at recv_buf (stream-ordered: the level's apply kernel reads them).
// send_cnt[world, world + 1] carry the rank's local {F, T} of the next level, summed with the targets
// sent by all ranks into glob = {sum F, sum T, sum sent} on the way: the count all-gather doubles as the
// level's all-reduce, so a push level waits for the host once (the gather).
fgi_status part_exchange(fgi_graph* g, uint64_t* n_recv, uint64_t* n_sent, uint64_t* glob) {
    PartState* p = ps(g);
    const uint32_t W = p->v.world, R = p->v.rank, S = W + 2;
    uint64_t c[8 * 10];   // c[q * S + r]: sent by q to r; c[q * S + W + i]: q's F, T
    FGI_TRY(p->ops->gather_words(g, p->v.send_cnt, true, S, c, "all-gather of the push level's counts"));
    sum_counts(c, W, glob);
    uint64_t soff[8], sb[8], roff[8], rb[8], recv = 0, sent = 0, mx = 0;
    for (uint32_t q = 0; q < W; ++q) {
        soff[q] = (uint64_t)q * p->v.block * 4;
        sb[q] = q == R ? 0 : c[(size_t)R * S + q] * 4;
        roff[q] = recv * 4;
        rb[q] = q == R ? 0 : c[(size_t)q * S + R] * 4;
        recv += rb[q] / 4;
        sent += sb[q] / 4;
        for (uint32_t r = 0; r < W; ++r)
            if (r != q) mx = std::max(mx, c[(size_t)q * S + r] * 4);
    }
    FGI_TRY(p->ops->alltoallv(g, p->v.send_buf, soff, sb, p->v.recv_buf, roff, rb, mx, false,
                              "exchange of a push level's targets"));
    *n_recv = recv;
    *n_sent = sent;
    return FGI_OK;
}

// every rank's local invalidated-bitmap words inv_bm[0, block/32) into front_global, stream-ordered
// (the planned waves' frontier exchange; part_allgather_front's full mode)
fgi_status part_allgather_front_full(fgi_graph* g) {
    PartState* p = ps(g);
    ++p->front_full;
    p->front_bytes += (uint64_t)(p->v.world - 1) * p->v.block / 8;
    return p->ops->allgather_dev(g, g->inv_bm, p->v.front_global, (uint64_t)(p->v.block / 32) * 4);
}

// a2a_send[q * C, + C) to rank q, into a2a_recv[r * C, + C) from every rank r (stream-ordered)
fgi_status part_alltoall_async(fgi_graph* g) {
    PartState* p = ps(g);
    return p->ops->alltoall_dev(g, p->a2a_send, p->a2a_recv, (uint64_t)p->a2a_C * 4);
}

fgi_status part_allreduce_u32(fgi_graph* g, uint32_t* dev, uint64_t n) { return ps(g)->ops->allreduce_u32(g, dev, n); }

// every rank's current-node bits (its owned slots: W64 = ceil(block / 64) words each, rank q's at
// q * W64) into the returned all-gathered array; the caller builds cur_local first (its W64 words)
fgi_status part_cur_buffers(fgi_graph* g, unsigned long long** local, unsigned long long** all, uint64_t* w64) {
    PartState* p = ps(g);
    if (!p->cur_local) {
        p->cur_w64 = ((uint64_t)p->v.block + 63) / 64;
        if (hipMalloc(&p->cur_local, p->cur_w64 * 8) != hipSuccess ||
            hipMalloc(&p->cur_all, p->cur_w64 * 8 * p->v.world) != hipSuccess)
            return set_err(g, FGI_ENOMEM, "current-node bitmaps");
    }
    *local = p->cur_local;
    *all = p->cur_all;
    *w64 = p->cur_w64;
    return FGI_OK;
}

fgi_status part_allgather_cur(fgi_graph* g) {
    PartState* p = ps(g);
    return p->ops->allgather_dev(g, p->cur_local, p->cur_all, p->cur_w64 * 8);
}

// the sharded loads' collectives (shard.hip)
fgi_status part_allgather_words(fgi_graph* g, const uint64_t* mine, uint32_t words, uint64_t* all) {
    if (words < 1 || words > kShardWords) return set_err(g, FGI_EINVAL, "part_allgather_words: %u words", words);
    return ps(g)->ops->gather_words(g, reinterpret_cast<const unsigned long long*>(mine), false, words, all,
                                    "all-gather of a sharded load's counts");
}
fgi_status part_allgatherv(fgi_graph* g, const void* src, const uint64_t* bytes, void* dst) {
    return ps(g)->ops->allgatherv(g, src, bytes, dst);
}
fgi_status part_alltoallv(fgi_graph* g, const void* src, const uint64_t* soff, const uint64_t* sbytes, void* dst,
                          const uint64_t* roff, const uint64_t* rbytes) {
    return ps(g)->ops->alltoallv(g, src, soff, sbytes, dst, roff, rbytes, kPairUnknown, true,
                                 "variable-size exchange of a sharded load");
}
uint32_t* part_weight(fgi_graph* g) { return ps(g)->weight; }

static fgi_status part_store_in(fgi_graph* g, const uint64_t* keys, const uint64_t* tags, uint64_t m);

// device entries (dependant local << 32 | used global, tag) appended to the in-store
fgi_status part_store_in_dev(fgi_graph* g, const uint64_t* keys, const uint64_t* tags, uint64_t m) {
    return part_store_in(g, keys, tags, m);
}

namespace {
// entries (dependant local << 32 | used global) whose used end is in the sorted list: tag 0 (a
// version is never 0, so the list build reads them as dead)
__global__ void k_in_kill(uint64_t m, const uint64_t* __restrict__ keys, uint64_t* tags, const uint32_t* __restrict__ list,
                          uint32_t nl) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t u = (uint32_t)keys[i];
    uint32_t lo = 0, hi = nl;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (list[mid] < u) lo = mid + 1;
        else hi = mid;
    }
    if (lo < nl && list[lo] == u) tags[i] = 0;
}
}  // namespace

fgi_status part_kill_used(fgi_graph* g, std::vector<uint32_t> slots) {
    PartState* p = ps(g);
    if (slots.empty() || p->in_n == 0) return FGI_OK;
    std::sort(slots.begin(), slots.end());
    slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    Tmp td;
    uint32_t* d;
    FGI_TRY(tmalloc(g, td, &d, slots.size()));
    FGI_HIP(g, hipMemcpyAsync(d, slots.data(), slots.size() * 4, hipMemcpyHostToDevice, g->stream));
    hipLaunchKernelGGL(k_in_kill, dim3((uint32_t)((p->in_n + 255) / 256)), dim3(256), 0, g->stream, p->in_n, p->in_keys, p->in_tags, d,
                       (uint32_t)slots.size());
    FGI_HIP(g, hipStreamSynchronize(g->stream));
    return FGI_OK;
}

fgi_status part_set_bucket(fgi_graph* g, int64_t words) {
    PartState* p = ps(g);
    if (!p) return set_err(g, FGI_ESTATE, "partition not initialised");
    if (words < 0) return set_err(g, FGI_EINVAL, "bucket words must be >= 0");
    p->a2a_C = words == 0 ? p->a2a_cap : (uint32_t)std::max<int64_t>(2, std::min<int64_t>(words, p->a2a_cap));
    return FGI_OK;
}

PartBuckets part_buckets(fgi_graph* g) {
    PartState* p = ps(g);
    return PartBuckets{p->a2a_C, p->a2a_send, p->a2a_recv, p->a2a_cur, p->red};
}

namespace {
// this rank's bitmap words that changed since the last exchange (front_global holds what the other
// ranks last received): listed as (global word << 32 | word) and written into front_global's own range
__global__ void k_front_delta(uint32_t words, const uint32_t* __restrict__ inv, uint32_t* own_front, uint32_t word_base,
                              uint64_t* dbuf, unsigned long long* dcnt) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t v = w < words ? inv[w] : 0u;
    const bool ch = w < words && v != own_front[w];
    const unsigned long long m = __ballot(ch);
    if (!m) return;
    const uint32_t lane = threadIdx.x & 63;
    unsigned long long b = 0;
    if (lane == 0) b = atomicAdd(dcnt, (unsigned long long)__popcll(m));
    b = __shfl(b, 0, 64);
    if (ch) {
        dbuf[b + __popcll(m & ((1ull << lane) - 1ull))] = ((uint64_t)(word_base + w) << 32) | v;
        own_front[w] = v;
    }
}

__global__ void k_front_apply(uint64_t n, const uint64_t* __restrict__ rbuf, uint32_t* front) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint64_t e = rbuf[i];
        front[e >> 32] = (uint32_t)e;
    }
}
}  // namespace

// The invalidated bitmap over all ranks' slots before a pull level (front_global). Full mode: an
// all-gather of every rank's block/32 words — (world - 1) * block / 8 bytes into every rank. Delta mode:
// each rank lists the words that gained bits since the previous exchange of the wave (8 B each) and
// sends the list to every other rank; the receivers patch their copy. FGI_OPT_FRONT_EXCHANGE 0 picks
// per level whichever moves fewer bytes (every rank decides alike from the all-gathered list sizes),
// 1 always full, 2 always delta. Either way front_global ends up identical.
fgi_status part_allgather_front(fgi_graph* g) {
    PartState* p = ps(g);
    const int mode = g->opt_front_exchange;
    if (mode == 1) return part_allgather_front_full(g);
    hipStream_t s = g->stream;
    const uint32_t words = p->v.block / 32, W = p->v.world, R = p->v.rank;
    FGI_HIP(g, hipMemsetAsync(p->dcnt, 0, 8, s));
    hipLaunchKernelGGL(k_front_delta, dim3((words + 255) / 256), dim3(256), 0, s, words, g->inv_bm,
                       p->v.front_global + (uint64_t)p->v.rank * words, p->v.rank * words, p->dbuf, p->dcnt);
    FGI_HIP(g, hipGetLastError());
    unsigned long long mine = 0;
    FGI_HIP(g, hipMemcpyAsync(&mine, p->dcnt, 8, hipMemcpyDeviceToHost, s));
    FGI_HIP(g, hipStreamSynchronize(s));
    uint64_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    FGI_TRY(p->ops->gather_words(g, &mine, false, 1, cnt, "all-gather of a count"));
    uint64_t total = 0;
    for (uint32_t q = 0; q < W; ++q) total += cnt[q];
    const uint64_t full_bytes = (uint64_t)(W - 1) * words * 4;
    if (mode == 0 && 8 * total >= full_bytes) {   // dense: the plain all-gather moves fewer bytes
        ++p->front_full;
        p->front_bytes += full_bytes;
        return p->ops->allgather_dev(g, g->inv_bm, p->v.front_global, (uint64_t)words * 4);
    }
    ++p->front_delta;
    // every rank's list dbuf[0, cnt[rank]) to every other rank, concatenated at rbuf (self skipped)
    uint64_t soff[8], sb[8], roff[8], rb[8], n_recv = 0, mx = 0;
    for (uint32_t q = 0; q < W; ++q) {
        soff[q] = 0;
        sb[q] = q == R ? 0 : cnt[R] * 8;
        roff[q] = n_recv * 8;
        rb[q] = q == R ? 0 : cnt[q] * 8;
        n_recv += rb[q] / 8;
        if (W > 1) mx = std::max(mx, cnt[q] * 8);
    }
    FGI_TRY(p->ops->alltoallv(g, p->dbuf, soff, sb, p->rbuf, roff, rb, mx, false, "exchange of the frontier's delta lists"));
    p->front_bytes += 8 * n_recv;
    if (n_recv)
        hipLaunchKernelGGL(k_front_apply, dim3((uint32_t)((n_recv + 255) / 256)), dim3(256), 0, s, n_recv, p->rbuf,
                           p->v.front_global);
    FGI_HIP(g, hipGetLastError());
    return FGI_OK;
}

// a wave's first exchange is relative to an empty bitmap (every rank's inv_bm starts cleared)
fgi_status part_front_reset(fgi_graph* g) {
    PartState* p = ps(g);
    if (g->opt_front_exchange == 1) return FGI_OK;   // every exchange overwrites the whole bitmap
    FGI_HIP(g, hipMemsetAsync(p->v.front_global, 0, p->v.front_words_global * 4, g->stream));
    return FGI_OK;
}

fgi_status part_front_stats(fgi_graph* g, uint64_t* full, uint64_t* delta, uint64_t* bytes) {
    PartState* p = ps(g);
    if (!p) return FGI_EINVAL;
    *full = p->front_full;
    *delta = p->front_delta;
    *bytes = p->front_bytes;
    return FGI_OK;
}

fgi_status part_allreduce_sum(fgi_graph* g, const unsigned long long* dev_val, uint64_t* out, uint32_t count) {
    if (count < 1 || count > kPartRedMax) return set_err(g, FGI_EINVAL, "part_allreduce_sum: count %u", count);
    return ps(g)->ops->allreduce_sum(g, dev_val, out, count);
}

namespace {

// versions by slot; with partition codes (ig: code -> slot) entry c holds the version of slot ig[c]
__global__ void k_versions_all(uint32_t n, uint64_t seed, uint64_t* ver, const uint32_t* __restrict__ ig) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ver[i] = synth_version(seed, ig ? ig[i] : (uint32_t)i);
}

__global__ void k_versions_local(uint32_t n, uint32_t base, uint64_t seed, unsigned long long* node,
                                 const uint32_t* __restrict__ ig) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) node[i] = synth_version(seed, ig ? ig[base + i] : base + i) | kW_Consistent;
}

// Row-range R-MAT (fgi_part_synth_rmat): edge i is a pure function of i, so every rank walks the
// global edge sequence and keeps only its share — the rows of the slots it owns (used == src) and the
// dependency-list entries of the slots it owns (dependant == dst, not stale) — without materialising
// the global edge list (at configs[2] that is 1.07G edges, 8.6 GB of keys per rank). Block b walks the
// contiguous edges [b * per, (b + 1) * per). Pass 0 counts both shares per block and adds every live
// edge to its dependant's weight (the list order: a slot's live dependencies over the whole graph);
// pass 1 writes the shares at the blocks' exclusive offsets (wave ballots, LDS cursors).
constexpr uint32_t kGenBlocks = 4096;
// With partition codes (gc: slot -> code, fill pass only) the kept keys hold codes, and each row entry's tag
// (computed from the slot ids, as build_rows_from_keys would: the dependant's version, + 1 if stale) goes to
// rtags. A slot's code has the slot's owner, so the shares and counts are those of the slot ids.
__global__ __launch_bounds__(256) void k_rmat_part(uint64_t m, uint64_t per, uint32_t scale, uint64_t seed, uint32_t base,
                                                   uint32_t n_local, uint32_t stale_pct, uint64_t stale_seed, int fill,
                                                   unsigned long long* blk_cnt, const unsigned long long* blk_off,
                                                   uint64_t* rows, uint64_t* ins, uint32_t* weight,
                                                   const uint32_t* __restrict__ gc, uint64_t* rtags) {
    __shared__ unsigned long long s_cur[2];
    __shared__ unsigned long long s_red[2][4];
    const uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per < m ? lo + per : m;
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (fill && threadIdx.x < 2) s_cur[threadIdx.x] = blk_off[threadIdx.x * kGenBlocks + blockIdx.x];
    __syncthreads();
    unsigned long long nr = 0, ni = 0;
    for (uint64_t i0 = lo; i0 < hi; i0 += blockDim.x) {   // block-uniform
        const uint64_t i = i0 + threadIdx.x;
        bool own_row = false, own_in = false;
        uint32_t s = 0, d = 0;
        if (i < hi) {
            rmat_edge(i, scale, seed, &s, &d);
            own_row = s - base < n_local;
            const bool live = !synth_stale(stale_pct, stale_seed, s, d);
            own_in = live && d - base < n_local;
            if (!fill && live) atomicAdd(weight + d, 1u);
        }
        if (!fill) {
            nr += own_row;
            ni += own_in;
            continue;
        }
        const unsigned long long mr = __ballot(own_row), mi = __ballot(own_in);
        unsigned long long br = 0, bi = 0;
        if (lane == 0) {
            if (mr) br = atomicAdd(&s_cur[0], (unsigned long long)__popcll(mr));
            if (mi) bi = atomicAdd(&s_cur[1], (unsigned long long)__popcll(mi));
        }
        br = __shfl(br, 0, 64);
        bi = __shfl(bi, 0, 64);
        const unsigned long long lt = (1ull << lane) - 1ull;
        uint32_t sc = s, dc = d;
        if (gc && (own_row || own_in)) {
            sc = gc[s];
            dc = gc[d];
        }
        if (own_row) {
            const uint64_t at = br + __popcll(mr & lt);
            rows[at] = ((uint64_t)(sc - base) << 32) | dc;
            if (rtags) rtags[at] = synth_version(seed, d) + (synth_stale(stale_pct, stale_seed, s, d) ? 1u : 0u);
        }
        if (own_in) ins[bi + __popcll(mi & lt)] = ((uint64_t)(dc - base) << 32) | sc;
    }
    if (fill) return;
    for (int dd = 32; dd >= 1; dd >>= 1) {
        nr += __shfl_xor(nr, dd, 64);
        ni += __shfl_xor(ni, dd, 64);
    }
    if (lane == 0) {
        s_red[0][wid] = nr;
        s_red[1][wid] = ni;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long t = 0;
        for (uint32_t q = 0; q < blockDim.x / 64; ++q) t += s_red[threadIdx.x][q];
        blk_cnt[threadIdx.x * kGenBlocks + blockIdx.x] = t;
    }
}

__global__ void k_in_tags_synth(uint64_t m, const uint64_t* __restrict__ keys, uint32_t base, uint64_t seed,
                                uint64_t* tags, const uint32_t* __restrict__ ig) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    const uint32_t c = (uint32_t)(keys[e] >> 32) + base;   // the dependant (its code, with partition codes)
    tags[e] = synth_version(seed, ig ? ig[c] : c);
}

// the in-store's live entries (tag == version of the dependant's node): flag for the compaction
__global__ void k_in_live(uint64_t m, const uint64_t* __restrict__ keys, const uint64_t* __restrict__ tags,
                          const unsigned long long* __restrict__ node, uint32_t* flag) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    const uint64_t t = tags[e];
    flag[e] = (t != 0 && (node[(uint32_t)(keys[e] >> 32)] & kVMask) == t) ? 1u : 0u;
}

__global__ void k_compact64(uint64_t m, const uint64_t* __restrict__ in, const uint32_t* __restrict__ flag,
                            const uint32_t* __restrict__ pos, uint64_t* out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < m && flag[e]) out[pos[e]] = in[e];
}

__global__ void k_in_part_unique(uint64_t m, const uint64_t* __restrict__ k, uint32_t* keep) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < m) keep[e] = (e == 0 || k[e] != k[e - 1]) ? 1u : 0u;
}

__global__ void k_in_part_rows(uint64_t m, const uint64_t* __restrict__ k, const uint32_t* __restrict__ keep,
                               const uint32_t* __restrict__ pos, uint32_t* src_out, uint64_t* off, uint32_t* len) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    const uint32_t d = (uint32_t)(k[e] >> 32);
    if (keep[e]) src_out[pos[e]] = (uint32_t)k[e];
    if (e == 0 || (uint32_t)(k[e - 1] >> 32) != d) off[d] = pos[e];
    if (e + 1 == m || (uint32_t)(k[e + 1] >> 32) != d) len[d] = pos[e] + keep[e];   // row end, fixed below
}

__global__ void k_in_part_fix(uint32_t n, const uint64_t* __restrict__ off, uint32_t* len) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d < n && len[d]) len[d] -= (uint32_t)off[d];
}

// fgi_part_register_nodes: every listed slot's version goes into the replica; the owner installs the
// node (as fgi_register_nodes: the slot must be empty)
__global__ void k_part_register(uint32_t n, const uint32_t* __restrict__ slot, const uint64_t* __restrict__ version,
                                const uint32_t* __restrict__ flags, uint32_t base, uint32_t n_local, uint64_t* ver_all,
                                unsigned long long* node, uint32_t* row_len, unsigned long long* err) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slot[i];
    const uint64_t v = version[i];
    ver_all[s] = v;
    const uint32_t h = s - base;
    if (h >= n_local) return;
    if (word_is_current(node[h])) {
        atomicAdd(err, 1ull);
        return;
    }
    node[h] = v ? flags_to_word(v, flags ? flags[i] : FGI_CONSISTENT) : 0ull;
    row_len[h] = 0;
}

// fgi_part_load_edges: every edge of the batch that is live when loaded adds to its dependant's weight
__global__ void k_part_weight(uint64_t m, const uint32_t* __restrict__ dep, const uint64_t* __restrict__ tag,
                              const uint64_t* __restrict__ ver_all, uint32_t* weight) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < m && tag[e] == ver_all[dep[e]]) atomicAdd(weight + dep[e], 1u);
}

inline uint32_t nblk(uint64_t n) { return (uint32_t)((n + 255) / 256); }

// ---- partition codes ------------------------------------------------------------------
// The code order: each rank's range sorted by weight class (8 classes per octave of weight + 1, the
// heaviest first, as the single device's labels), ties in slot order. A slot's code comes from its position
// in that order (pc_code), inside its owner's range ([q * block, q * block + n_local)), so a slot keeps its
// owner and every rank computes the same tables from the same global weights.
__device__ __forceinline__ uint32_t pc_class(uint32_t w) {
    const uint32_t x = w + 1u;
    const uint32_t l = 31u - (uint32_t)__builtin_clz(x);
    const uint32_t frac = l >= 3 ? (x >> (l - 3)) & 7u : (x << (3 - l)) & 7u;
    return l * kClassPerOctave + frac;
}
__global__ void k_pc_keys(uint32_t N, uint32_t B, const uint32_t* __restrict__ w, uint64_t* keys) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= N) return;
    keys[x] = ((uint64_t)(x / B) << 48) | ((uint64_t)(kLabelClasses - 1u - pc_class(w[x])) << 32) | x;
}
// Position i of that order (rank q's range [q * B, q * B + n_q)) -> its code. Contiguous (T = 0), the heaviest
// slots of a rank would all fall to its first pull blocks (a pull block owns a fixed run of T slots); so the
// order is dealt round-robin over the runs of T slots instead: run j gets positions j, j + S, j + 2S, ... (S
// runs, the last one short; once the short run is full the rest are dealt over the S - 1 full runs), and
// every pull block starts with its share of the hubs, in weight order.
__device__ __forceinline__ uint32_t pc_code(uint32_t i, uint32_t N, uint32_t B, uint32_t T) {
    const uint32_t q = i / B, base = q * B, nq = min(B, N - base), r = i - base;
    if (T == 0 || nq <= T) return i;
    const uint32_t S = (nq + T - 1) / T, last = nq - (S - 1) * T, A = last * S;
    uint32_t run, k;
    if (r < A) {
        run = r % S;
        k = r / S;
    } else {
        run = (r - A) % (S - 1);
        k = last + (r - A) / (S - 1);
    }
    return base + run * T + k;
}
__global__ void k_pc_tables(uint32_t N, uint32_t B, uint32_t T, const uint64_t* __restrict__ sorted, uint32_t* gc,
                            uint32_t* ig) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint32_t x = (uint32_t)sorted[i];
    const uint32_t c = pc_code(i, N, B, T);
    gc[x] = c;
    ig[c] = x;
}
// what was installed before the codes (registered nodes, versions, weights), moved to the codes
__global__ void k_pc_move_local(uint32_t nl, uint32_t base, const uint32_t* __restrict__ gc,
                                const unsigned long long* __restrict__ node_old, unsigned long long* node,
                                const uint32_t* __restrict__ used_old, uint32_t* used) {
    const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= nl) return;
    const uint32_t c = gc[base + h] - base;
    node[c] = node_old[h];
    used[c] = used_old[h];
}
__global__ void k_pc_move_global(uint32_t N, const uint32_t* __restrict__ gc, const uint64_t* __restrict__ ver_old,
                                 uint64_t* ver, const uint32_t* __restrict__ w_old, uint32_t* w) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= N) return;
    const uint32_t c = gc[x];
    if (ver) ver[c] = ver_old[x];   // null: the weights only
    w[c] = w_old[x];
}
// local handles <-> local code indices (owned range only), in place
__global__ void k_pc_local(uint64_t n, uint32_t* a, const uint32_t* __restrict__ table, uint32_t base, uint32_t nl) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t h = a[i];
        if (h < nl) a[i] = table[base + h] - base;
    }
}
// global slots -> codes, in place
__global__ void k_pc_global(uint64_t n, uint32_t* a, const uint32_t* __restrict__ gc, uint32_t N) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t x = a[i];
        if (x < N) a[i] = gc[x];
    }
}

// exclusive scan of flag[0, m) into pos; returns the total (synchronises the stream)
fgi_status scan_flags(fgi_graph* g, const uint32_t* flag, uint32_t* pos, uint64_t m, uint64_t* total) {
    hipStream_t s = g->stream;
    size_t tb = 0;
    FGI_HIP(g, rocprim::exclusive_scan(nullptr, tb, flag, pos, 0u, (size_t)m, rocprim::plus<uint32_t>(), s));
    Tmp tt;
    char* tmp;
    FGI_TRY(tmalloc(g, tt, &tmp, tb));
    FGI_HIP(g, rocprim::exclusive_scan(tmp, tb, flag, pos, 0u, (size_t)m, rocprim::plus<uint32_t>(), s));
    uint32_t lp = 0, lf = 0;
    hipError_t e = hipMemcpyAsync(&lp, pos + m - 1, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&lf, flag + m - 1, 4, hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);   // also when a copy failed: the other may be writing lp
    FGI_HIP(g, e);
    FGI_HIP(g, es);
    *total = (uint64_t)lp + lf;
    return FGI_OK;
}

}  // namespace

// The owned slots' dependency lists (pull levels) from the in-store: its live entries (tag == the
// owned dependant node's version: the reference's d._used, Computed.cs:365-366) sorted and
// deduplicated into lists of global used ids, each ordered by the entries' weights (as the single
// engine: most-depended-on first), then the heads and the pull candidates. Local to the rank.
// Choose the codes from every slot's weight (weight_dev: [n_global], by slot; replaced by the weights in
// code order) and move what is already installed: the owned node words and |_used| counts, the version
// replica. Only before any row or dependency entry exists and while no detached handle is taken.
fgi_status part_codes_choose(fgi_graph* g, uint32_t* weight_dev) {
    PartState* p = ps(g);
    const uint32_t N = p->v.n_global, B = p->v.block, base = p->v.base, nl = p->v.n_local;
    hipStream_t s = g->stream;
    FGI_TRY(fold(g));
    if (!g->pg_gc) FGI_TRY(dmalloc(g, &g->pg_gc, N));
    if (!g->pg_ig) FGI_TRY(dmalloc(g, &g->pg_ig, N));
    Tmp tk0, tk1, tt, tv, tw, tn, tu;
    uint64_t *k0, *k1, *ver_old;
    uint32_t *w_old, *used_old;
    unsigned long long* node_old;
    char* tmp;
    FGI_TRY(tmalloc(g, tk0, &k0, N));
    FGI_TRY(tmalloc(g, tk1, &k1, N));
    hipLaunchKernelGGL(k_pc_keys, dim3(nblk(N)), dim3(256), 0, s, N, B, weight_dev, k0);
    size_t tb = 0;
    FGI_HIP(g, rocprim::radix_sort_keys(nullptr, tb, k0, k1, (size_t)N, 0, 56, s));
    FGI_TRY(tmalloc(g, tt, &tmp, tb));
    FGI_HIP(g, rocprim::radix_sort_keys(tmp, tb, k0, k1, (size_t)N, 0, 56, s));
    uint32_t pgrid = 0, ptpb = 0;
    pull_geometry(g, &pgrid, &ptpb);
    const uint32_t T = pgrid ? ptpb * kPullTile : 0u;   // the slots a pull block owns
    hipLaunchKernelGGL(k_pc_tables, dim3(nblk(N)), dim3(256), 0, s, N, B, T, k1, g->pg_gc, g->pg_ig);
    FGI_TRY(tmalloc(g, tv, &ver_old, N));
    FGI_TRY(tmalloc(g, tw, &w_old, N));
    FGI_TRY(tmalloc(g, tn, &node_old, nl));
    FGI_TRY(tmalloc(g, tu, &used_old, nl));
    FGI_HIP(g, hipMemcpyAsync(ver_old, p->v.ver_all, (size_t)N * 8, hipMemcpyDeviceToDevice, s));
    FGI_HIP(g, hipMemcpyAsync(w_old, weight_dev, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
    if (nl) {
        FGI_HIP(g, hipMemcpyAsync(node_old, g->node, (size_t)nl * 8, hipMemcpyDeviceToDevice, s));
        FGI_HIP(g, hipMemcpyAsync(used_old, g->used_cnt, (size_t)nl * 4, hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(k_pc_move_global, dim3(nblk(N)), dim3(256), 0, s, N, g->pg_gc, ver_old, p->v.ver_all, w_old,
                       weight_dev);
    if (nl)
        hipLaunchKernelGGL(k_pc_move_local, dim3(nblk(nl)), dim3(256), 0, s, nl, base, g->pg_gc, node_old,
                           reinterpret_cast<unsigned long long*>(g->node), used_old, g->used_cnt);
    g->pg_gc_h.resize(N);
    g->pg_ig_h.resize(N);
    FGI_HIP(g, hipMemcpyAsync(g->pg_gc_h.data(), g->pg_gc, (size_t)N * 4, hipMemcpyDeviceToHost, s));
    FGI_HIP(g, hipMemcpyAsync(g->pg_ig_h.data(), g->pg_ig, (size_t)N * 4, hipMemcpyDeviceToHost, s));
    FGI_HIP(g, hipStreamSynchronize(s));
    // the table's fingerprint: the wave's first all-reduce checks that every rank chose the same codes (each
    // rank chooses them alone, from the same arrays; a rank given other arrays would number slots otherwise)
    uint64_t hsh = 0xcbf29ce484222325ull;
    for (uint32_t x = 0; x < N; ++x) hsh = (hsh ^ g->pg_gc_h[x]) * 0x100000001b3ull;
    g->pg_hash = hsh ? hsh : 1;
    g->lbl_perm = true;
    touch(g);
    note_words(g);
    if (getenv("FGI_TRACE")) fprintf(stderr, "[fgi] partition codes: rank %u of %u, %u slots\n", p->v.rank, p->v.world, N);
    return FGI_OK;   // the installed words moved: the callers rebuild the state view once their load is in
}

// the first bulk load of a partition that wants codes (nothing loaded, no detached handle taken)
bool part_codes_now(fgi_graph* g) {
    PartState* p = ps(g);
    return !g->lbl_perm && part_codes_wanted(g, p->v.n_global) && g->pool_top == 0 && p->in_n == 0 &&
           g->free_detached.size() == g->n_detached;
}

fgi_status part_rebuild_lists(fgi_graph* g) {
    PartState* p = ps(g);
    hipStream_t s = g->stream;
    const uint64_t m = p->in_n;
    g->uin_epoch = 0;
    if (p->v.block % 32 != 0) return FGI_OK;   // pull levels all-gather whole bitmap words per rank
    FGI_HIP(g, hipMemsetAsync(g->uin_len, 0, (size_t)g->n_slots * 4, s));
    FGI_HIP(g, hipMemsetAsync(g->uin_off, 0, (size_t)g->n_slots * 8, s));
    if (!g->uin_src) FGI_TRY(grow(g, &g->uin_src, &g->uin_cap, 1024, "the dependency lists"));
    Tmp tf, tp;
    uint32_t *flag = nullptr, *pos = nullptr;
    uint64_t mi = 0;
    if (m) {
        FGI_TRY(tmalloc(g, tf, &flag, m));
        FGI_TRY(tmalloc(g, tp, &pos, m));
        hipLaunchKernelGGL(k_in_live, dim3(nblk(m)), dim3(256), 0, s, m, p->in_keys, p->in_tags,
                           reinterpret_cast<const unsigned long long*>(g->node), flag);
        FGI_TRY(scan_flags(g, flag, pos, m, &mi));
    }
    if (mi) {
        Tmp tk1, tk2, tkeep, tkpos, tst;
        uint64_t *k1, *k2;
        uint32_t *keep, *kpos;
        char* st;
        FGI_TRY(tmalloc(g, tk1, &k1, mi));
        FGI_TRY(tmalloc(g, tk2, &k2, mi));
        FGI_TRY(tmalloc(g, tkeep, &keep, mi));
        FGI_TRY(tmalloc(g, tkpos, &kpos, mi));
        hipLaunchKernelGGL(k_compact64, dim3(nblk(m)), dim3(256), 0, s, m, p->in_keys, flag, pos, k1);
        tf.reset();   // before the sort's buffers
        tp.reset();
        size_t sb = 0;
        FGI_HIP(g, rocprim::radix_sort_keys(nullptr, sb, k1, k2, (size_t)mi, 0, 64, s));
        FGI_TRY(tmalloc(g, tst, &st, sb));
        FGI_HIP(g, rocprim::radix_sort_keys(st, sb, k1, k2, (size_t)mi, 0, 64, s));
        hipLaunchKernelGGL(k_in_part_unique, dim3(nblk(mi)), dim3(256), 0, s, mi, k2, keep);
        uint64_t total = 0;
        FGI_TRY(scan_flags(g, keep, kpos, mi, &total));
        // (the lists are rebuilt whole: nothing of the old ones is kept)
        FGI_TRY(grow(g, &g->uin_src, &g->uin_cap, std::max<uint64_t>(total, 1024), "the dependency lists"));
        hipLaunchKernelGGL(k_in_part_rows, dim3(nblk(mi)), dim3(256), 0, s, mi, k2, keep, kpos, g->uin_src, g->uin_off,
                           g->uin_len);
        hipLaunchKernelGGL(k_in_part_fix, dim3(nblk(g->n_slots)), dim3(256), 0, s, g->n_slots, g->uin_off, g->uin_len);
        FGI_TRY(sort_in_lists(g, total, p->weight, p->v.n_global));
    }
    FGI_TRY(build_in_heads(g));
    FGI_HIP(g, hipStreamSynchronize(s));
    g->uin_epoch = g->mut_epoch;   // rows, versions and lists agree
    return FGI_OK;
}

fgi_status part_ensure_lists(fgi_graph* g) {
    PartState* p = ps(g);
    if (!p || g->uin_epoch == g->mut_epoch || p->in_n == 0) return FGI_OK;
    return part_rebuild_lists(g);
}

bool part_codes_wanted(const fgi_graph* g, uint32_t n_global) {
    return labels_capacity(n_global, g->opt_labels) != 0;   // fgi_config.labels / FGI_LABELS, auto from 2^25
}

const uint32_t* part_codes_in(const fgi_graph* g, uint64_t n, const uint32_t* in, std::vector<uint32_t>& out) {
    if (!g->lbl_perm || !in || n == 0) return in;
    out.resize(n);
    const uint64_t N = g->pg_gc_h.size();
    for (uint64_t i = 0; i < n; ++i) out[i] = in[i] < N ? g->pg_gc_h[in[i]] : in[i];
    return out.data();
}

fgi_status part_codes_local(fgi_graph* g, uint32_t* dev, uint64_t n, bool out) {
    PartState* p = ps(g);
    if (!g->lbl_perm || !p || n == 0) return FGI_OK;
    hipLaunchKernelGGL(k_pc_local, dim3(std::min<uint32_t>(nblk(n), 8192)), dim3(256), 0, g->stream, n, dev,
                       out ? g->pg_ig : g->pg_gc, p->v.base, p->v.n_local);
    FGI_HIP(g, hipGetLastError());
    return FGI_OK;
}

uint32_t part_code_local_h(const fgi_graph* g, uint32_t h, bool out) {
    const PartState* p = reinterpret_cast<const PartState*>(g->part);
    if (!g->lbl_perm || !p || h >= p->v.n_local) return h;
    return (out ? g->pg_ig_h : g->pg_gc_h)[p->v.base + h] - p->v.base;
}

// append m device entries (keys: dependant local << 32 | used global, tags) to the in-store
static fgi_status part_store_in(fgi_graph* g, const uint64_t* keys, const uint64_t* tags, uint64_t m) {
    PartState* p = ps(g);
    if (m == 0) return FGI_OK;
    if (p->in_n + m > p->in_cap) {
        const uint64_t cap = std::max<uint64_t>(p->in_n + m, p->in_cap + p->in_cap / 2);
        DevOwn<uint64_t> nk, nt;   // until they are installed
        if (hipMalloc(&nk.p, cap * 8) != hipSuccess || hipMalloc(&nt.p, cap * 8) != hipSuccess)
            return set_err(g, FGI_ENOMEM, "dependency-entry store");
        if (p->in_n) {
            FGI_HIP(g, hipMemcpyAsync(nk.p, p->in_keys, p->in_n * 8, hipMemcpyDeviceToDevice, g->stream));
            FGI_HIP(g, hipMemcpyAsync(nt.p, p->in_tags, p->in_n * 8, hipMemcpyDeviceToDevice, g->stream));
            FGI_HIP(g, hipStreamSynchronize(g->stream));
        }
        hipFree(p->in_keys);
        hipFree(p->in_tags);
        p->in_keys = nk.release();
        p->in_tags = nt.release();
        p->in_cap = cap;
    }
    FGI_HIP(g, hipMemcpyAsync(p->in_keys + p->in_n, keys, m * 8, hipMemcpyDefault, g->stream));
    FGI_HIP(g, hipMemcpyAsync(p->in_tags + p->in_n, tags, m * 8, hipMemcpyDefault, g->stream));
    FGI_HIP(g, hipStreamSynchronize(g->stream));
    p->in_n += m;
    return FGI_OK;
}

static void part_clear_store(PartState* p) {
    hipFree(p->in_keys);
    hipFree(p->in_tags);
    p->in_keys = p->in_tags = nullptr;
    p->in_n = p->in_cap = 0;
}

}  // namespace fgi

using namespace fgi;

extern "C" {

fgi_status fgi_part_unique_id(uint8_t* id128) {
    if (!id128) return FGI_EINVAL;
    if (!rccl_ok()) return FGI_ENOTSUP;
    ncclUniqueId id;
    if (rccl().GetUniqueId(&id) != ncclSuccess) return FGI_EDEVICE;
    std::memcpy(id128, id.internal, NCCL_UNIQUE_ID_BYTES);
    return FGI_OK;
}

static fgi_status part_alloc(fgi_graph* g, uint32_t n_global);

fgi_status fgi_part_init(fgi_graph* g, uint32_t n_global, const uint8_t* id128) {
    if (!g || !id128) return FGI_EINVAL;
    if (g->part) return set_err(g, FGI_ESTATE, "partition already initialised");
    if (!rccl_ok())
        return set_err(g, FGI_ENOTSUP, "RCCL not available (%s: %s)", rccl().path.c_str(), rccl().err.c_str());
    FGI_TRY(part_alloc(g, n_global));
    PartState* p = ps(g);
    ncclUniqueId id;
    std::memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
    // non-blocking communicator: its creation (every rank must join) and every later call that reports
    // ncclInProgress are waited out with a bound (nccl_settle); FGI_RCCL_BLOCKING=1 makes the plain
    // blocking communicator instead (no bounds)
    const char* blk = getenv("FGI_RCCL_BLOCKING");
    ncclResult_t r;
    if (blk && blk[0] == '1') {
        r = rccl().CommInitRank(&p->comm, (int)p->v.world, id, g->rank);
    } else {
        ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
        cfg.blocking = 0;
        r = rccl().CommInitRankConfig(&p->comm, (int)p->v.world, id, g->rank, &cfg);
        if (r == ncclInProgress) {
            const fgi_status st = nccl_settle(g, p->comm, r, "ncclCommInitRankConfig (every rank must join)",
                                              wait_limit_s("FGI_RCCL_INIT_TIMEOUT_S", 120.0));
            if (st != FGI_OK) {
                const std::string err = g->err;
                part_destroy(g);
                g->failed = false;   // the graph itself is intact: the partition was not created
                return set_err(g, st, "%s", err.c_str());
            }
            r = ncclSuccess;
        }
    }
    if (r != ncclSuccess) {
        part_destroy(g);
        return set_err(g, FGI_EDEVICE, "rank %d of %d: ncclCommInitRank: %s", g->rank, g->world, rccl().GetErrorString(r));
    }
    p->ops.reset(new RcclComm());
    return FGI_OK;
}

fgi_status fgi_part_init_host(fgi_graph* g, uint32_t n_global, fgi_allgather_fn fn, void* ctx) {
    if (!g || !fn) return FGI_EINVAL;
    if (g->part) return set_err(g, FGI_ESTATE, "partition already initialised");
    FGI_TRY(part_alloc(g, n_global));
    ps(g)->ops.reset(new HostComm(fn, ctx));
    return FGI_OK;
}

static fgi_status part_alloc(fgi_graph* g, uint32_t n_global) {
    if (!g || g->world < 1 || g->rank < 0 || g->rank >= g->world) return FGI_EINVAL;
    if (g->lbl_K) {   // a partition numbers its slots by rank ranges: no hub-first labels (a fresh graph drops them)
        // node words already written sit at labels K + x (and detached homes hold K + slot): dropping K
        // would lose them, so only a graph with nothing in it yet may join
        if (g->lbl_done || g->pool_top || g->nodes_written)
            return set_err(g, FGI_ESTATE, "a graph with registered nodes or loaded edges cannot join a partition");
        g->lbl_K = 0;
        g->n_slots = g->ext_slots;
        g->n_handles = g->ext_handles;
        g->free_detached.clear();
        for (uint32_t i = g->n_detached; i > 0; --i) g->free_detached.push_back(g->n_slots + i - 1);
    }
    if ((uint32_t)g->world > 8) return set_err(g, FGI_ENOTSUP, "at most 8 partitions (one node)");
    if (g->part) return set_err(g, FGI_ESTATE, "partition already initialised");
    const uint32_t W = (uint32_t)g->world;
    const uint32_t block = (uint32_t)(((uint64_t)n_global + W - 1) / W);
    if (g->n_slots < block) return set_err(g, FGI_EINVAL, "graph has %u slots, partition needs %u", g->n_slots, block);
    hipSetDevice(g->device);
    PartState* p = new PartState();
    g->part = p;
    p->v.rank = (uint32_t)g->rank;
    p->v.world = W;
    p->v.n_global = n_global;
    p->v.block = block;
    p->v.base = (uint32_t)std::min<uint64_t>((uint64_t)block * g->rank, n_global);
    p->v.n_local = (uint32_t)std::min<uint64_t>(block, n_global - p->v.base);
    p->v.sent_words = (uint64_t)n_global / 32 + 2;
    auto fail = [&](const char* what) {
        part_destroy(g);
        return set_err(g, FGI_ENOMEM, "partition allocation failed: %s", what);
    };
    // an empty slot's version is 0 in the replica (fgi_part_register_nodes writes only the present ones)
    if (hipMalloc(&p->v.ver_all, (size_t)n_global * 8) != hipSuccess ||
        hipMemset(p->v.ver_all, 0, (size_t)n_global * 8) != hipSuccess)
        return fail("versions");
    if (hipMalloc(&p->v.sent_bm, p->v.sent_words * 4) != hipSuccess) return fail("sent bitmap");
    if (hipMalloc(&p->v.send_buf, (size_t)W * block * 4) != hipSuccess) return fail("send buffer");
    if (hipMalloc(&p->v.recv_buf, (size_t)W * block * 4) != hipSuccess) return fail("recv buffer");
    if (hipMalloc(&p->v.send_cnt, (size_t)(W + 2) * 8) != hipSuccess) return fail("counts");
    if (hipMalloc(&p->gw, (size_t)(1 + W) * kPartRedMax * 8) != hipSuccess) return fail("counts");
    if (hipMalloc(&p->scalar, 32) != hipSuccess) return fail("scalar");
    // even, so the hot heads' snapshot past its end (kHot / 32 words, build_candidates) is 64-bit aligned
    p->v.front_words_global = ((uint64_t)n_global / 32 + 3) & ~1ull;
    if (hipMalloc(&p->v.front_global, (p->v.front_words_global + kHot / 32) * 4) != hipSuccess) return fail("frontier bitmap");
    // the pull levels' probe summary covers the all-gathered bitmap: one bit per 64-bit word of it
    hipFree(g->sum_bm);
    g->sum_bm = nullptr;
    if (hipMalloc(&g->sum_bm, ((uint64_t)n_global / 4096 + 4) * 8) != hipSuccess) return fail("probe summary");
    if (hipMemset(p->v.front_global, 0, (p->v.front_words_global + kHot / 32) * 4) != hipSuccess) return fail("frontier bitmap");
    if (hipMalloc(&p->v.scratch_u64, 32) != hipSuccess) return fail("scratch");
    if (hipMalloc(&p->weight, (size_t)n_global * 4) != hipSuccess) return fail("list weights");
    if (hipMalloc(&p->dbuf, (size_t)(block / 32 + 1) * 8) != hipSuccess ||
        hipMalloc(&p->rbuf, (size_t)(W > 1 ? W - 1 : 1) * (block / 32 + 1) * 8) != hipSuccess ||
        hipMalloc(&p->dcnt, 8) != hipSuccess)
        return fail("frontier delta buffers");
    if (hipMemset(p->weight, 0, (size_t)n_global * 4) != hipSuccess) return fail("list weights");
    if (hipHostMalloc(reinterpret_cast<void**>(&p->gw_host), (size_t)(1 + W) * kPartRedMax * 8) != hipSuccess)
        return fail("host");
    if (hipHostMalloc(reinterpret_cast<void**>(&p->scalar_host), 32) != hipSuccess) return fail("host");
    // planned waves: buckets of a2a_C words per peer (a push level's forwarded targets beyond that wait
    // for the next push level); 64 K ids per peer moves (world - 1) * 256 KB per rank and level
    p->a2a_C = p->a2a_cap = (uint32_t)std::min<uint64_t>(65536, (uint64_t)block + 1);
    if (hipMalloc(&p->a2a_send, (size_t)W * p->a2a_C * 4) != hipSuccess ||
        hipMalloc(&p->a2a_recv, (size_t)W * p->a2a_C * 4) != hipSuccess || hipMalloc(&p->a2a_cur, (size_t)W * 8) != hipSuccess ||
        hipMalloc(&p->red, (size_t)kPartRedMax * 8) != hipSuccess)
        return fail("planned-wave buffers");
    if (hipMemset(p->a2a_send, 0, (size_t)W * p->a2a_C * 4) != hipSuccess ||
        hipMemset(p->a2a_recv, 0, (size_t)W * p->a2a_C * 4) != hipSuccess)
        return fail("planned-wave buffers");
    if (hipHostMalloc(reinterpret_cast<void**>(&p->red_host), (size_t)kPartRedMax * 8) != hipSuccess) return fail("host");
    return FGI_OK;
}

fgi_status fgi_part_init_local(fgi_graph* const* gs, uint32_t P, uint32_t n_global) {
    if (!gs || P == 0) return FGI_EINVAL;
    for (uint32_t r = 0; r < P; ++r) {
        if (!gs[r] || gs[r]->rank != (int)r || gs[r]->world != (int)P) return FGI_EINVAL;
        FGI_TRY(part_alloc(gs[r], n_global));
    }
    auto grp = std::make_shared<LocalGroup>(std::vector<fgi_graph*>(gs, gs + P));
    for (uint32_t r = 0; r < P; ++r) ps(gs[r])->ops.reset(new LocalComm(grp, r));
    return FGI_OK;
}

// In-process driver: run_part_wave on every rank, one host thread per rank; the collectives meet
// in the group's LocalComm (exactly the level sequence of the RCCL path).
fgi_status fgi_part_local_invalidate(fgi_graph* const* gs, uint32_t P, uint32_t n_roots, const uint32_t* roots,
                                     const uint8_t* immediately, fgi_wave_stats* stats) {
    if (!gs || P == 0 || (n_roots && !roots)) return FGI_EINVAL;
    LocalComm* c0 = nullptr;
    for (uint32_t r = 0; r < P; ++r) {
        if (!gs[r] || !gs[r]->part || ps(gs[r])->v.world != P) return FGI_EINVAL;
        LocalComm* c = dynamic_cast<LocalComm*>(ps(gs[r])->ops.get());
        if (!c || c->rank != r) return set_err(gs[r], FGI_EINVAL, "graph is not rank %u of an in-process group", r);
        if (c0 && c->grp != c0->grp) return set_err(gs[r], FGI_EINVAL, "graphs of different in-process groups");
        c0 = c;
    }
    c0->grp->reset();
    std::vector<fgi_status> st(P, FGI_OK);
    std::vector<std::thread> ts;
    for (uint32_t r = 0; r < P; ++r) {
        ts.emplace_back([&, r]() {
            fgi_graph* g = gs[r];
            hipSetDevice(g->device);
            // the rank's own graph and stream only: its temporaries come from its own cache
            std::vector<uint32_t> mapped;
            const uint32_t* rr = part_codes_in(g, n_roots, roots, mapped);
            Tmp tr, ti;
            uint32_t* rd = nullptr;
            uint8_t* id = nullptr;
            auto wave = [&]() -> fgi_status {
                if (n_roots) {
                    FGI_TRY(tmalloc(g, tr, &rd, n_roots));
                    FGI_HIP(g, hipMemcpyAsync(rd, rr, (size_t)n_roots * 4, hipMemcpyHostToDevice, g->stream));
                    if (immediately) {
                        FGI_TRY(tmalloc(g, ti, &id, n_roots));
                        FGI_HIP(g, hipMemcpyAsync(id, immediately, n_roots, hipMemcpyHostToDevice, g->stream));
                    }
                    FGI_HIP(g, hipStreamSynchronize(g->stream));   // pageable sources
                }
                FGI_TRY(run_part_wave(g, n_roots, rd, id, stats ? stats + r : nullptr));
                part_out_mark(g, kPoutWave);
                return timers_arm_part(g);   // the rank's delay timers of what the wave flagged (timers.hip)
            };
            part_out_mark(g, kPoutOther);   // until the rank's wave stands
            st[r] = wave();
            if (st[r] != FGI_OK) c0->grp->fail();
        });
    }
    for (auto& t : ts) t.join();
    for (uint32_t r = 0; r < P; ++r)
        if (st[r] != FGI_OK) return st[r];
    return FGI_OK;
}

// Checks that gs[0..P) is one in-process group, rank by rank; returns its first member's comm.
static fgi_status local_group(fgi_graph* const* gs, uint32_t P, LocalComm** out) {
    if (!gs || P == 0) return FGI_EINVAL;
    LocalComm* c0 = nullptr;
    for (uint32_t r = 0; r < P; ++r) {
        if (!gs[r] || !gs[r]->part || ps(gs[r])->v.world != P) return FGI_EINVAL;
        LocalComm* c = dynamic_cast<LocalComm*>(ps(gs[r])->ops.get());
        if (!c || c->rank != r) return set_err(gs[r], FGI_EINVAL, "graph is not rank %u of an in-process group", r);
        if (c0 && c->grp != c0->grp) return set_err(gs[r], FGI_EINVAL, "graphs of different in-process groups");
        c0 = c;
    }
    *out = c0;
    return FGI_OK;
}

// Runs fn(rank) on one host thread per rank of an in-process group (the ranks' collectives meet
// in the group); a failing rank fails the group so that the others leave their collectives.
extern "C++" template <class F>
static fgi_status local_run(fgi_graph* const* gs, uint32_t P, LocalComm* c0, F fn) {
    c0->grp->reset();
    std::vector<fgi_status> st(P, FGI_OK);
    std::vector<std::thread> ts;
    for (uint32_t r = 0; r < P; ++r) {
        ts.emplace_back([&, r]() {
            hipSetDevice(gs[r]->device);
            const fgi_status s = fn(r);
            if (s != FGI_OK) c0->grp->fail();
            st[r] = s;
        });
    }
    for (auto& t : ts) t.join();
    for (uint32_t r = 0; r < P; ++r)
        if (st[r] != FGI_OK) return st[r];
    return FGI_OK;
}

// fgi_part_run_batch on every rank of an in-process group. Each rank writes its step outputs into
// private buffers; they are merged afterwards: a detached handle comes from the slot's owner, the
// add_used results and set flags (which every rank computes) must agree across the ranks.
fgi_status fgi_part_local_run_batch(fgi_graph* const* gs, uint32_t P, uint32_t n_steps, const fgi_step* steps,
                                    uint32_t* out_ids, uint64_t cap, uint64_t* out_n, fgi_batch_stats* stats) {
    LocalComm* c0 = nullptr;
    FGI_TRY(local_group(gs, P, &c0));
    if (n_steps && !steps) return FGI_EINVAL;
    std::vector<std::vector<fgi_step>> rs(P, std::vector<fgi_step>(steps, steps + n_steps));
    std::vector<std::vector<std::vector<uint32_t>>> outs(P, std::vector<std::vector<uint32_t>>(n_steps));
    for (uint32_t r = 0; r < P; ++r)
        for (uint32_t k = 0; k < n_steps; ++k)
            if (steps[k].out) {
                outs[r][k].assign(steps[k].n, 0);   // u8 flags fit in the first quarter
                rs[r][k].out = outs[r][k].data();
            }
    std::vector<std::vector<uint32_t>> ids(P);
    std::vector<uint64_t> nid(P, 0);
    FGI_TRY(local_run(gs, P, c0, [&](uint32_t r) -> fgi_status {
        fgi_batch_stats* sr = stats ? stats + r : nullptr;
        if (sr) *sr = fgi_batch_stats{};
        if (out_ids) ids[r].resize(cap);
        return fgi_part_run_batch(gs[r], n_steps, rs[r].data(), out_ids ? ids[r].data() : nullptr, cap, &nid[r], sr);
    }));
    uint64_t total = 0;
    for (uint32_t r = 0; r < P; ++r) total += nid[r];
    if (out_n) *out_n = total;
    if (out_ids && total > cap) return FGI_ECAPACITY;
    for (uint32_t r = 0, at = 0; out_ids && r < P; at += (uint32_t)nid[r], ++r)
        std::memcpy(out_ids + at, ids[r].data(), nid[r] * 4);
    for (uint32_t k = 0; k < n_steps; ++k) {
        const fgi_step& sp = steps[k];
        if (!sp.out) continue;
        if (sp.kind == FGI_STEP_BEGIN_COMPUTE) {
            auto* o = static_cast<uint32_t*>(sp.out);
            for (uint32_t i = 0; i < sp.n; ++i) {
                o[i] = FGI_NONE;
                for (uint32_t r = 0; r < P; ++r) {
                    const PartView& v = ps(gs[r])->v;
                    if (sp.handles[i] - v.base < v.n_local) o[i] = outs[r][k][i];
                }
            }
        } else {
            const size_t bytes = sp.kind == FGI_STEP_SET_OUTPUT ? sp.n : (size_t)sp.n * 4;
            for (uint32_t r = 1; r < P; ++r)
                if (std::memcmp(outs[r].at(k).data(), outs[0][k].data(), bytes) != 0)
                    return set_err(gs[r], FGI_ESTATE, "step %u: rank %u's results differ from rank 0's", k, r);
            std::memcpy(sp.out, outs[0][k].data(), bytes);
        }
    }
    return FGI_OK;
}

// fgi_part_prune on every rank of an in-process group (stats: P entries, nullable).
fgi_status fgi_part_local_prune(fgi_graph* const* gs, uint32_t P, fgi_prune_stats* stats) {
    LocalComm* c0 = nullptr;
    FGI_TRY(local_group(gs, P, &c0));
    return local_run(gs, P, c0, [&](uint32_t r) { return fgi_part_prune(gs[r], stats ? stats + r : nullptr); });
}

// The RCCL library the engine's collectives bind to: the file its entry points were resolved from
// (rccl(): /opt/rocm's librccl, opened privately, whatever other RCCL the process has loaded).
fgi_status fgi_rccl_info(int* version, char* path, uint64_t cap) {
    if (!rccl_ok()) return FGI_ENOTSUP;
    int v = 0;
    if (rccl().GetVersion(&v) != ncclSuccess) return FGI_EDEVICE;
    if (version) *version = v;
    if (path && cap) {
        Dl_info info{};
        const char* f = (dladdr(reinterpret_cast<void*>(rccl().GetVersion), &info) && info.dli_fname) ? info.dli_fname
                                                                                                      : rccl().path.c_str();
        std::strncpy(path, f, cap - 1);
        path[cap - 1] = 0;
    }
    return FGI_OK;
}

fgi_status fgi_part_synth_rmat(fgi_graph* g, uint32_t scale, uint32_t edge_factor, uint64_t seed, uint32_t stale_pct,
                               uint64_t stale_seed) {
    if (!g || !g->part || scale == 0 || scale > 31 || edge_factor == 0 || stale_pct > 100) return FGI_EINVAL;
    PartState* p = ps(g);
    if ((1ull << scale) != p->v.n_global) return set_err(g, FGI_EINVAL, "partition was initialised for %u slots",
                                                         p->v.n_global);
    hipSetDevice(g->device);
    hipStream_t s = g->stream;
    const uint32_t N = p->v.n_global, base = p->v.base, nl = p->v.n_local;
    FGI_HIP(g, hipMemsetAsync(g->node, 0, (size_t)g->n_handles * 8, s));
    FGI_HIP(g, hipMemsetAsync(g->vis_bm, 0, g->bm_words * 4, s));   // a new node table
    g->v_dirty = false;
    g->vis_stale = false;
    note_words(g);
    // partition codes: chosen after the count pass (the weights); a graph that already has codes keeps them
    const bool choose = !g->lbl_perm && part_codes_wanted(g, N) && g->free_detached.size() == g->n_detached;
    hipLaunchKernelGGL(k_versions_local, dim3((nl + 255) / 256), dim3(256), 0, s, nl, base, seed,
                       reinterpret_cast<unsigned long long*>(g->node), g->lbl_perm ? g->pg_ig : (const uint32_t*)nullptr);
    hipLaunchKernelGGL(k_versions_all, dim3((N + 255) / 256), dim3(256), 0, s, N, seed, p->v.ver_all,
                       g->lbl_perm ? g->pg_ig : (const uint32_t*)nullptr);
    part_clear_store(p);
    FGI_HIP(g, hipMemsetAsync(p->weight, 0, (size_t)N * 4, s));
    // the rank's rows and dependency entries, generated by edge-index range (k_rmat_part)
    const uint64_t m = (uint64_t)edge_factor << scale;
    const uint64_t per = (m + kGenBlocks - 1) / kGenBlocks;
    Tmp tcnt, toff, trows, tins, ttags, trtags;
    unsigned long long *cnt, *off;
    uint64_t *rows, *ins, *tags, *rtags = nullptr;
    FGI_TRY(tmalloc(g, tcnt, &cnt, 2 * kGenBlocks));
    FGI_TRY(tmalloc(g, toff, &off, 2 * kGenBlocks));
    hipLaunchKernelGGL(k_rmat_part, dim3(kGenBlocks), dim3(256), 0, s, m, per, scale, seed, base, nl, stale_pct,
                       stale_seed, 0, cnt, (const unsigned long long*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr,
                       p->weight, (const uint32_t*)nullptr, (uint64_t*)nullptr);
    if (choose) {   // the weights by slot are complete: codes, then the versions at them
        g->pool_top = 0;   // the rows are rebuilt below
        FGI_TRY(part_codes_choose(g, p->weight));
        hipLaunchKernelGGL(k_versions_local, dim3((nl + 255) / 256), dim3(256), 0, s, nl, base, seed,
                           reinterpret_cast<unsigned long long*>(g->node), (const uint32_t*)g->pg_ig);
        hipLaunchKernelGGL(k_versions_all, dim3((N + 255) / 256), dim3(256), 0, s, N, seed, p->v.ver_all,
                           (const uint32_t*)g->pg_ig);
    } else if (g->lbl_perm) {   // the weights by slot into code order
        Tmp tw2;
        uint32_t* w2;
        FGI_TRY(tmalloc(g, tw2, &w2, N));
        FGI_HIP(g, hipMemcpyAsync(w2, p->weight, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
        // the weights only: ver_all was written at the codes above
        hipLaunchKernelGGL(k_pc_move_global, dim3(nblk(N)), dim3(256), 0, s, N, (const uint32_t*)g->pg_gc,
                           (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)w2, p->weight);
        FGI_HIP(g, hipGetLastError());
    }
    std::vector<unsigned long long> hc(2 * kGenBlocks), ho(2 * kGenBlocks);
    FGI_HIP(g, hipMemcpyAsync(hc.data(), cnt, hc.size() * 8, hipMemcpyDeviceToHost, s));
    FGI_HIP(g, hipStreamSynchronize(s));
    uint64_t tot[2] = {0, 0};
    for (int c = 0; c < 2; ++c)
        for (uint32_t b = 0; b < kGenBlocks; ++b) {
            ho[c * kGenBlocks + b] = tot[c];
            tot[c] += hc[c * kGenBlocks + b];
        }
    const uint64_t mo = tot[0], mi = tot[1];
    FGI_TRY(tmalloc(g, trows, &rows, mo));
    FGI_TRY(tmalloc(g, tins, &ins, mi));
    FGI_TRY(tmalloc(g, ttags, &tags, mi));
    if (g->lbl_perm) FGI_TRY(tmalloc(g, trtags, &rtags, mo));
    FGI_HIP(g, hipMemcpyAsync(off, ho.data(), ho.size() * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_rmat_part, dim3(kGenBlocks), dim3(256), 0, s, m, per, scale, seed, base, nl, stale_pct,
                       stale_seed, 1, cnt, (const unsigned long long*)off, rows, ins, (uint32_t*)nullptr,
                       g->lbl_perm ? (const uint32_t*)g->pg_gc : (const uint32_t*)nullptr, rtags);
    if (mi)
        hipLaunchKernelGGL(k_in_tags_synth, dim3(nblk(mi)), dim3(256), 0, s, mi, ins, base, seed, tags,
                           g->lbl_perm ? (const uint32_t*)g->pg_ig : (const uint32_t*)nullptr);
    FGI_HIP(g, hipStreamSynchronize(s));
    tcnt.reset();
    toff.reset();
    // rows: (owned used << 32 | global dependant), tags synthesised from global ids (with codes: from the
    // slot ids, by the generator)
    FGI_TRY(build_rows_from_keys(g, mo, rows, rtags, seed, stale_pct, stale_seed, base, base));
    trows.reset();   // before the store grows
    trtags.reset();
    FGI_TRY(part_store_in(g, ins, tags, mi));
    FGI_TRY(part_rebuild_lists(g));
    return view_rebuild(g);   // a new node table: the state view's full build
}

fgi_status fgi_part_register_nodes(fgi_graph* g, uint32_t n, const uint32_t* slot, const uint64_t* version,
                                   const uint32_t* state_flags) {
    if (!g || (n && (!slot || !version))) return FGI_EINVAL;
    if (!g->part) return set_err(g, FGI_ESTATE, "fgi_part_register_nodes: partition not initialised");
    PartState* p = ps(g);
    for (uint32_t i = 0; i < n; ++i) {
        if (slot[i] >= p->v.n_global) return set_err(g, FGI_EINVAL, "slot %u out of range", slot[i]);
        if (version[i] > kVMask) return set_err(g, FGI_EINVAL, "version of slot %u exceeds 2^56-1", slot[i]);
        if (state_flags && (state_flags[i] & 3u) == 3u) return set_err(g, FGI_EINVAL, "bad state for slot %u", slot[i]);
    }
    if (n == 0) return FGI_OK;
    // a Computing node, or one with an invalidation delay, can be flagged by a visit (flagged sets). Any
    // listed node counts, owned or not: every rank sees the same list, so every rank decides alike.
    for (uint32_t i = 0; i < n && state_flags && !g->flag_gate; ++i)
        if (version[i] && ((state_flags[i] & FGI_STATE_MASK) == FGI_COMPUTING || (state_flags[i] & FGI_F_HAS_DELAY)))
            g->flag_gate = true;
    std::vector<uint32_t> mapped;
    slot = part_codes_in(g, n, slot, mapped);   // partition codes
    hipSetDevice(g->device);
    hipStream_t s = g->stream;
    FGI_TRY(fold(g));
    Tmp ts, tv, tf;
    uint32_t *ds, *df = nullptr;
    uint64_t* dv;
    FGI_TRY(tmalloc(g, ts, &ds, n));
    FGI_TRY(tmalloc(g, tv, &dv, n));
    if (state_flags) FGI_TRY(tmalloc(g, tf, &df, n));
    touch(g);          // versions change: the pull lists are rebuilt before the next wave
    note_words(g);
    unsigned long long bad = 0;
    hipError_t e = hipMemcpyAsync(ds, slot, (size_t)n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dv, version, (size_t)n * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && df) e = hipMemcpyAsync(df, state_flags, (size_t)n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(p->scalar, 0, 8, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_part_register, dim3(nblk(n)), dim3(256), 0, s, n, ds, dv, df, p->v.base, p->v.n_local,
                           p->v.ver_all, reinterpret_cast<unsigned long long*>(g->node), g->row_len, p->scalar);
        e = hipMemcpyAsync(&bad, p->scalar, 8, hipMemcpyDeviceToHost, s);
    }
    const hipError_t es = hipStreamSynchronize(s);   // whatever was queued reads the caller's arrays
    FGI_HIP(g, e);
    FGI_HIP(g, es);
    if (bad) return set_err(g, FGI_ESTATE, "%llu owned slots already had a current node", bad);
    return view_rebuild(g);   // a bulk import: the state view's full build
}

fgi_status fgi_part_load_edges(fgi_graph* g, uint64_t m, const uint32_t* used, const uint32_t* dependant,
                               const uint64_t* tag) {
    if (!g || (m && (!used || !dependant || !tag))) return FGI_EINVAL;
    if (!g->part) return set_err(g, FGI_ESTATE, "fgi_part_load_edges: partition not initialised");
    PartState* p = ps(g);
    const uint32_t base = p->v.base, nl = p->v.n_local, N = p->v.n_global;
    for (uint64_t e = 0; e < m; ++e) {
        if (used[e] >= N || dependant[e] >= N)
            return set_err(g, FGI_EINVAL, "edge %llu out of range", (unsigned long long)e);
        if (tag[e] == 0) return set_err(g, FGI_EINVAL, "edge %llu has tag 0 (LTags are positive)", (unsigned long long)e);
    }
    hipSetDevice(g->device);
    // list weights: every rank sees the whole batch (and every version, ver_all). At the first bulk load of a
    // partition that wants codes they decide the codes (by slot), which then number the batch and all else.
    const bool choose = m && part_codes_now(g);
    std::vector<uint32_t> mu, md;
    if (!choose) {
        used = part_codes_in(g, m, used, mu);
        dependant = part_codes_in(g, m, dependant, md);
    }
    if (m) {
        hipStream_t s = g->stream;
        Tmp td, tt;
        uint32_t* dd;
        uint64_t* dt;
        FGI_TRY(tmalloc(g, td, &dd, m));
        FGI_TRY(tmalloc(g, tt, &dt, m));
        hipError_t e = hipMemcpyAsync(dd, dependant, m * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(dt, tag, m * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess)
            hipLaunchKernelGGL(k_part_weight, dim3(nblk(m)), dim3(256), 0, s, m, dd, dt, p->v.ver_all, p->weight);
        const hipError_t es = hipStreamSynchronize(s);   // whatever was queued reads the caller's arrays
        FGI_HIP(g, e);
        FGI_HIP(g, es);
    }
    if (choose) {
        FGI_TRY(part_codes_choose(g, p->weight));
        FGI_TRY(view_rebuild(g));   // the installed words moved: the state view's full build through the new map
        used = part_codes_in(g, m, used, mu);
        dependant = part_codes_in(g, m, dependant, md);
    }
    std::vector<uint64_t> rk, rt, ik, it;
    for (uint64_t e = 0; e < m; ++e) {
        if (used[e] - base < nl) {   // a row this rank owns: (local used, global dependant)
            rk.push_back(((uint64_t)(used[e] - base) << 32) | dependant[e]);
            rt.push_back(tag[e]);
        }
        if (dependant[e] - base < nl) {   // a dependency entry of a slot this rank owns
            ik.push_back(((uint64_t)(dependant[e] - base) << 32) | used[e]);
            it.push_back(tag[e]);
        }
    }
    FGI_TRY(load_rows(g, rk.size(), rk.data(), rt.data(), base, base));
    FGI_TRY(part_store_in(g, ik.data(), it.data(), ik.size()));
    return part_rebuild_lists(g);
}

fgi_status fgi_part_invalidate(fgi_graph* g, uint32_t n_roots, const uint32_t* roots_dev, const uint8_t* imm_dev,
                               uint64_t* out_n, fgi_wave_stats* stats) {
    if (!g || !g->part || (n_roots && !roots_dev)) return FGI_EINVAL;
    hipSetDevice(g->device);
    if (g->lbl_perm && n_roots) {   // the roots' codes (the caller's buffer stays as it is)
        PartState* p = ps(g);
        FGI_TRY(grow(g, &p->roots_codes, &p->roots_cap, n_roots, "the roots' codes"));
        FGI_HIP(g, hipMemcpyAsync(p->roots_codes, roots_dev, (size_t)n_roots * 4, hipMemcpyDeviceToDevice, g->stream));
        hipLaunchKernelGGL(k_pc_global, dim3(std::min<uint32_t>(nblk(n_roots), 4096)), dim3(256), 0, g->stream,
                           (uint64_t)n_roots, p->roots_codes, (const uint32_t*)g->pg_gc, p->v.n_global);
        roots_dev = p->roots_codes;
    }
    part_out_mark(g, kPoutOther);   // until the wave stands
    FGI_TRY(run_part_wave(g, n_roots, roots_dev, imm_dev, stats));
    part_out_mark(g, kPoutWave);
    if (out_n) *out_n = g->last_wave_n;
    return timers_arm_part(g);   // the rank's delay timers of what the wave flagged (timers.hip)
}

// What fgi_part_invalidate_host and fgi_part_invalidate_bits share: the roots checked on the host (every
// rank holds the same list, so every rank refuses alike, before any launch or collective), staged through
// the graph's pinned buffer, mapped to codes on the device, and the wave.
static fgi_status part_wave_from_host(fgi_graph* g, const char* what, uint32_t n_roots, const uint32_t* roots,
                                      const uint8_t* immediately, fgi_wave_stats* stats) {
    if (!g->part) return set_err(g, FGI_ENOTSUP, "%s: not a partitioned graph (fgi_invalidate)", what);
    if (g->failed) return set_err(g, FGI_ESTATE, "%s: the graph is poisoned; fgi_restore or fgi_destroy", what);
    PartState* p = ps(g);
    for (uint32_t i = 0; i < n_roots; ++i)
        if (roots[i] >= p->v.n_global)
            return set_err(g, FGI_EINVAL, "%s: root %u is slot %u of %u", what, i, roots[i], p->v.n_global);
    hipSetDevice(g->device);
    uint32_t* rd = nullptr;
    uint8_t* id = nullptr;
    FGI_TRY(part_out_stage_roots(g, n_roots, roots, immediately, &rd, &id));
    if (g->lbl_perm && n_roots) {
        hipLaunchKernelGGL(k_pc_global, dim3(std::min<uint32_t>(nblk(n_roots), 4096)), dim3(256), 0, g->stream,
                           (uint64_t)n_roots, rd, (const uint32_t*)g->pg_gc, p->v.n_global);
        FGI_HIP(g, hipGetLastError());
    }
    part_out_mark(g, kPoutOther);   // until the wave stands
    FGI_TRY(run_part_wave(g, n_roots, rd, id, stats));
    part_out_mark(g, kPoutWave);
    return timers_arm_part(g);
}

fgi_status fgi_part_invalidate_host(fgi_graph* g, uint32_t n_roots, const uint32_t* roots, const uint8_t* immediately,
                                    uint32_t* out_ids, uint64_t cap, uint64_t* out_n, fgi_wave_stats* stats) {
    if (!g || (n_roots && !roots)) return FGI_EINVAL;
    FGI_TRY(part_wave_from_host(g, "fgi_part_invalidate_host", n_roots, roots, immediately, stats));
    return fgi_part_last_wave_ids(g, out_ids, cap, out_n);   // a short cap: FGI_ECAPACITY, the wave has completed
}

fgi_status fgi_part_invalidate_bits(fgi_graph* g, uint32_t n_roots, const uint32_t* roots, const uint8_t* immediately,
                                    uint64_t* out_bits, uint64_t words, uint64_t* out_n, fgi_wave_stats* stats) {
    if (!g || (n_roots && !roots)) return FGI_EINVAL;
    // a bitmap too short is refused before the wave, as fgi_invalidate_bits refuses it
    if (g->part && out_bits && words < ((uint64_t)g->ext_handles + 63) / 64)
        return set_err(g, FGI_ECAPACITY, "bitmap of %llu words needs %llu", (unsigned long long)words,
                       (unsigned long long)(((uint64_t)g->ext_handles + 63) / 64));
    FGI_TRY(part_wave_from_host(g, "fgi_part_invalidate_bits", n_roots, roots, immediately, stats));
    return fgi_part_last_wave_bits(g, out_bits, words, out_n);
}

fgi_status fgi_part_front_stats(fgi_graph* g, uint64_t* full, uint64_t* delta, uint64_t* bytes) {
    if (!g || !g->part || !full || !delta || !bytes) return FGI_EINVAL;
    return part_front_stats(g, full, delta, bytes);
}

// (a wave's ids without the host loop and sort: fgi_part_last_wave_ids / fgi_part_last_wave_bits, part_out.hip)
fgi_status fgi_part_export_ids(fgi_graph* g, uint32_t* out_ids, uint64_t cap, uint64_t* out_n) {
    if (!g || !g->part) return FGI_EINVAL;
    const uint64_t n = g->last_wave_n;
    if (out_n) *out_n = n;
    if (!out_ids) return FGI_OK;
    if (n > cap) return FGI_ECAPACITY;
    hipSetDevice(g->device);
    FGI_HIP(g, hipMemcpy(out_ids, g->inv, n * 4, hipMemcpyDeviceToHost));
    const uint32_t base = ps(g)->v.base;
    for (uint64_t i = 0; i < n; ++i) out_ids[i] = part_slot_of(g, out_ids[i] + base);   // local -> global slot
    if (g->lbl_perm) std::sort(out_ids, out_ids + n);   // ascending slots
    return FGI_OK;
}

}  // extern "C"

namespace fgi {
fgi_status part_local_run(fgi_graph* const* gs, uint32_t P, const std::function<fgi_status(uint32_t)>& fn) {
    LocalComm* c0 = nullptr;
    FGI_TRY(local_group(gs, P, &c0));
    return local_run(gs, P, c0, fn);
}
}  // namespace fgi
