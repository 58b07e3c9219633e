/*
 * fgi.h — C-ABI of the MI355X cascading-invalidation engine ("fgi": Fusion Graph Invalidation).
 *
 * The engine keeps Stl.Fusion's reverse dependency graph (every Computed's `_usedBy` set) in HBM
 * and runs `Computed.Invalidate()` cascades as batched frontier BFS waves in gfx950 HIP kernels.
 * The reference exposes no FFI seam for the cascade (Computed<T>.Invalidate is non-virtual,
 * `_usedBy` private: src/Stl.Fusion/Computed.cs:36-37, 162); the boundary is a host layer that
 * mirrors ComputedRegistry / `using (Computed.Invalidate())` / IComputed.Invalidated and calls
 * this library (C# `[LibraryImport("fgi")]` stubs in INTEGRATION.md; the C++ mirror is
 * stl.fusion_amd/host/fusion.hpp). Every entry point below names the reference member it
 * replaces.
 *
 * Conventions
 *   - Plain C types only; all arrays are HOST pointers unless the name ends in `_dev`.
 *   - Every function returns an fgi_status; nothing throws or aborts, mirroring
 *     "Invalidate doesn't throw - ever" (Computed.cs:200-229). fgi_last_error() describes the
 *     last failure on a graph.
 *   - A graph is externally synchronised: one caller thread at a time (the host layer funnels
 *     all calls through one dispatcher, which replaces the per-node `lock(this)` of
 *     Computed.cs:42). Calls are synchronous: they return after the device work completed.
 *
 * Node model ("handles")
 *   - A slot is a ComputedInput (ComputedInput.cs / ComputeMethodInput.cs); the host maps each
 *     input to a dense slot id in [0, n_slots). Handle h < n_slots addresses the slot's current
 *     node (the registry entry, ComputedRegistry.cs:22).
 *   - Handles >= n_slots are "detached" nodes: nodes displaced from the registry by a newer
 *     computation while still Computing or while a delayed invalidation is pending
 *     (ComputedRegistry.cs:91-96 leaves such an object alive and unregistered). They keep their
 *     own `_usedBy` row and state; fgi_begin_compute hands them out.
 *   - state_flags word: bits 0-1 ConsistencyState (Computing 0, Consistent 1, Invalidated 2 —
 *     ConsistencyState.cs:5-10), bit 2 InvalidateOnSetOutput, bit 3 InvalidationDelayStarted
 *     (ComputedFlags.cs:4-8), bit 4 hasDelay (ComputedOptions.InvalidationDelay != 0).
 *     Reported flags are canonical: an Invalidated node reports no IOSO/DelayStarted bits and a
 *     non-Computing node no IOSO bit (the reference never reads them again, Computed.cs:145,
 *     164-172), so results are independent of the order in which a batch is applied.
 *   - version: the node's LTag (LTag.cs:13-22), 1 <= version < 2^56 (ConcurrentLTagGenerator
 *     yields values in [1, 2^55]). Edge tags are full 64-bit LTags.
 */
#ifndef FGI_H
#define FGI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int fgi_status;
#define FGI_OK 0
#define FGI_EINVAL 1     /* bad argument */
#define FGI_ENOMEM 2     /* device allocation failed */
#define FGI_ECAPACITY 3  /* output buffer too small: *out_n holds the required size */
#define FGI_EDEVICE 4    /* HIP / RCCL runtime error */
#define FGI_ESTATE 5     /* operation invalid in the node's state */
#define FGI_ENOTSUP 6    /* not supported in this configuration */

#define FGI_NONE 0xFFFFFFFFu

#define FGI_COMPUTING 0u
#define FGI_CONSISTENT 1u
#define FGI_INVALIDATED 2u
#define FGI_STATE_MASK 3u
#define FGI_F_INVALIDATE_ON_SET_OUTPUT 4u
#define FGI_F_INVALIDATION_DELAY_STARTED 8u
#define FGI_F_HAS_DELAY 16u

/* fgi_add_used per-item outcome (Computed.cs:347-385) */
#define FGI_USED_ADDED 0u        /* (dependant.input, dependant.version) added to used._usedBy */
#define FGI_USED_DROPPED 1u      /* dependant not Computing: no-op (Computed.cs:351-364) */
#define FGI_USED_INVALIDATED 2u  /* used already Invalidated: dependant gets InvalidateOnSetOutput (376-378) */
#define FGI_USED_ESTATE 3u       /* used is Computing: the reference throws WrongComputedState (374-375) */

typedef struct fgi_graph fgi_graph;

typedef struct fgi_config {
    uint32_t struct_size;      /* sizeof(fgi_config) */
    int32_t device;            /* HIP device ordinal */
    uint32_t n_slots;          /* slot capacity (registry keys) */
    uint32_t n_detached;       /* capacity for detached nodes (handles n_slots .. n_slots+n_detached) */
    uint64_t edge_capacity;    /* initial edge-pool capacity (grows on demand) */
    /* multi-GPU 1-D vertex partition (fgi_part_*); 0/1 for a single device */
    int32_t rank;
    int32_t world;
    /* Internal labels: 0 auto — a single-device graph of at least 2^25 slots (an
     * invalidated bitmap larger than one XCD's L2) relabels its heaviest slots into a prefix of the
     * engine's handle space at its first bulk edge load; 1 always (tests); -1 never. Invisible at the
     * boundary: every entry point takes and returns slots and handles as before. Callers built against
     * the previous layout of this struct (struct_size without this field) get 0. */
    int32_t labels;
    int32_t reserved;
} fgi_config;

typedef struct fgi_wave_stats {
    uint64_t roots;            /* root entries submitted */
    uint64_t levels;           /* BFS levels with a non-empty frontier */
    uint64_t v_inv;            /* Consistent -> Invalidated transitions (= expanded nodes) */
    uint64_t e_trav;           /* sum of |_usedBy| over invalidated nodes (TEPS numerator). Exact on a
                                  graph's first wave (and after fgi_restore / fgi_prune); after earlier
                                  waves it also counts the entries RemoveUsedBy would have removed
                                  (Computed.cs:387-398), which the engine drops lazily at the next prune,
                                  so it can exceed the reference's count until then */
    uint64_t e_match;          /* traversed edges whose tag == version of the dst slot's node */
    uint64_t n_flagged;        /* visits that only set InvalidateOnSetOutput / DelayStarted */
    uint64_t alg_bytes;        /* algorithmic HBM bytes of the wave */
    double kernel_ms;          /* device time of the wave's kernels (HIP events) */
    double total_ms;           /* wall time of the call */
    uint64_t remote_msgs;      /* multi-GPU: frontier messages sent to other partitions */
    uint64_t f_total;          /* frontier entries expanded (invalidated nodes with |_usedBy| > 0) */
    uint64_t expand_launches;  /* expand kernel launches that had work */
    double expand_ms;          /* summed device time of those launches (HIP events) */
    uint64_t expand_bytes;     /* algorithmic bytes of those launches */
    uint64_t pull_levels;      /* levels run bottom-up */
    uint64_t pull_edges;       /* dependency-list entries examined by pull levels */
    double pull_ms;            /* device time of the k_pull launches (HIP events) */
    uint64_t pull_bytes;       /* algorithmic bytes of the k_pull launches */
    uint64_t pull_launches;    /* k_pull launches (every level of a wave that may pull) */
    /* fused waves: the head and tail launches that run the roots, the small push levels,
       the collect after a pull level and the final count inside one persistent grid each */
    uint64_t fused_launches;   /* persistent launches: the wave tail (k_wave_tail), or a fused wave's head / tail */
    double fused_ms;           /* their summed device time (HIP events, FGI_OPT_LEVEL_TIMING) */
    uint64_t fused_push_bytes; /* algorithmic bytes of the push levels they ran (20 B per edge + 40 B
                                  per frontier entry, as a k_level push) */
    uint64_t host_syncs;       /* times the wave waited for the device */
    uint64_t pull_pushed;      /* asynchronous waves: levels past the queued group that the automatic
                                  direction choice would pull and the wave ran as push (same result,
                                  slower; the next queued wave's group covers them) */
} fgi_wave_stats;

typedef struct fgi_prune_stats {
    uint64_t old_edges;        /* sum of |_usedBy| over pruned (Consistent, registered) nodes before */
    uint64_t new_edges;        /* ... and after (ComputedGraphPruner.cs:91-93) */
    uint64_t pool_before;      /* edge-pool slots in use (pool top) before */
    uint64_t pool_after;       /* ... and after (smaller only if the pass defragmented the pool) */
    double kernel_ms;          /* device time of the pruning kernels (HIP events) */
    double total_ms;           /* wall time of the call */
    uint64_t live_edges;       /* entries left in the rows the call visited */
    uint64_t dropped_edges;    /* entries of Invalidated nodes' rows dropped (their `_usedBy` was cleared) */
    uint32_t first, count;     /* the handle range visited */
    uint64_t stale_estimate;   /* fgi_prune_step: the estimate that triggered the batch */
} fgi_prune_stats;

/* ---- lifetime ------------------------------------------------------------------------------ */
fgi_status fgi_create(const fgi_config* cfg, fgi_graph** out);      /* new ComputedRegistry (ComputedRegistry.cs:38-52) */
fgi_status fgi_destroy(fgi_graph* g);                                /* ComputedRegistry.Dispose (54-55) */
const char* fgi_last_error(const fgi_graph* g);
fgi_status fgi_version(uint32_t* major, uint32_t* minor);

/* ---- registry / node state ---------------------------------------------------------------- */
/* Bulk import of current nodes (ComputedRegistry.Register, ComputedRegistry.cs:72-105, without
 * displacement: the slots must be empty). version[i] == 0 leaves the slot empty. */
fgi_status fgi_register_nodes(fgi_graph* g, uint32_t n, const uint32_t* slot, const uint64_t* version,
                              const uint32_t* state_flags);
/* Bulk import of `_usedBy` entries: used[i]._usedBy += (dependant_slot[i], tag[i])
 * (IComputedImpl.AddUsedBy body, Computed.cs:381-382, no state checks). Set semantics
 * (HashSetSlim3.Add, HashSetSlim3.cs:31-64): duplicate entries collapse. */
fgi_status fgi_load_edges(fgi_graph* g, uint64_t m, const uint32_t* used, const uint32_t* dependant_slot,
                          const uint64_t* tag);
/* IComputed.Version / ConsistencyState / flags for handles (Computed.cs:46-48). */
fgi_status fgi_get_state(fgi_graph* g, uint32_t n, const uint32_t* handle, uint64_t* version,
                         uint32_t* state_flags);
/* Whole-table dump (n_slots + n_detached entries) — for parity checks. */
fgi_status fgi_dump_states(fgi_graph* g, uint64_t* version, uint32_t* state_flags);
/* IComputedImpl.UsedBy (Computed.cs:337-345): the `_usedBy` entries of one node as the reference
 * would hold them: an entry (d, t) whose node d@t was invalidated is gone (RemoveUsedBy,
 * Computed.cs:387-398; the engine removes it lazily), and an Invalidated node reports none (its
 * set was cleared, Computed.cs:217). fgi_export_edges shows the raw pool instead. */
fgi_status fgi_get_used_by(fgi_graph* g, uint32_t handle, uint32_t* dependant_slot, uint64_t* tag,
                           uint64_t cap, uint64_t* out_n);
/* IComputedImpl.Used.Length for a node (Computed.cs:327-335). */
fgi_status fgi_get_used_count(fgi_graph* g, uint32_t handle, uint32_t* out);
/* Out-degree (|_usedBy|) of every handle, and the total. */
fgi_status fgi_get_degrees(fgi_graph* g, uint32_t* degree /*n_slots+n_detached, nullable*/, uint64_t* total);

/* ---- host-memory state view (C-ABI 0.6) ------------------------------------------------------- */
/* IComputed.ConsistencyState as the reference reads it: a plain field (Computed.cs:46), on its most
 * frequent path, the cache hit of ComputedExt.TryUseExisting (Internal/ComputedExt.cs:13-22). The view is
 * a state table in host memory that the device keeps current, so a state read is a load and no call.
 * Layout: six bit planes of `words` 64-bit words each, in host memory the engine owns and the device
 * writes. Bit h % 64 of word h / 64 addresses boundary handle h, detached handles included.
 *   registered     handle h holds a node (version != 0)
 *   consistent     state == Consistent
 *   computing      registered and state == Computing
 *   ioso           canonical FGI_F_INVALIDATE_ON_SET_OUTPUT (Computing nodes only)
 *   delay_started  canonical FGI_F_INVALIDATION_DELAY_STARTED (never on an Invalidated node)
 *   has_delay      FGI_F_HAS_DELAY
 * fgi_view_flags(v, h) is the state_flags word fgi_get_state reports for h (0 for an empty handle). A wave
 * clears bits of `consistent` only (and of `delay_started` where an `immediately` root invalidates a
 * delayed node), so a dense wave moves one plane, and fgi_view_is_consistent is one load and one bit test.
 * Guarantee: when a synchronous entry point returns — fgi_state_view_open itself included, on a graph
 * already populated — the view is exact. After fgi_wave_wait* returns for ticket t the view holds at
 * least the waves up to t. With waves in flight each 64-bit plane word is either its old or its new
 * value. *seq is written by the calling host thread: odd from a call's first launch that may touch the
 * view (an asynchronous wave: from its queueing) until the wait that makes the view exact, even
 * otherwise. Any thread may read the planes at any time (relaxed atomic loads: the helpers below); a
 * reader that needs several planes consistent with each other reads seq before and after and retries
 * if it was odd or has changed.
 * Reading the view and keeping it current have no other observable effect: no wave result, flagged set
 * or statistic changes. A graph that never opened a view allocates and launches nothing for it. With a
 * view open a wave keeps its invalidated bitmap to its end, so the next wave starts with its init
 * kernel again (as on a graph that can flag), and a call on a graph that can flag waits once more for
 * the device (fgi_view_stats.extra_waits); on a graph that cannot flag a wave's view update is queued
 * before the wave's own publish and costs no further wait.
 * FGI_ENOTSUP on a partitioned graph (each rank holds its slots' share: fgi_part_state_view_open
 * below); FGI_ESTATE on a poisoned graph. After a call that failed with FGI_EDEVICE the view is
 * undefined until fgi_restore; fgi_restore with a view open returns only once the view shows the
 * snapshot's states (it waits for the device; without a view it stays stream-ordered). fgi_destroy
 * closes the view; the planes stay mapped until then, a closed view is no longer updated, and a second
 * open returns the same planes, rebuilt. */
typedef struct fgi_state_view {
    uint32_t struct_size;          /* in: sizeof(fgi_state_view) */
    uint32_t n_handles;            /* n_slots + n_detached */
    uint64_t words;                /* 64-bit words per plane = (n_handles + 63) / 64 */
    const uint64_t* registered;
    const uint64_t* consistent;
    const uint64_t* computing;
    const uint64_t* ioso;
    const uint64_t* delay_started;
    const uint64_t* has_delay;
    const uint64_t* seq;           /* even: no update in progress; odd: one is */
} fgi_state_view;
fgi_status fgi_state_view_open(fgi_graph* g, fgi_state_view* out);
fgi_status fgi_state_view_close(fgi_graph* g);
/* updates: calls that updated the view; words_published: 64-bit plane words written to host memory
 * (a full build writes every plane); full_builds: passes over every handle (open, bulk loads,
 * fgi_restore); extra_waits: device waits made for the view alone. All zero on a graph that never
 * opened a view. */
typedef struct fgi_view_stats {
    uint64_t updates, words_published, full_builds, extra_waits;
} fgi_view_stats;
fgi_status fgi_state_view_stats(fgi_graph* g, fgi_view_stats* out);

/* The same view per rank of a partition (C-ABI 0.7), over the rank's local boundary handles exactly as
 * fgi_get_state and fgi_dump_states address them on that rank: bit h with h < cfg.n_slots is global slot
 * rank * block + h (block = ceil(n_global / world)) in the host's numbering (partition codes are never
 * visible), the rank's detached handles follow the slots, n_handles = n_slots + n_detached. Slot bits
 * past the rank's last owned slot (the last rank when it owns fewer than block slots, or n_slots > block) stay 0 in every plane.
 * *out_base (nullable) = rank * block. The contract is fgi_state_view_open's, per rank: when a
 * synchronous fgi_part_* call returns on a rank, that rank's view is exact (fgi_part_local_*: every
 * rank's, when the group call returns); *seq is written by the rank's own calling thread. No collective
 * runs: a rank opens, reads and closes (fgi_state_view_close, fgi_state_view_stats) on its own, at any
 * time, and a partition that never opens a view allocates and launches nothing for it. A wave's update
 * rides on the wave's own last wait; a rank whose graph can flag waits once more per cascade. A direct
 * mutation call waits once more for its own items: fgi_part_begin_compute and fgi_part_set_output at
 * most twice with a view open (their cascade's flagged records, then their items), fgi_part_add_used
 * once, fgi_release once; fgi_part_run_batch once for the whole batch (all counted in extra_waits). FGI_ENOTSUP on a graph that is not partitioned, FGI_ESTATE on a poisoned one. */
fgi_status fgi_part_state_view_open(fgi_graph* g, fgi_state_view* out, uint32_t* out_base /*nullable*/);

/* The read path. The helpers are inline C for hosts that include this header; the library also exports
 * them under the same names for bindings that cannot inline C (its own build defines
 * FGI_VIEW_OUT_OF_LINE). */
#define FGI_VIEW_BIT(plane, h) ((__atomic_load_n((plane) + ((h) >> 6), __ATOMIC_RELAXED) >> ((h) & 63u)) & 1u)
#ifdef FGI_VIEW_OUT_OF_LINE
#define FGI_VIEW_INLINE
#else
#define FGI_VIEW_INLINE static inline
#endif
/* one load, one bit test */
FGI_VIEW_INLINE int fgi_view_is_consistent(const fgi_state_view* v, uint32_t h) {
    return h < v->n_handles && FGI_VIEW_BIT(v->consistent, h);
}
/* A global slot over the p views of a partition's ranks (rank order; block = ceil(n_global / p)), for a
 * host that runs the ranks in one process: one divide, one load, one bit test; 0 for slot >= p * block. */
FGI_VIEW_INLINE int fgi_part_view_is_consistent(const fgi_state_view* views, uint32_t p, uint32_t block, uint32_t slot) {
    const uint32_t r = block ? slot / block : p;
    return r < p && fgi_view_is_consistent(views + r, slot - r * block);
}
/* the canonical state_flags of handle h (what fgi_get_state reports); 0 for an empty handle */
FGI_VIEW_INLINE uint32_t fgi_view_flags(const fgi_state_view* v, uint32_t h) {
    uint32_t f;
    if (h >= v->n_handles || !FGI_VIEW_BIT(v->registered, h)) return 0u;
    f = FGI_VIEW_BIT(v->has_delay, h) ? FGI_F_HAS_DELAY : 0u;
    if (FGI_VIEW_BIT(v->consistent, h))
        return f | FGI_CONSISTENT | (FGI_VIEW_BIT(v->delay_started, h) ? FGI_F_INVALIDATION_DELAY_STARTED : 0u);
    if (FGI_VIEW_BIT(v->computing, h))
        return f | FGI_COMPUTING | (FGI_VIEW_BIT(v->ioso, h) ? FGI_F_INVALIDATE_ON_SET_OUTPUT : 0u) |
               (FGI_VIEW_BIT(v->delay_started, h) ? FGI_F_INVALIDATION_DELAY_STARTED : 0u);
    return f | FGI_INVALIDATED;
}

/* ---- dependency capture (compute-method call path) ----------------------------------------- */
/* ComputeMethodFunctionBase.Compute (ComputeMethodFunctionBase.cs:19-27): a new Computing node of
 * version[i] becomes the current node of slot[i] (registered in its ctor,
 * ComputeMethodComputed.cs:9-11). A current node is displaced as ComputedRegistry.Register does
 * (ComputedRegistry.cs:83-97): it is invalidated (immediately=false) — a cascade root — and, if it
 * survives that (Computing, or Consistent with an invalidation delay), it is detached and its
 * handle returned in out_detached[i] (FGI_NONE otherwise). Slots must be distinct in one call. */
fgi_status fgi_begin_compute(fgi_graph* g, uint32_t n, const uint32_t* slot, const uint64_t* version,
                             const uint8_t* has_delay /*nullable*/, uint32_t* out_detached /*nullable*/,
                             fgi_wave_stats* stats /*nullable*/);
/* dependant.AddUsed(used) for each pair (IComputedImpl.AddUsed/AddUsedBy, Computed.cs:347-385,
 * reached from ComputedExt.UseNew / TryUseExisting, Internal/ComputedExt.cs:13-22, 70-76).
 * out_result[i] gets an FGI_USED_* code. Pairs in one call are applied as one batch. A `used` handle that
 * names no node (an empty slot, a released detached handle) counts as Invalidated: FGI_USED_INVALIDATED, and
 * the dependant gets InvalidateOnSetOutput (the reference passes node objects, so it has no such case; a
 * computed that is gone can only be treated as one that must not be relied on).
 * Deviation from SURVEY.md §8(b)'s sketch `(src_slot, dst_slot, dst_version)`: the pairs are node
 * handles, as the reference's AddUsed takes node objects (Computed.cs:347, `AddUsed(IComputedImpl
 * used)`), not (input, version) keys. The dependant's version is its node's own (a handle names one
 * node: a slot's current node, or a detached one), so an entry can never carry a version the
 * dependant node does not have, and a detached (displaced, still Computing) dependant is addressable. */
fgi_status fgi_add_used(fgi_graph* g, uint32_t n, const uint32_t* dependant, const uint32_t* used,
                        uint32_t* out_result /*nullable*/);
/* Computed<T>.TrySetOutput (Computed.cs:141-160) for each handle: Computing -> Consistent;
 * nodes flagged InvalidateOnSetOutput are invalidated at once in one cascade wave.
 * out_set[i] = 1 if the node was Computing. */
fgi_status fgi_set_output(fgi_graph* g, uint32_t n, const uint32_t* handle, uint8_t* out_set /*nullable*/,
                          uint32_t* out_ids /*nullable*/, uint64_t cap, uint64_t* out_n /*nullable*/,
                          fgi_wave_stats* stats /*nullable*/);

/* ---- invalidation (the hot path) ----------------------------------------------------------- */
/* One batched cascade: for each root handle, `existing.Invalidate(immediately[i])`
 * (Computed.Invalidate() scope -> ComputedExt.TryUseExisting -> Computed.cs:162-230, recursing
 * through every `_usedBy` entry whose version still matches, 212-216). immediately may be NULL
 * (all false — what the scope does). The invalidated set is written to out_ids (handles, in
 * ascending order); if cap is too small, FGI_ECAPACITY is returned with *out_n = required size (the
 * wave itself has completed). out_ids may be NULL to skip the copy: the wave then only counts (no list
 * is written) and the list is made on demand by fgi_last_wave_ids / fgi_wave_ids_dev. */
fgi_status fgi_invalidate(fgi_graph* g, uint32_t n_roots, const uint32_t* roots, const uint8_t* immediately,
                          uint32_t* out_ids, uint64_t cap, uint64_t* out_n, fgi_wave_stats* stats);
/* Same with device-resident roots / flags / output (bench and pipelined host layers). out_ids_dev
 * may be NULL: the call then returns the count alone, the wave writes no id list and keeps its
 * invalidated bitmap in device memory until the next wave starts; fgi_wave_ids_dev / fgi_last_wave_ids
 * make the ascending list from it on demand (0.03 ms for configs[1]'s 7.4M ids, 0.10 ms for configs[2]'s
 * 41M). With out_ids_dev the list is written inside the wave, as before. */
fgi_status fgi_invalidate_dev(fgi_graph* g, uint32_t n_roots, const uint32_t* roots_dev,
                              const uint8_t* immediately_dev, uint32_t* out_ids_dev, uint64_t* out_n,
                              fgi_wave_stats* stats);
/* The same wave as fgi_invalidate, with the invalidated set returned as a bitmap over handles: bit h of
 * out_bits[h / 64] set = handle h was invalidated by this wave; `words` >= (n_slots + n_detached + 63)
 * / 64 (else FGI_ECAPACITY). *out_n = V_inv. A 16.8M-slot graph's bitmap is 2 MB against 29.5 MB of
 * ids for configs[1]'s 7.4M-node wave: the host decodes it where it consumes the set. The id list
 * stays available through fgi_last_wave_ids / fgi_wave_ids_dev (made on demand). out_bits may be NULL. */
fgi_status fgi_invalidate_bits(fgi_graph* g, uint32_t n_roots, const uint32_t* roots, const uint8_t* immediately,
                               uint64_t* out_bits, uint64_t words, uint64_t* out_n, fgi_wave_stats* stats);
/* Asynchronous waves (ComputedExt.WhenInvalidated, ComputedExt.cs:99-125, which the RPC server awaits
 * at Client/Internal/RpcInboundComputeCall.cs:53): fgi_invalidate_async queues the wave
 * fgi_invalidate_dev would run (device-resident roots, boundary handles) on the graph's stream and
 * returns without waiting; *ticket names it (1, 2, ...). At most two waves are in flight: a third call
 * first waits for the oldest. The next call's host work (fgi_restore, root uploads, its launches)
 * overlaps the device's previous wave. fgi_wave_wait waits for the ticket's wave (and every earlier
 * one) and returns its V_inv, its statistics and a device pointer to its invalidated ids (ascending;
 * valid until the wave two tickets later is queued, or any synchronous wave runs); waiting again for a
 * completed ticket returns its results again until the wave two tickets later is queued (FGI_EINVAL
 * after that). Every other entry point except fgi_restore and
 * fgi_set_option first waits for the waves in flight. A wave queued this way runs all its levels in
 * one queue (no second level group): its later pull levels, if the previous wave's shape predicted
 * fewer, run as push levels — same result, slower, and counted in fgi_wave_stats.pull_pushed. A wave
 * whose tail's grid barrier times out fails its fgi_wave_wait with FGI_EDEVICE and poisons the graph
 * until fgi_restore, as a synchronous wave does. */
fgi_status fgi_invalidate_async(fgi_graph* g, uint32_t n_roots, const uint32_t* roots_dev, const uint8_t* imm_dev,
                                uint64_t* ticket);
fgi_status fgi_wave_wait(fgi_graph* g, uint64_t ticket, uint64_t* out_n, const uint32_t** ids_dev,
                         fgi_wave_stats* stats);
/* The same pair for a host layer that holds its roots and wants its ids in host memory (the scope-dispose
 * flush of `using (Computed.Invalidate())` with ComputedExt.WhenInvalidated awaited later): the roots
 * (boundary handles, as fgi_invalidate) are staged through a pinned buffer of the ticket's own and copied
 * on the graph's stream, so the call returns without waiting; fgi_wave_wait_ids waits like fgi_wave_wait
 * and copies the ticket's ids (ascending) into out_ids (FGI_ECAPACITY with *out_n set if cap is short;
 * out_ids may be NULL for the count). A wave queued after the ticket keeps running during the copy. */
fgi_status fgi_invalidate_async_host(fgi_graph* g, uint32_t n_roots, const uint32_t* roots, const uint8_t* immediately,
                                     uint64_t* ticket);
fgi_status fgi_wave_wait_ids(fgi_graph* g, uint64_t ticket, uint32_t* out_ids, uint64_t cap, uint64_t* out_n,
                             fgi_wave_stats* stats);
/* Page-locked host memory for the calls' host arrays (roots in, ids / bitmaps out): copies from and
 * to it run at full PCIe rate without a staging copy (SURVEY.md §8(b) "Ownership"). */
fgi_status fgi_alloc_pinned(uint64_t bytes, void** out);
fgi_status fgi_free_pinned(void* p);
/* Device pointer to the last wave's invalidated-slot list (valid until the next call). */
fgi_status fgi_wave_ids_dev(fgi_graph* g, const uint32_t** ids_dev, uint64_t* n);
/* Host copy of the last wave's invalidated handles — e.g. the displacement cascade of
 * fgi_begin_compute, whose Invalidated handlers the host must still run. */
fgi_status fgi_last_wave_ids(fgi_graph* g, uint32_t* out_ids, uint64_t cap, uint64_t* out_n);
/* The two branches of Computed.Invalidate() that do not invalidate (Computed.cs:173-178: a Computing node
 * only gets InvalidateOnSetOutput, and InvalidationDelayStarted from an `immediately` root; Computed.cs:186-197:
 * a Consistent node with an InvalidationDelay only gets InvalidationDelayStarted and schedules its own
 * timer, ComputedExt.Invalidate(TimeSpan), ComputedExt.cs:10-37, which later calls Invalidate(true)).
 * The flagged set of a call: every handle whose canonical state_flags gained
 * FGI_F_INVALIDATE_ON_SET_OUTPUT and / or FGI_F_INVALIDATION_DELAY_STARTED during the call and that the call
 * did not invalidate — the difference of two state dumps, whatever the order of the visits
 * (fgi_wave_stats.n_flagged stays a visit count). The host starts its timers from it.
 * fgi_last_wave_flagged: the flagged set of the last cascade of the last call (fgi_invalidate, _dev, _bits,
 * fgi_invalidate_all, fgi_begin_compute's displacement cascade, fgi_set_output's cascade; empty if the call
 * ran no cascade): boundary handles (detached ones included), ascending; out_flags[i] (nullable) = the
 * node's canonical state_flags after the call. A slot fgi_begin_compute displaced is not listed (its
 * handle names the new node when the call returns; the displaced node is out_detached[i]). FGI_ECAPACITY
 * with *out_n set if cap is short; out_ids NULL = count only. Valid until the next call that runs a wave.
 * After fgi_run_batch: FGI_ENOTSUP (a batch's cascades report through fgi_last_batch_flagged); after any
 * fgi_part_* call, and on any partitioned graph: FGI_ENOTSUP (a partition's cascades report through
 * fgi_part_last_flagged, rank by rank).
 * A graph that never held a Computing node or one with hasDelay reports empty sets at no cost: its waves
 * launch nothing for them. */
fgi_status fgi_last_wave_flagged(fgi_graph* g, uint32_t* out_ids, uint32_t* out_flags, uint64_t cap, uint64_t* out_n);
/* The same for an asynchronous ticket (waits like fgi_wave_wait; same validity window as the ticket's ids:
 * until the wave two tickets later is queued or a synchronous wave runs); out_flags[i] = the node's
 * canonical state_flags after the ticket's wave. */
fgi_status fgi_wave_wait_flagged(fgi_graph* g, uint64_t ticket, uint32_t* out_ids, uint32_t* out_flags,
                                 uint64_t cap, uint64_t* out_n);
/* ComputedRegistry.InvalidateEverything (ComputedRegistry.cs:142-147). */
fgi_status fgi_invalidate_all(fgi_graph* g, uint32_t* out_ids, uint64_t cap, uint64_t* out_n,
                              fgi_wave_stats* stats);

/* ---- replica fan-out (C-ABI 0.9) ----------------------------------------------- */
/* The RPC server's side of a replica: RpcInboundComputeCall awaits WhenInvalidated on the computed it served
 * and then sends one `$sys-c.Invalidate(callId)` to its peer (Client/Internal/RpcInboundComputeCall.cs:53-62,
 * 102-106; ComputedExt.WhenInvalidated, ComputedExt.cs:99-125). The engine keeps those subscriptions in device
 * memory and joins them with a wave's invalidated set there: {invalidated handles} x {handle -> (peer, call
 * id)}, returned as call ids grouped by peer, ready to send. No per-node data crosses to the host.
 * Entries and lifetime
 *   - An entry is (boundary handle, peer < FGI_MAX_PEERS, 64-bit call id); detached handles are included.
 *   - No set semantics: the same triple stored twice is delivered twice.
 *   - One-shot: the fan-out that delivers an entry removes it (WhenInvalidated completes once).
 * fgi_subscribe stores n entries. out_result[i] (nullable) is FGI_SUB_ADDED, or FGI_SUB_INVALIDATED when the
 * node is already Invalidated or the handle is empty: WhenInvalidated completes at once (ComputedExt.cs:99-125),
 * nothing is stored and the host sends the message now. The state is the node's as it stands after the last
 * wave, read from its node word and visit bit: no fold, no pass over the graph, and the last wave's id list,
 * bitmap and flagged set stay as they are. A handle >= n_slots + n_detached or a peer >= FGI_MAX_PEERS returns
 * FGI_EINVAL and stores nothing.
 * fgi_last_wave_fanout returns the entries of every handle in the last wave's invalidated set. It is valid
 * exactly where fgi_last_wave_ids is (after fgi_invalidate, _dev, _bits, fgi_invalidate_all, fgi_begin_compute,
 * fgi_set_output) until the next call that runs a cascade or a fan-out, or fgi_restore. The lists are made on
 * demand, once per wave: a second call returns the same arrays again, and so does a retry after FGI_ECAPACITY
 * (*out_n holds the count). The entries leave the table when the lists are made, not when they are copied.
 * n_peers must exceed every stored peer id (and be at most FGI_MAX_PEERS), else FGI_EINVAL and nothing is
 * removed. After fgi_restore, or before any wave: FGI_OK with 0 entries. After fgi_run_batch or an asynchronous
 * ticket: FGI_ENOTSUP (use fgi_fanout_ids). On a partitioned graph these four calls return FGI_ENOTSUP (each
 * rank has its own: the fgi_part_* section below); on a poisoned graph FGI_ESTATE.
 * A host that subscribes takes the fan-out of every wave before it begins a new computation on an invalidated
 * slot: an entry left on a slot whose node a wave invalidated would otherwise fire with the next node there.
 * fgi_fanout_ids is the same join for any strictly ascending handle list the host already holds (a batch's
 * out_ids cascade by cascade, fgi_wave_wait_ids): one upload, and a handle without entries costs one bit test.
 * A list that is not strictly ascending or names a handle out of range returns FGI_EINVAL. If cap is short it
 * returns FGI_ECAPACITY with *out_n set and removes nothing.
 * Output: peer_off[p] .. peer_off[p + 1] is peer p's range of call_ids / handles, peer_off[n_peers] == *out_n,
 * a peer without entries has an empty range. Within a peer the order is ascending handle (the order the C++
 * mirror delivers in); entries of the same handle and peer come in unspecified order. handles[i] is the handle
 * whose invalidation released call_ids[i] (the host drops its RpcInboundComputeCall by it).
 * Entries follow the node, not the slot: when fgi_begin_compute displaces a node that survives
 * (out_detached[i] != FGI_NONE) its entries move to the detached handle; fgi_run_batch applies the same moves
 * for its BEGIN_COMPUTE steps behind the batch, in step order (nobody can subscribe mid-batch, so only the
 * first such step on a slot can have entries to move). fgi_release of a handle that still has entries drops
 * them, fgi_unsubscribe_peer drops a disconnected peer's; both count in fgi_sub_stats.dropped.
 * fgi_snapshot / fgi_restore leave the table alone.
 * A graph that never subscribes allocates and launches nothing for any of this. */
#define FGI_MAX_PEERS 4096u
#define FGI_SUB_ADDED 0u
#define FGI_SUB_INVALIDATED 1u
fgi_status fgi_subscribe(fgi_graph* g, uint32_t n, const uint32_t* handle, const uint32_t* peer,
                         const uint64_t* call_id, uint32_t* out_result /*nullable*/);
fgi_status fgi_last_wave_fanout(fgi_graph* g, uint32_t n_peers, uint64_t* peer_off /*n_peers+1*/,
                                uint64_t* call_ids /*nullable*/, uint32_t* handles /*nullable*/,
                                uint64_t cap, uint64_t* out_n);
fgi_status fgi_fanout_ids(fgi_graph* g, uint64_t n, const uint32_t* ids /*host, strictly ascending*/,
                          uint32_t n_peers, uint64_t* peer_off, uint64_t* call_ids, uint32_t* handles,
                          uint64_t cap, uint64_t* out_n);
fgi_status fgi_unsubscribe_peer(fgi_graph* g, uint32_t peer, uint64_t* out_dropped /*nullable*/);
/* live: entries stored now; pool: record capacity of the table; delivered / dropped: entries that left through
 * a fan-out / through fgi_release and fgi_unsubscribe_peer (delivered + dropped + live = entries ever stored);
 * fanouts: fan-outs that launched kernels, of which from_list read an id list and from_bits the invalidated
 * bitmap; last_kernel_ms: device time of the last one's kernels (HIP events). All zero on a graph that never
 * subscribed. */
typedef struct fgi_sub_stats {
    uint64_t live, pool, delivered, dropped, fanouts, from_list, from_bits;
    double last_kernel_ms;
} fgi_sub_stats;
fgi_status fgi_sub_stats_get(fgi_graph* g, fgi_sub_stats* out);

/* ---- replica fan-out per rank of a partition (C-ABI 0.10) ------------------------------------------ */
/* The same subscriptions (RpcInboundComputeCall.cs:53-62, 102-106; ComputedExt.WhenInvalidated,
 * ComputedExt.cs:99-125) on a partitioned graph: each rank keeps the entries of the slots it owns and returns
 * its own share of a wave's fan-out in the host's numbering. Every call here is rank-local: none joins a
 * collective, and a rank may call them at any time and in any order, as fgi_part_last_wave_ids. On a graph
 * that is not partitioned they return FGI_ENOTSUP (use the call of the section above), on a poisoned graph
 * FGI_ESTATE. fgi_sub_stats_get reads a rank's table as it is. The contract is the section above's, per rank,
 * with these differences.
 * fgi_part_subscribe: slots are global ids in the host's numbering (partition codes are never visible). A slot
 * >= n_global or a peer >= FGI_MAX_PEERS returns FGI_EINVAL and stores nothing. A slot this rank does not own
 * gets FGI_SUB_NOT_OWNED and is not stored, so a host may hand every rank the same list or each rank its share.
 * An owned slot that is empty or Invalidated gets FGI_SUB_INVALIDATED; anything else is stored under the local
 * handle slot - rank * block and gets FGI_SUB_ADDED. The state is the node's as it stands after the rank's last
 * wave (its node word and visit bit, what the rank's state view reports): no fold, no pass over the graph, and
 * fgi_part_last_wave_ids / _bits and fgi_part_last_flagged answer as before the call. Detached handles cannot be
 * subscribed to: a partition addresses slots.
 * fgi_part_last_wave_fanout returns the entries of every owned slot the rank's last wave invalidated. It is
 * valid exactly where fgi_part_last_wave_ids is, until the rank's next call that runs a cascade or a fan-out,
 * or fgi_restore. slots[i] is the global slot whose invalidation released call_ids[i]; within a peer the order
 * is ascending slot. The lists are made once per wave: a second call returns the same arrays, and so does a
 * retry after FGI_ECAPACITY (*out_n holds the count; the entries have left the table). n_peers at or below a
 * stored peer id: FGI_EINVAL, nothing is removed. After fgi_part_begin_compute, fgi_part_set_output or
 * fgi_part_run_batch: FGI_ENOTSUP (pass their ids to fgi_part_fanout_ids). Before any wave and after
 * fgi_restore: FGI_OK with 0 entries. A rank whose share of the wave is empty launches nothing.
 * fgi_part_fanout_ids is the same join for a strictly ascending list of global slots (an entry >= n_global or a
 * list that does not ascend: FGI_EINVAL). Slots the rank does not own are skipped on the device, so one
 * cascade's share of fgi_part_run_batch's or fgi_part_local_run_batch's out_ids can be passed as it is. A short
 * cap returns FGI_ECAPACITY with *out_n set and removes nothing.
 * Entries follow the node: where fgi_part_begin_compute, directly or as a batch's step, hands out a detached
 * handle on the owner (out_detached[i] != FGI_NONE), the slot's entries move to that local detached handle and
 * never fire with the slot's next node. No partitioned cascade reaches a detached node (a partition's roots
 * are slots), so those entries leave in three ways only: through fgi_part_fanout_detached when the host ends
 * the displaced node itself (its delay timer, its own TrySetOutput) - handles: this rank's detached handles,
 * strictly ascending, within [n_slots, n_slots + n_detached), else FGI_EINVAL; handles_out[i] is the detached
 * handle that released call_ids[i] -, through fgi_release, which drops them (fgi_sub_stats.dropped), and
 * through fgi_part_unsubscribe_peer.
 * FGI_OPT_FANOUT_PATH on a partition: 1 the rank's ascending id list (made if absent), 2 the bitmap form (the
 * host-order bitmap if fgi_part_last_wave_bits made it; else, with partition codes, the wave's bitmap probed at
 * the subscribed handles only; else the wave's bitmap in place), 0 the list if the rank's ascending ids already
 * stand, else the bitmap form. 3 is for measurement: the bitmap form with the host-order bitmap made inside the
 * call (the gather or scatter of fgi_part_last_wave_bits), the form the probe replaces; on a single device it is
 * 2. Results never depend on it. */
#define FGI_SUB_NOT_OWNED 2u
fgi_status fgi_part_subscribe(fgi_graph* g, uint32_t n, const uint32_t* slot /*global*/, const uint32_t* peer,
                              const uint64_t* call_id, uint32_t* out_result /*nullable*/);
fgi_status fgi_part_last_wave_fanout(fgi_graph* g, uint32_t n_peers, uint64_t* peer_off /*n_peers+1*/,
                                     uint64_t* call_ids /*nullable*/, uint32_t* slots /*nullable*/,
                                     uint64_t cap, uint64_t* out_n);
fgi_status fgi_part_fanout_ids(fgi_graph* g, uint64_t n, const uint32_t* slots_in /*host, global, strictly ascending*/,
                               uint32_t n_peers, uint64_t* peer_off, uint64_t* call_ids, uint32_t* slots,
                               uint64_t cap, uint64_t* out_n);
fgi_status fgi_part_fanout_detached(fgi_graph* g, uint64_t n, const uint32_t* handles /*host, this rank's detached
                               local handles, strictly ascending*/, uint32_t n_peers, uint64_t* peer_off,
                               uint64_t* call_ids, uint32_t* handles_out, uint64_t cap, uint64_t* out_n);
fgi_status fgi_part_unsubscribe_peer(fgi_graph* g, uint32_t peer, uint64_t* out_dropped /*nullable*/);

/* ---- delayed invalidation: timers in device memory (C-ABI 0.11; timers.hip) ---------- */
/* A Consistent node with an InvalidationDelay that a cascade reaches only gets InvalidationDelayStarted
 * (Computed.cs:183-197) and then schedules its own timer, which later calls Invalidate(true)
 * (ComputedExt.cs:10-45, the Timeouts.Invalidate timer set). The engine keeps that timer set in device memory:
 * at most one entry (handle, version, due) per boundary handle, armed by kernels queued behind the calls that
 * flag nodes, fired by one call per clock tick. This section serves single-device graphs (a rank of a partition:
 * the next section), off until fgi_timers_open; a graph that never opens timers allocates and launches nothing
 * for any of this.
 * Clock: uint64_t ticks in a unit the host chooses; the engine only adds and compares. The graph holds `now`;
 * fgi_timers_set_now and fgi_timers_run_due advance it, a value below the current one is FGI_EINVAL and
 * changes nothing.
 * Delay (ComputedOptions.InvalidationDelay): a property of the handle, set by fgi_timers_set_delay, sticky for
 * a slot across recomputations. 0: the graph's default_delay. FGI_TIMER_NEVER: TimeSpan.MaxValue, the node is
 * flagged and no entry is ever stored (ComputedExt.cs:12). An effective delay of 0 stores nothing either. A
 * detached handle fgi_begin_compute (or a batch's BEGIN_COMPUTE step) hands out takes a copy of its slot's delay.
 * Arm rule, for a candidate handle h: the node now at h, its visit bit folded in as fgi_subscribe reads it, is
 * Consistent with InvalidationDelayStarted, and no entry (h, its version) exists: store (h, version,
 * due = now + delay(h)), saturating at FGI_TIMER_NEVER - 1. An entry of another version at h is overwritten
 * (counted as dropped and as armed); one of the same version keeps its earlier due time
 * (ConcurrentTimerSet.AddOrUpdateToEarlier). Candidates: the records of every flagged-set post-pass
 * (fgi_last_wave_flagged, fgi_wave_wait_flagged: armed by a kernel queued behind the post-pass, no wait, no
 * copy); the records of a batch's cascades, armed once behind the batch from the states the batch left; every
 * detached handle handed out.
 * Move: when a displaced node survives to detached handle d, an entry (slot, its version) moves to d with its
 * due time unchanged; without one the arm rule runs on d. A batch applies its moves behind itself, in step
 * order, before it arms its records. fgi_begin_compute arms its displacement cascade's records behind its install:
 * a displaced node that the cascade also reached along an edge is armed under d like any other displaced node
 * (not under its slot and then moved), so `moved` counts only entries that stood before the call.
 * Fire: fgi_timers_run_due(now) sets the clock, removes every entry with due <= now, and fires those whose
 * node still has the entry's version and is Consistent with InvalidationDelayStarted (the others are stale:
 * counted in dropped). The fired handles, ascending, are the roots of ONE wave with immediately = 1, run as
 * fgi_invalidate_dev runs one: fgi_last_wave_ids, fgi_wave_ids_dev, fgi_last_wave_flagged, fgi_last_wave_fanout,
 * the state view and the statistics follow it, and its own flagged set arms at `now`. out_ids / cap / out_n
 * follow fgi_invalidate's contract: a short cap returns FGI_ECAPACITY with *out_n set; the wave has run and
 * fgi_last_wave_ids returns its ids. *out_fired (nullable): entries fired. Nothing due: no wave, 0 ids, and the
 * last wave's results stay as they are.
 * Lazy removal: the entry of a node invalidated before its due time stays until it comes due or is
 * overwritten, so `stored` may include stale entries. fgi_release of a detached handle drops its entry;
 * fgi_restore drops all entries and keeps the clock and the delays; fgi_timers_open on a populated graph arms
 * every node already Consistent with InvalidationDelayStarted.
 * fgi_timers_next_due: the smallest due time stored (FGI_TIMER_NONE without entries), a reduction over the
 * entries. fgi_timers_list (diagnostics, tests): the stored entries ascending by handle; a short cap returns
 * FGI_ECAPACITY with *out_n set.
 * Counter identity, over a graph's life since fgi_timers_open: armed == fired + dropped + stored. `moved`
 * counts entries that changed handle (a move neither arms nor drops). runs: fgi_timers_run_due calls that
 * launched a wave. last_kernel_ms: device time of the last fgi_timers_run_due's own kernels (HIP events).
 * Memory: 8 bytes per handle (a delay code and an entry index) plus 48 bytes per possible entry: the entries
 * stored when fgi_timers_set_delay was last called (a slot set back to delay 0 keeps its entry until that
 * comes due), the slots with a delay of their own and the detached handles, at most every handle; or every
 * handle when default_delay is set. The pool does not shrink.
 * Before fgi_timers_open every other call here returns FGI_ESTATE and fgi_timers_stats_get returns zeros; on a
 * poisoned graph FGI_ESTATE; fgi_timers_open on a partitioned graph FGI_ENOTSUP (fgi_part_timers_open), and so do
 * fgi_timers_set_delay and fgi_timers_run_due there, whether or not the rank's timers are open (before 0.12 they
 * returned FGI_ESTATE on a rank, whose timers could not be open). */
#define FGI_TIMER_NEVER 0xFFFFFFFFFFFFFFFFull
#define FGI_TIMER_NONE 0xFFFFFFFFFFFFFFFFull /* fgi_timers_next_due: nothing stored */
typedef struct fgi_timers_config {
    uint32_t struct_size, reserved;
    uint64_t default_delay, now;
} fgi_timers_config;
typedef struct fgi_timer_stats {
    uint64_t stored, armed, fired, dropped, moved, runs;
    double last_kernel_ms;
} fgi_timer_stats;
fgi_status fgi_timers_open(fgi_graph* g, const fgi_timers_config* cfg);
fgi_status fgi_timers_close(fgi_graph* g);
fgi_status fgi_timers_set_delay(fgi_graph* g, uint32_t n, const uint32_t* handle, const uint64_t* delay);
fgi_status fgi_timers_set_now(fgi_graph* g, uint64_t now);
fgi_status fgi_timers_run_due(fgi_graph* g, uint64_t now, uint32_t* out_ids /*nullable*/, uint64_t cap,
                              uint64_t* out_n, uint64_t* out_fired /*nullable*/, fgi_wave_stats* stats /*nullable*/);
fgi_status fgi_timers_next_due(fgi_graph* g, uint64_t* out_due, uint64_t* out_stored /*nullable*/);
fgi_status fgi_timers_stats_get(fgi_graph* g, fgi_timer_stats* out);
fgi_status fgi_timers_list(fgi_graph* g, uint32_t* handle, uint64_t* version, uint64_t* due, uint64_t cap,
                           uint64_t* out_n);

/* ---- auto-invalidation timers: armed at TrySetOutput (C-ABI 0.13; timers.hip) ---------- */
/* The other half of the Timeouts.Invalidate timer set: a node that becomes Consistent schedules Invalidate(true)
 * after ComputedOptions.AutoInvalidationDelay, or after TransientErrorInvalidationDelay when its output is a
 * transient error (StartAutoInvalidation, Computed.cs:235-246, called by TrySetOutput, Computed.cs:158). Both go
 * through ComputedExt.Invalidate(TimeSpan) -> AddOrUpdateToEarlier (ComputedExt.cs:10-25), as the delay timers
 * of the section above do, so the entries share that section's pool, due pass and fire wave; an entry carries a
 * kind (bit 0: auto) beside (handle, version, due). These six calls serve a single device: on a partitioned
 * graph all of them return FGI_ENOTSUP, and a rank uses the fgi_part_* calls of the section "auto-invalidation
 * timers per rank of a partition" (C-ABI 0.14) below.
 * Opt-in: fgi_timers_auto_open needs open timers (FGI_ESTATE before fgi_timers_open, when already on, or on a
 * poisoned graph). Until it is called no call here allocates or launches anything: fgi_set_output,
 * fgi_set_output_ex and fgi_run_batch behave and launch exactly as before 0.13, fgi_timers_set_auto_delay and
 * fgi_timers_start_auto return FGI_ESTATE, fgi_timers_auto_stats_get returns zeros, fgi_timers_list_ex lists
 * every kind as 0. fgi_timers_close turns auto off too.
 * Delays: two per handle (auto, transient error), set by fgi_timers_set_auto_delay (a null array leaves that
 * delay as it is; a handle out of range or listed twice: FGI_EINVAL, nothing stored), sticky for a slot across
 * recomputations and copied onto a detached handle by the move, exactly as fgi_timers_set_delay's. 0: the
 * graph's default of that kind (fgi_timers_auto_config; 0 = none). FGI_TIMER_NEVER: none (TimeSpan.MaxValue,
 * Computed.cs:244, ComputedExt.cs:12). An effective delay of 0 or NEVER stores nothing. The reference's "delay <= 0 means
 * invalidate at once" (ComputedExt.cs:15-18) is NOT built: a host that wants it calls fgi_invalidate.
 * Candidates: an item of fgi_set_output / fgi_set_output_ex, or of a batch's SET_OUTPUT step, whose node went
 * Computing -> Consistent and did NOT carry InvalidateOnSetOutput (Computed.cs:153-156 returns before
 * StartAutoInvalidation; a node with an InvalidationDelay survives its own cascade as Consistent with
 * InvalidationDelayStarted and gets its delay entry only). fgi_set_output is fgi_set_output_ex with
 * transient == NULL; transient[i] != 0 marks item i's output as a transient error. A SET_OUTPUT step's flags
 * (nullable) are its items' transient flags, read only on a graph with auto open. fgi_timers_start_auto lists
 * candidates explicitly (handles in range and distinct, else FGI_EINVAL and nothing stored): for nodes
 * registered Consistent in bulk, whose TrySetOutput the engine never saw.
 * Auto arm rule, for candidate h, run by a kernel queued behind the call's cascade: the node now at h, its visit
 * bit folded in, is Consistent, and d = transient ? transient_delay(h) : auto_delay(h) is finite and non-zero:
 * store (h, version, due = now + d, saturating as above, kind = auto). An entry of another version at h is
 * overwritten (dropped + armed, as above). One of the same version takes due = min(stored, new) and the union
 * of the kinds, counted in `merged`, neither armed nor dropped (AddOrUpdateToEarlier, ComputedExt.cs:22).
 * Delay arm rule meeting an auto entry of the same version: due = min, the kind bit stays, counted in `merged`;
 * two delay arms of one version keep the stored due time, as before.
 * Fire: a due entry fires if its version matches and the node is Consistent and (InvalidationDelayStarted or
 * the entry is auto): the reference's timer calls Invalidate(true) on any live computed (ComputedExt.cs:35).
 * Everything after that is the section above's: one wave with immediately = 1, its flagged set arms at `now`,
 * and armed == fired + dropped + stored holds with auto entries included. fired_auto counts the fired entries
 * of kind auto, armed_auto the entries the auto arm rule stored (new or overwriting).
 * Move: a moved entry keeps its kind. Behind a moved auto entry the delay arm rule also runs on the detached
 * handle (min merge): the displacement's Invalidate() has just set InvalidationDelayStarted on the surviving
 * node, and the reference adds its delay timer to the auto one and keeps the earlier
 * (ComputedRegistry.cs:91-96 -> Computed.cs:186-197).
 * Batches: behind the batch the steps are walked in order: a SET_OUTPUT step auto-arms, a BEGIN_COMPUTE step
 * applies its moves; then the batch's flagged records arm once, as before. A SET_OUTPUT item's candidate handle
 * is where that node lives when the batch ends: the item's handle, or the detached handle of the first later
 * BEGIN_COMPUTE step on its slot, or nothing if that step's out is FGI_NONE; its delays are the item's own
 * handle's. The arm rule reads end-of-batch states, so a node the batch later invalidated is not Consistent and
 * gets no entry. A step's `out` stays 0 / 1.
 * Memory: 8 more bytes per handle. The pool bound counts a handle with an auto or transient code of its own as
 * a holder, and every handle when a default of either kind is set; still at most one entry per handle.
 * fgi_restore, fgi_release, lazy removal, fgi_timers_next_due, fgi_timers_list (which omits the kind) and
 * fgi_timers_stats_get behave as in the section above; fgi_restore keeps the auto delays and counters. */
typedef struct fgi_timers_auto_config {
    uint32_t struct_size, reserved;
    uint64_t default_auto_delay, default_transient_delay; /* 0 = none */
} fgi_timers_auto_config;
typedef struct fgi_timer_auto_stats {
    uint64_t armed_auto, merged, fired_auto;
} fgi_timer_auto_stats;
fgi_status fgi_timers_auto_open(fgi_graph* g, const fgi_timers_auto_config* cfg);
fgi_status fgi_timers_set_auto_delay(fgi_graph* g, uint32_t n, const uint32_t* handle,
                                     const uint64_t* auto_delay /*nullable*/, const uint64_t* transient_delay /*nullable*/);
fgi_status fgi_set_output_ex(fgi_graph* g, uint32_t n, const uint32_t* handle, const uint8_t* transient /*nullable*/,
                             uint8_t* out_set, uint32_t* out_ids, uint64_t cap, uint64_t* out_n, fgi_wave_stats* stats);
fgi_status fgi_timers_start_auto(fgi_graph* g, uint32_t n, const uint32_t* handle, const uint8_t* transient /*nullable*/);
fgi_status fgi_timers_auto_stats_get(fgi_graph* g, fgi_timer_auto_stats* out);
fgi_status fgi_timers_list_ex(fgi_graph* g, uint32_t* handle, uint64_t* version, uint64_t* due,
                              uint8_t* kind /*bit 0: auto*/, uint64_t cap, uint64_t* out_n);

/* ---- delay timers per rank of a partition (C-ABI 0.12; timers.hip) -------------------- */
/* The same timers on a partitioned graph: each rank keeps the entries of its own local handles in its own
 * device memory, arms them behind its own share of every cascade, and a clock tick is ONE collective call whose
 * due entries, from all ranks, become the roots of one partitioned wave. A partition that never opens timers
 * allocates and launches nothing for this. The contract is the section above's, per rank, with these differences.
 * The table: a rank's table covers its local handles, addressed as fgi_dump_states and the rank's state view
 * address them: h < n_slots is global slot rank * block + h in the host's numbering (partition codes are never
 * visible), the rank's detached handles follow; the handles [n_local, n_slots) of a short last rank never hold
 * a node and never an entry. The state read is the node word with the rank's visit bit folded in, as
 * fgi_part_subscribe reads it: no fold, no pass over the graph.
 * fgi_part_timers_open: rank-local, no collective. FGI_ENOTSUP on a graph that is not partitioned (use
 * fgi_timers_open), FGI_ESTATE on a poisoned graph or with the timers already open. On a populated rank it arms
 * every handle whose node is already Consistent with InvalidationDelayStarted.
 * fgi_part_timers_set_delay: rank-local; slots are global ids. A slot >= n_global or a slot listed twice is
 * FGI_EINVAL and nothing is stored. A slot the rank does not own is skipped, so a host may hand every rank the
 * same list or each rank its share, as with fgi_part_subscribe. A detached handle takes its slot's delay by
 * the move, as above.
 * fgi_timers_close, fgi_timers_set_now, fgi_timers_next_due, fgi_timers_stats_get and fgi_timers_list take no
 * slot arguments and serve a rank's table as they are (fgi_timers_list returns local handles; a host takes the
 * minimum of the ranks' next_due). fgi_timers_set_delay and fgi_timers_run_due return FGI_ENOTSUP on a
 * partitioned graph: use the calls of this section.
 * Arming: every fgi_part_* call that runs cascades arms once, behind its last cascade and its moves, with a
 * kernel queued on the rank's stream: fgi_part_invalidate, _host, _bits and _all, each rank of
 * fgi_part_local_invalidate, fgi_part_begin_compute, fgi_part_set_output, and fgi_part_run_batch once for the
 * whole batch (also when a later step is refused after earlier ones were applied). The candidates are the
 * rank's records of the call (what fgi_part_last_flagged returns), counted on the device; the arm rule runs on
 * the states the call left. Nothing waits and nothing is copied: a wave's host_syncs are what they are without
 * timers. A call that runs no cascade arms nothing.
 * Moves and drops: fgi_part_begin_compute, directly or as a batch's step, moves the entry of an owned slot to the
 * detached handle it hands out (or arms it there), beside the subscriptions' move. fgi_release drops a detached
 * handle's entry; fgi_restore drops every entry of the rank and keeps its clock and delays.
 * Firing, fgi_part_timers_run_due(now): collective, every rank calls it with the same `now`.
 *  - Agreement first. Each rank's verdict (timers open, graph not poisoned, now >= its clock) and its `now` travel
 *    with the call's first collective. If any rank refuses or the `now` values differ, every rank returns the
 *    same status, FGI_ESTATE for a refusing rank, FGI_EINVAL for a clock or `now` problem, fgi_last_error names
 *    the rank, no rank removes an entry and nothing runs.
 *  - The due pass runs on each rank's own pool (a rank with an empty pool launches nothing but joins the
 *    collectives): it removes what is due, drops what went stale and separates the fired handles into owned
 *    slots and detached handles.
 *  - The fired slots of all ranks, as global ids, are gathered in rank order: the ascending root list, identical
 *    on every rank. If it is empty no wave runs and every rank's last-wave results stay as they are. Otherwise
 *    ONE partitioned wave runs with immediately = 1, driven as fgi_part_invalidate drives one:
 *    fgi_part_last_wave_ids, _bits, fgi_part_wave_ids_dev, fgi_part_last_flagged, fgi_part_last_wave_fanout, the
 *    rank's state view and the statistics follow it, and its own flagged set arms at `now`, so timers cascade.
 *    out_ids / cap / out_n follow fgi_part_invalidate_host's contract (this rank's ids, ascending; a short cap:
 *    FGI_ECAPACITY with *out_n set, the wave has run and fgi_part_last_wave_ids returns the list).
 *  - *out_fired (nullable) counts this rank's fired entries, slots and detached handles. fgi_timer_stats.runs
 *    counts the calls that launched a wave and is the same on every rank.
 *  - Detached handles: no partitioned cascade reaches a detached node (the section on the fan-out per rank), so
 *    a due entry on a detached handle that passes the fire test is removed, counted in `fired` and reported, not
 *    cascaded; the engine does not change the node word. *out_fired_detached (nullable) is this rank's count and
 *    fgi_part_timers_fired_detached returns them: this rank's local detached handles, ascending, valid until
 *    the rank's next fgi_part_timers_run_due, fgi_restore or fgi_timers_close. A second call returns the same
 *    list; a short cap returns FGI_ECAPACITY with *out_n set and loses nothing. The host ends that node itself,
 *    as it does for the fan-out (fgi_part_fanout_detached, then fgi_release).
 * fgi_part_local_timers_run_due runs the call on every rank of an in-process group, one host thread per rank
 * (out_fired, out_fired_detached, stats: p entries each, nullable); ids are then read per rank with
 * fgi_part_last_wave_ids. */
fgi_status fgi_part_timers_open(fgi_graph* g, const fgi_timers_config* cfg);
fgi_status fgi_part_timers_set_delay(fgi_graph* g, uint32_t n, const uint32_t* slot /*global*/, const uint64_t* delay);
fgi_status fgi_part_timers_run_due(fgi_graph* g, uint64_t now, uint32_t* out_ids /*nullable*/, uint64_t cap,
                                   uint64_t* out_n, uint64_t* out_fired /*nullable*/,
                                   uint64_t* out_fired_detached /*nullable*/, fgi_wave_stats* stats /*nullable*/);
fgi_status fgi_part_timers_fired_detached(fgi_graph* g, uint32_t* out_handles /*nullable*/, uint64_t cap,
                                          uint64_t* out_n);
fgi_status fgi_part_local_timers_run_due(fgi_graph* const* gs, uint32_t p, uint64_t now,
                                         uint64_t* out_fired /*p, nullable*/, uint64_t* out_fired_detached /*p, nullable*/,
                                         fgi_wave_stats* stats /*p, nullable*/);

/* ---- auto-invalidation timers per rank of a partition (C-ABI 0.14; timers.hip) ---------- */
/* The auto-invalidation timers of the 0.13 section on a partitioned graph: each call is the 0.13 call per rank,
 * on the rank's own table (the 0.12 section: local handles, h < n_slots is global slot rank * block + h), with
 * slot arguments as global ids in the host's numbering; partition codes are never visible. The 0.13 names keep
 * returning FGI_ENOTSUP on a partitioned graph, and the calls of this section return FGI_ENOTSUP on a graph that
 * is not partitioned. The 0.13 section's rules (delays, candidates, the auto arm rule, the min merge, the fire
 * rule, the move, the counters) apply per rank, with these differences.
 * Opt-in, per rank: fgi_part_timers_auto_open needs the rank's timers open (FGI_ESTATE before
 * fgi_part_timers_open, when auto is already on, or on a poisoned graph). Until it is called the rank allocates
 * and launches nothing for this: fgi_part_set_output, fgi_part_set_output_ex and fgi_part_run_batch behave and
 * launch exactly as before 0.14 whatever transient flags they are given, fgi_part_timers_set_auto_delay and
 * fgi_part_timers_start_auto return FGI_ESTATE, fgi_part_timers_auto_stats_get returns zeros and
 * fgi_part_timers_list_ex lists every kind as 0. fgi_timers_close turns a rank's auto off too.
 * Rank-local calls: fgi_part_timers_auto_open, _set_auto_delay, _start_auto, _auto_stats_get and _list_ex use no
 * collective. A slot >= n_global or a slot listed twice is FGI_EINVAL and nothing is stored. A slot the rank does
 * not own is skipped, and the transient flag of a skipped item with it, so a host may hand every rank the same
 * list, as with fgi_part_timers_set_delay. fgi_part_timers_list_ex returns local handles, as fgi_timers_list does
 * on a rank.
 * fgi_part_set_output_ex is collective, as fgi_part_set_output is, which is fgi_part_set_output_ex with
 * transient == NULL. Candidates: the owned items whose node went Computing -> Consistent without
 * InvalidateOnSetOutput. The auto arm rule runs in a kernel queued on the rank's stream behind the call's cascade
 * and before the call's delay arm (the 0.12 section). It adds no wait and no copy back:
 * fgi_wave_stats.host_syncs is what it is with auto closed. The transient flags are read only on a rank with
 * auto open.
 * Batches (fgi_part_run_batch, fgi_part_local_run_batch): a SET_OUTPUT step's flags (nullable) are its items'
 * transient flags, read only on a rank with auto open. A partition applies a batch step by step, and the step
 * auto-arms behind its own cascade, on the states that step left, at the item's own slot. If a later
 * BEGIN_COMPUTE step of the same batch displaces the node, that step's move carries the entry to the detached
 * handle, kind included, and the delay arm rule then runs there with the min merge, as for any displacement. The
 * batch's flagged records still arm once behind the whole batch. THIS DIFFERS from the single-device batch of
 * 0.13, which resolves every SET_OUTPUT item to the handle where its node lives when the batch ends and reads
 * end-of-batch states: here a node that a later step of the same batch invalidates keeps a stale entry until the
 * entry comes due, and is then counted in `dropped`. armed == fired + dropped + stored holds either way.
 * Firing: fgi_part_timers_run_due is unchanged in shape. A due entry fires if its version matches and its node
 * is Consistent and (InvalidationDelayStarted or the entry is auto). An auto entry on an owned slot becomes a
 * root of the tick's wave; one on a detached handle is reported through fgi_part_timers_fired_detached, not
 * cascaded. fired_auto counts both.
 * Other calls: fgi_restore drops the rank's entries and keeps its auto delays and counters; fgi_release drops a
 * detached handle's entry; fgi_timers_next_due, fgi_timers_stats_get and fgi_timers_list serve the rank as in
 * the 0.12 section.
 * Memory: 8 more bytes per local handle. The pool bound is the 0.13 section's with every term the rank's own: a
 * slot with an auto or transient code counts only on the rank that owns it (no other rank stores the code). */
fgi_status fgi_part_timers_auto_open(fgi_graph* g, const fgi_timers_auto_config* cfg);
fgi_status fgi_part_timers_set_auto_delay(fgi_graph* g, uint32_t n, const uint32_t* slot /*global*/,
                                          const uint64_t* auto_delay /*nullable*/, const uint64_t* transient_delay /*nullable*/);
fgi_status fgi_part_set_output_ex(fgi_graph* g, uint32_t n, const uint32_t* slot, const uint8_t* transient /*nullable*/,
                                  uint8_t* out_set, uint32_t* out_ids, uint64_t cap, uint64_t* out_n, fgi_wave_stats* stats);
fgi_status fgi_part_timers_start_auto(fgi_graph* g, uint32_t n, const uint32_t* slot /*global*/,
                                      const uint8_t* transient /*nullable*/);
fgi_status fgi_part_timers_auto_stats_get(fgi_graph* g, fgi_timer_auto_stats* out);
fgi_status fgi_part_timers_list_ex(fgi_graph* g, uint32_t* handle /*local*/, uint64_t* version, uint64_t* due,
                                   uint8_t* kind /*bit 0: auto*/, uint64_t cap, uint64_t* out_n);

/* ---- streaming batches (BASELINE.json configs[4]) ------------------------------- */
/* One step of a batch: the arguments of the matching single call. */
#define FGI_STEP_INVALIDATE 1     /* fgi_invalidate: handles, flags = immediately (nullable) */
#define FGI_STEP_BEGIN_COMPUTE 2  /* fgi_begin_compute: handles = slots, version, flags = has_delay (nullable) */
#define FGI_STEP_ADD_USED 3       /* fgi_add_used: handles = dependants, used */
#define FGI_STEP_SET_OUTPUT 4     /* fgi_set_output: handles */
typedef struct fgi_step {
    uint32_t kind;
    uint32_t n;
    const uint32_t* handles;
    const uint32_t* used;
    const uint64_t* version;
    const uint8_t* flags;
    void* out;   /* nullable: BEGIN_COMPUTE uint32_t detached[n]; ADD_USED uint32_t result[n];
                    SET_OUTPUT uint8_t set[n] */
} fgi_step;

typedef struct fgi_batch_stats {
    uint64_t waves;        /* cascade waves run (steps with a non-empty root set count; empty ones too) */
    uint64_t levels;       /* BFS levels with a non-empty frontier, summed over the waves */
    uint64_t v_inv;        /* Consistent -> Invalidated transitions, summed over the waves */
    uint64_t e_trav;
    uint64_t e_match;
    uint64_t n_flagged;
    double kernel_ms;      /* device time from the batch's first launch to its last (HIP events) */
    double wave_ms;        /* of which the cascades' one-launch waves (HIP events) */
    double total_ms;       /* wall time of the call */
    uint32_t host_syncs;   /* times the call waited for the device */
    uint32_t pad;
} fgi_batch_stats;

/* A host layer's batch of compute-method work in one call: the steps are applied in order, each
 * exactly as the matching single call would apply it (fgi_invalidate, fgi_begin_compute — its
 * displacement cascade included —, fgi_add_used, fgi_set_output — its InvalidateOnSetOutput cascade
 * included; Computed.cs:141-230, 347-385, ComputedRegistry.cs:83-97), but every count stays on the
 * device and each cascade runs as one launch (one block per CU, grid barriers between its levels): the
 * call uploads the batch once and waits for the device once (once more if an add_used step must grow
 * the edge pool, and once more to copy out_ids). out_ids gets the handles invalidated by the batch's
 * cascades, cascade after cascade (each in ascending order); FGI_ECAPACITY with *out_n = the count if
 * cap is too small. If the batch runs out of detached handles, FGI_ECAPACITY names the step: the
 * steps before it are applied, it and the later ones are not. FGI_EINVAL (a bad argument in any step)
 * applies nothing.
 * FGI_EDEVICE if a cascade's grid barrier timed out (blocks of one cascade's grid were not resident
 * together, e.g. other work held the device). The batch is then half-applied: the steps before the
 * failed cascade are, the cascade may have been partly folded into node words, the later steps are
 * not. The graph is poisoned: every later call but fgi_restore, fgi_destroy, fgi_last_error and
 * fgi_set_option returns FGI_ESTATE until fgi_restore brings back the last snapshot (node words, rows,
 * detached handles); without a snapshot, only fgi_destroy remains. This mirrors the reference's
 * "Invalidate never throws" (Computed.cs:200-229) as far as a device fault allows: the failure is
 * reported once and nothing later runs on an undefined registry. */
fgi_status fgi_run_batch(fgi_graph* g, uint32_t n_steps, const fgi_step* steps, uint32_t* out_ids, uint64_t cap,
                         uint64_t* out_n, fgi_batch_stats* stats);
/* The flagged sets of the last fgi_run_batch, cascade after cascade (steps of kind INVALIDATE,
 * BEGIN_COMPUTE, SET_OUTPUT, in step order): out_step[i] = index of the step whose cascade flagged
 * out_ids[i]; within a step ascending boundary handles (detached ones included); out_flags[i] = the
 * node's canonical state_flags right after that cascade.
 * The flagged set of a cascade is fgi_last_wave_flagged's, per cascade: every handle whose canonical
 * state_flags gained FGI_F_INVALIDATE_ON_SET_OUTPUT and / or FGI_F_INVALIDATION_DELAY_STARTED during that
 * cascade and that the cascade did not invalidate, whatever the visit order. A handle may appear under
 * more than one step (a Computing node a cascade reaches in step 0 gains InvalidateOnSetOutput; an
 * `immediately` root on it in step 2 adds InvalidationDelayStarted). A begin_compute step's own slots are
 * not listed under that step (fgi_last_wave_flagged's rule: the displaced node that survives is the
 * step's out[i]).
 * Slot reuse: a record names the node that lived at the handle when its cascade ended. If a later step of
 * the same batch begins a computation on that slot, that node lives on at that step's out[i] detached
 * handle, or is gone if out[i] is FGI_NONE; the host that starts timers from the records follows it there.
 * out_step and out_flags are nullable; out_ids NULL = count only; FGI_ECAPACITY with *out_n set if cap is
 * short. The batch itself copies nothing for this: the records stay on the device and the first call after
 * the batch copies them (one device-to-host copy, one wait). Valid until the next call that runs a wave or
 * a batch, or fgi_restore. After a batch that failed with FGI_ECAPACITY at step k (out of detached
 * handles): the cascades of the steps before k. FGI_ENOTSUP if the last call that ran cascades was not
 * fgi_run_batch, and on a partitioned graph (fgi_part_run_batch reports through fgi_part_last_flagged);
 * FGI_ESTATE on a poisoned graph. A graph that never held a
 * Computing node or one with hasDelay reports empty sets at no cost: its batches allocate and launch
 * nothing for them (the records take 16 bytes of device memory per handle otherwise). */
fgi_status fgi_last_batch_flagged(fgi_graph* g, uint32_t* out_step, uint32_t* out_ids, uint32_t* out_flags,
                                  uint64_t cap, uint64_t* out_n);

/* ---- graph maintenance ---------------------------------------------------------------------- */
/* One ComputedGraphPruner pass (Internal/ComputedGraphPruner.cs:79-94): PruneUsedBy on every
 * registered Consistent node (Computed.cs:400-419) — keep (slot, tag) iff the slot's current node
 * exists with version == tag — then compact the edge pool. While no mutation and no compaction has
 * happened since the pull dependency lists were built, the version half of that test is read from the
 * liveness the list build recorded per pool entry, and only "current" from a bitmap of the node words
 * (same result, no per-entry gather of the dependant's node word). */
fgi_status fgi_prune(fgi_graph* g, fgi_prune_stats* stats);
/* The same PruneUsedBy pass over the rows of handles [first, first + count) only (one batch of
 * ComputedGraphPruner's walk, ComputedGraphPruner.cs:79-94). Rows are compacted in place: their
 * offsets and capacities stay, the freed entries become slack the rows grow into. fgi_prune visits
 * every row and, when holes exceed FGI_OPT_DEFRAG_PCT of the pool, copies the rows to a fresh pool
 * (each with max(4, len / 8) slack). */
fgi_status fgi_prune_range(fgi_graph* g, uint32_t first, uint32_t count, fgi_prune_stats* stats);
/* Incremental pruning: the next `batch` handles after the previous step's (wrapping around), but
 * only while the engine's estimate of stale entries exceeds stale_pct of the pool (waves add the
 * entries they make stale: the rows of invalidated nodes and the entries pointing at them);
 * otherwise returns at once with zero counts. */
fgi_status fgi_prune_step(fgi_graph* g, uint32_t batch, uint32_t stale_pct, fgi_prune_stats* stats);
/* Release a detached handle once the host no longer references the node. */
fgi_status fgi_release(fgi_graph* g, uint32_t n, const uint32_t* handle);

/* ---- bench / test support ------------------------------------------------------------------- */
/* Save / restore node states and row lengths on the device (reset from a pristine copy).
 * fgi_restore is stream-ordered: it may return before the device copies finish; every later call
 * on the graph runs after them. On a poisoned graph (a failed fgi_run_batch, FGI_EDEVICE) fgi_restore
 * copies back every saved table, clears the wave bitmaps and the detached-handle list to the
 * snapshot's, and makes the graph usable again. fgi_restore refuses (FGI_ESTATE) once the edge pool
 * was rebuilt or rows were compacted since the snapshot (a bulk load, fgi_prune / fgi_prune_range that
 * moved entries, a defragmentation): a poisoned graph then stays poisoned, and fgi_destroy is all that
 * is left for it — take a new snapshot after such a call. */
fgi_status fgi_snapshot(fgi_graph* g);
fgi_status fgi_restore(fgi_graph* g);
/* Device-side synthetic workloads. All nodes Consistent with
 * version (splitmix64(seed ^ slot) & (2^55-1)) | 1. stale_pct% of edges (by hash with
 * stale_seed) carry tag = version + 1. The graph must be empty. */
fgi_status fgi_synth_layered(fgi_graph* g, uint32_t levels, uint32_t width, uint32_t fanout, uint64_t seed);
fgi_status fgi_synth_rmat(fgi_graph* g, uint32_t scale, uint32_t edge_factor, uint64_t seed,
                          uint32_t stale_pct, uint64_t stale_seed);
/* Copy the full edge set (sorted by (used, dependant, tag)) to the host: parity tests. */
fgi_status fgi_export_edges(fgi_graph* g, uint32_t* used, uint32_t* dependant_slot, uint64_t* tag,
                            uint64_t cap, uint64_t* out_n);
/* HIP stream the graph's kernels run on (as void* = hipStream_t) — for event timing in bench. */
fgi_status fgi_stream(fgi_graph* g, void** stream);
/* Traversal options (defaults in brackets). Results never depend on them; they exist so tests can
 * pin each code path and benches can compare them.
 *   FGI_OPT_DEAD_FILTER [1]  skip edges whose dependant was invalidated in an earlier level using
 *                            a per-wave bitmap (E_match then counts examined edges only). The bitmap is
 *                            read without synchronisation, so an edge whose dependant another lane
 *                            visits in the same level is examined or skipped as the lanes happen to
 *                            run: with the filter on, e_match of a wave whose levels reach a node along
 *                            several edges may differ between two runs of the same wave (every other
 *                            count and every result is the same). 0 makes e_match exact and repeatable
 *   FGI_OPT_DIRECTION   [0]  0 auto (push/pull per level), 1 push only, 2 pull only
 *   FGI_OPT_PULL_ALPHA  [28] auto: pull when frontier edges > total edges / alpha
 *   FGI_OPT_PULL_BETA   [32] auto: after a pull level, pull again while the frontier holds more
 *                            than n_slots / beta nodes (0: the alpha rule only)
 *   FGI_OPT_LEVEL_TIMING [1] with a stats argument, time every level's traversal launch with HIP
 *                            events (per-kernel figures for the roofline); 0 keeps only the
 *                            wave-boundary events, so measured waves carry no per-level markers
 *   FGI_OPT_DEFRAG_PCT  [60] fgi_prune copies the rows to a fresh pool when holes exceed this % of
 *                            it (0: never)
 *   FGI_OPT_PULL_TPB    [0]  pull tiles (1,024 slots) per block, 1..32; 0 sizes the grid from the CU
 *                            count (measurement / tests: results never depend on it)
 *   FGI_OPT_PART_COLLECTIVES [0] a one-rank partition skips its collectives (identities there);
 *                            1 runs them anyway (tests of the RCCL level loop on one GPU)
 *   FGI_OPT_FRONT_EXCHANGE [0] partitions, before a pull level: 0 per level whichever moves fewer
 *                            bytes, 1 all-gather of the whole invalidated bitmap, 2 only the words
 *                            that changed since the previous exchange (8 B each, to every rank);
 *                            all ranks of a partition must set the same value
 *   FGI_OPT_HOT_HEADS   [0]  most list heads a pull level probes through the hot snapshot: 0 sizes
 *                            it from the graph (65,536-262,144); n > 0 caps it at n rounded up to 256,
 *                            so the other heads are probed in the invalidated bitmap itself (tests pin
 *                            that path on small graphs; results never depend on it)
 *   FGI_OPT_PART_PLAN   [1]  partitions: a wave follows the previous wave's directions (when every
 *                            rank can) and queues all its levels' collectives at fixed sizes, with one
 *                            host synchronisation at its end (two with remote ranks: the start's
 *                            all-reduce too); 0 decides every level on the host after an all-reduce.
 *                            All ranks must set the same value
 *   FGI_OPT_PART_BUCKET [0]  partitions, planned waves: words per peer of a push level's bucket (a
 *                            count, then ids; 0 = the allocated 65,536); smaller buckets only delay
 *                            ids to later push levels (tests pin that path; results never change)
 *   FGI_OPT_FAULT_INJECT [0] tests only: value (k << 16) | b, b > 0: in the (k+1)-th streaming
 *                            cascade launched from now (fgi_run_batch), block b - 1 leaves at its first
 *                            grid barrier without arriving, and that cascade's barrier times out after
 *                            20 ms: the failure path runs deterministically (FGI_EDEVICE, then the
 *                            poisoned graph)
 *   FGI_OPT_FAULT_INJECT_TAIL [0] tests only: the same for the (k+1)-th wave tail (the persistent
 *                            launch that runs a wave's last small push levels, synchronous or
 *                            asynchronous waves): fgi_invalidate* / fgi_wave_wait return FGI_EDEVICE and
 *                            the graph is poisoned until fgi_restore
 *   FGI_OPT_PART_VIEW_PATH [0] partitions with codes and a state view open (fgi_part_state_view_open):
 *                            how a wave's invalidated set reaches the planes: 0 by the wave's size (gather
 *                            from n_local / 16 invalidated handles on), 1 scatter, 2 gather. Results never
 *                            depend on it (tests pin both paths on small graphs).
 *   FGI_OPT_PART_IDS_PATH  [0] partitions with codes: how fgi_part_last_wave_ids / _bits bring a wave's
 *                            invalidated set into the host's numbering: 0 by the wave's size, 1 scatter
 *                            from the wave's list, 2 gather per bitmap word. Results never
 *                            depend on it (tests pin both paths); setting it makes the last wave's result
 *                            again on the next call.
 *   FGI_OPT_FANOUT_PATH [0]  which form of the invalidated set a fan-out joins with the subscriptions: 0 by what
 *                            the wave left (its kept bitmap, else its id list), 1 the id list, 2 the bitmap
 *                            (made from the list if the wave kept none). Results never depend on it (tests pin
 *                            both paths). On a partition: the fgi_part_* section; 3 there is a measurement form.
 *   FGI_OPT_RUN_OFFSET_BITS [28] tests only: a pull candidate's record names its tail run by an offset
 *                            below 2^bits words from its pull block's base; a candidate past that is
 *                            found through the per-slot list offsets instead (tests pin that path on
 *                            small graphs with 1..27; results never depend on it) */
#define FGI_OPT_DEAD_FILTER 1
#define FGI_OPT_DIRECTION 2
#define FGI_OPT_PULL_ALPHA 3
#define FGI_OPT_LEVEL_TIMING 4
#define FGI_OPT_PULL_BETA 5
#define FGI_OPT_DEFRAG_PCT 6
#define FGI_OPT_PART_COLLECTIVES 7
#define FGI_OPT_PULL_TPB 8
#define FGI_OPT_FRONT_EXCHANGE 9
#define FGI_OPT_HOT_HEADS 10
#define FGI_OPT_FAULT_INJECT 11
#define FGI_OPT_PART_PLAN 13
#define FGI_OPT_PART_BUCKET 14
#define FGI_OPT_FAULT_INJECT_TAIL 16
#define FGI_OPT_RUN_OFFSET_BITS 17
#define FGI_OPT_PART_VIEW_PATH 18
#define FGI_OPT_PART_IDS_PATH 19
#define FGI_OPT_FANOUT_PATH 20
/* 12 and 15: the measurement variants' options (include/fgi_variants.h); FGI_ENOTSUP here */
fgi_status fgi_set_option(fgi_graph* g, int option, int64_t value);

/* ---- multi-GPU (1-D vertex-range partition, RCCL all-to-all frontier exchange) --------------- */
/* RCCL unique id (128 bytes) made by rank 0 and broadcast by the caller (e.g. torch.distributed). */
fgi_status fgi_part_unique_id(uint8_t* id128);
/* Join the partitioned engine: this graph owns slots [rank*ceil(N/world), ...) of a global
 * N = n_global slots; cfg->rank/world must be set. */
fgi_status fgi_part_init(fgi_graph* g, uint32_t n_global, const uint8_t* id128);
/* Join the partitioned engine with the host's own transport instead of RCCL: every collective of the
 * partition (the waves' exchanges, the mutations' all-reduces, the prune's all-gather) reduces to
 * fn(ctx, send, bytes, recv) — an all-gather of `bytes` from every rank into recv (world * bytes,
 * rank-major; 0 = success), e.g. torch.distributed over gloo. The ranks may then share a GPU (RCCL
 * refuses two ranks on one device): the multi-process path runs on any box. Every collective
 * synchronises the rank's stream (correct, not fast). Same results as fgi_part_init's. */
typedef int (*fgi_allgather_fn)(void* ctx, const void* send, uint64_t bytes, void* recv);
fgi_status fgi_part_init_host(fgi_graph* g, uint32_t n_global, fgi_allgather_fn fn, void* ctx);
/* Partitioned R-MAT: every rank walks the global edge sequence by index (edge i is a pure function of
 * i) and keeps only its share — the rows of its slots and the dependency entries of its slots —
 * without materialising the global edge list. */
fgi_status fgi_part_synth_rmat(fgi_graph* g, uint32_t scale, uint32_t edge_factor, uint64_t seed,
                               uint32_t stale_pct, uint64_t stale_seed);
/* Bulk import into a partitioned graph (ComputedRegistry.Register, ComputedRegistry.cs:72-105, without
 * displacement; the single-device fgi_register_nodes refuses a partition). The replicated form: every
 * rank is given the same global node list (a host that holds the whole registry in every process; one
 * that holds a shard per process calls fgi_part_register_shard instead): each rank installs the nodes
 * of the slots it owns and records every listed version in its replica (ver_all), against which it
 * checks the tags of edges into other ranks' slots. No collective runs. */
fgi_status fgi_part_register_nodes(fgi_graph* g, uint32_t n, const uint32_t* slot, const uint64_t* version,
                                   const uint32_t* state_flags);
/* Bulk import of `_usedBy` entries with global ids (IComputedImpl.AddUsedBy body, Computed.cs:381-382;
 * set semantics). The replicated form (fgi_part_load_edges_shard takes a shard per rank instead and
 * cannot number the slots differently): every rank is given the same batch. It keeps the rows of the
 * `used` slots it owns
 * (entries keep global dependant ids) and the dependency entries of the dependants it owns, from
 * which it rebuilds its pull lists (the reference's `_used`, Computed.cs:36, 365-366). No collective
 * runs. The first bulk load of a partition that uses partition codes (labels: automatic from 2^25
 * slots, fgi_config.labels = 1 forces them) also numbers every rank's slots by weight, each rank on
 * its own from the arrays it was given; ranks given different arrays number them differently, and
 * the next collective wave then fails on every rank with FGI_ESTATE. */
fgi_status fgi_part_load_edges(fgi_graph* g, uint64_t m, const uint32_t* used, const uint32_t* dependant,
                               const uint64_t* tag);
/* The same imports from per-rank shards (C-ABI 0.5; ComputedRegistry.Register, ComputedRegistry.cs:72-105,
 * and the AddUsedBy body, Computed.cs:381-382, with global ids). Collective: every rank joins every call and
 * passes ITS OWN shard — any nodes / edges, whoever owns them, possibly none (n / m = 0 with null arrays).
 * The engine routes them to their owners over the partition's transport. With A the concatenation of the
 * ranks' shards in rank order, every rank is left in the state fgi_part_register_nodes / fgi_part_load_edges
 * given A on every rank would have left: owned node words, the version replica, rows and dependency entries
 * (set semantics across shards and across earlier loads), list weights and pull lists, the flag gate of the
 * flagged sets, and the partition codes if this is the first bulk load of a partition that wants them (every
 * rank then holds the same weights by construction, so the ranks cannot number the slots differently).
 * Sharded and replicated calls may be mixed on one partition, in any order.
 * Errors strand no peer: each rank checks its own shard (slot range, version <= 2^56-1, state != 3, tag != 0)
 * and its verdict travels with the call's first collective, the counts; if any rank's shard is bad every rank
 * returns FGI_EINVAL, nothing is applied and fgi_last_error names the rank and the item. A listed slot that
 * already holds a current node — a slot listed in two shards included — fails fgi_part_register_shard with
 * FGI_ESTATE on every rank (the owners' counts are all-reduced). FGI_ESTATE on a graph that is not
 * partitioned or is poisoned; FGI_EDEVICE naming the rank and the collective when a peer is lost.
 * Buffers: one round per call. A rank stages 2 x 16 bytes per edge of its shard for sending (beside the
 * 16-byte upload of the edge itself) plus 16 bytes per record it receives (two per edge whose ends it owns).
 * A host that wants less peak memory calls several times with smaller shards: set semantics hold across calls.
 * fgi_part_local_register_shards / fgi_part_local_load_shards run the same on every rank of an in-process
 * group (fgi_part_init_local), one host thread per rank: entry r of each array is rank r's shard. */
fgi_status fgi_part_register_shard(fgi_graph* g, uint32_t n, const uint32_t* slot, const uint64_t* version,
                                   const uint32_t* state_flags /*nullable*/);
fgi_status fgi_part_load_edges_shard(fgi_graph* g, uint64_t m, const uint32_t* used, const uint32_t* dependant,
                                     const uint64_t* tag);
fgi_status fgi_part_local_register_shards(fgi_graph* const* gs, uint32_t p, const uint32_t* n,
                                          const uint32_t* const* slot, const uint64_t* const* version,
                                          const uint32_t* const* state_flags /*nullable, entries nullable*/);
fgi_status fgi_part_local_load_shards(fgi_graph* const* gs, uint32_t p, const uint64_t* m,
                                      const uint32_t* const* used, const uint32_t* const* dependant,
                                      const uint64_t* const* tag);
/* Collective wave: every rank passes the same global root list; each rank reports the
 * invalidated slots it owns (global ids) and its own share of the statistics. */
fgi_status fgi_part_invalidate(fgi_graph* g, uint32_t n_roots, const uint32_t* roots_dev,
                               const uint8_t* immediately_dev, uint64_t* out_n, fgi_wave_stats* stats);
/* (fgi_part_export_ids serves every call kind; after a wave, fgi_part_last_wave_ids / _bits below return
 * the same set without the host-side mapping and sort) */
fgi_status fgi_part_export_ids(fgi_graph* g, uint32_t* out_ids, uint64_t cap, uint64_t* out_n);
/* The same collective wave from HOST roots (C-ABI 0.8): the scope-dispose flush of
 * `using (Computed.Invalidate())` on a multi-GPU host — for each root, `existing.Invalidate(immediately[i])`
 * (Computed.cs:162-230, as fgi_invalidate). Every rank passes the same root list (global slots); the roots
 * are staged through a pinned buffer the graph owns, copied on its stream and, with partition codes, mapped
 * on the device. A root >= n_global: FGI_EINVAL on every rank alike, before anything is launched or any
 * collective joined.
 * fgi_part_invalidate_host returns this rank's invalidated slots: the global slot ids it owns, in the
 * host's numbering, strictly ascending; *out_n = the rank's V_inv. A short cap: FGI_ECAPACITY with *out_n
 * set, the wave has completed (fgi_part_last_wave_ids then returns the ids). out_ids NULL: count only.
 * fgi_part_invalidate_bits returns them as a bitmap addressed exactly like the planes of
 * fgi_part_state_view_open: bit h % 64 of out_bits[h / 64] = global slot rank * block + h, h < cfg.n_slots;
 * the bits past the rank's last owned slot and the detached handles' bits are 0, so a host applies it word
 * for word against its view-indexed tables. `words` >= (n_slots + n_detached + 63) / 64, else FGI_ECAPACITY
 * (nothing runs). out_bits NULL: count only.
 * Both are made on the device from the wave's invalidated bitmap (no host loop, no sort), on demand. */
fgi_status fgi_part_invalidate_host(fgi_graph* g, uint32_t n_roots, const uint32_t* roots,
                                    const uint8_t* immediately /*nullable*/, uint32_t* out_ids /*nullable*/, uint64_t cap,
                                    uint64_t* out_n, fgi_wave_stats* stats /*nullable*/);
fgi_status fgi_part_invalidate_bits(fgi_graph* g, uint32_t n_roots, const uint32_t* roots,
                                    const uint8_t* immediately /*nullable*/, uint64_t* out_bits /*nullable*/, uint64_t words,
                                    uint64_t* out_n, fgi_wave_stats* stats /*nullable*/);
/* This rank's share of its last wave (the set Computed.Invalidate(), Computed.cs:162-230, moved from
 * Consistent to Invalidated; a partition's fgi_last_wave_ids / fgi_wave_ids_dev), made on demand, once per
 * wave: ids and bitmap as described above, ids_dev the same ascending list in device memory. No collective
 * runs: any rank may ask at any time, in any order. Valid after fgi_part_invalidate, fgi_part_invalidate_host,
 * fgi_part_invalidate_bits, fgi_part_invalidate_all and each rank of fgi_part_local_invalidate, until the
 * rank's next call that runs a cascade (ids_dev too). After any other call that ran cascades
 * (fgi_part_begin_compute, fgi_part_set_output, fgi_part_run_batch, which return ids through their own
 * out_ids): FGI_ENOTSUP. After fgi_restore, and before any wave: FGI_OK with 0 ids / a zero bitmap.
 * FGI_ENOTSUP on a graph that is not partitioned, FGI_ESTATE on a poisoned one, and FGI_ESTATE naming the
 * rank and both counts if the ids made from the bitmap are not as many as the wave counted. */
fgi_status fgi_part_last_wave_ids(fgi_graph* g, uint32_t* out_ids /*nullable*/, uint64_t cap, uint64_t* out_n);
fgi_status fgi_part_last_wave_bits(fgi_graph* g, uint64_t* out_bits /*nullable*/, uint64_t words, uint64_t* out_n);
fgi_status fgi_part_wave_ids_dev(fgi_graph* g, const uint32_t** ids_dev, uint64_t* n /*nullable*/);
/* In-process partition group: `p` graphs (created with rank = i, world = p) emulate p ranks in
 * one process — on one device or several. fgi_part_local_invalidate runs the RCCL path's own level
 * loop on every rank (one host thread per rank); only the collectives differ (device copies
 * between the group's buffers instead of RCCL). Used to test and rehearse the multi-GPU engine on
 * one GPU. */
fgi_status fgi_part_init_local(fgi_graph* const* gs, uint32_t p, uint32_t n_global);
fgi_status fgi_part_local_invalidate(fgi_graph* const* gs, uint32_t p, uint32_t n_roots, const uint32_t* roots,
                                     const uint8_t* immediately /*nullable*/, fgi_wave_stats* stats /*p entries*/);
/* ---- mutations, batches and pruning on a partition ----------------
 * The registry's mutations on a partitioned graph. Every rank makes the same call with the same
 * arguments — global slot ids, the whole batch — in the same order (the host broadcasts them): each
 * rank applies the items of the slots it owns, records every listed version in its replica (ver_all),
 * and joins the call's collectives: the cascades (displacement, InvalidateOnSetOutput, invalidation
 * steps) run as partitioned waves, and an all-reduce carries a pair's state between the ranks owning
 * its two ends. Results are those of the single-device call on the whole graph: out_ids gets this
 * rank's invalidated slots (global ids; cascade after cascade, each ascending).
 *   fgi_part_begin_compute  fgi_begin_compute; out_detached[i]: the detached local handle on the
 *                           slot's owner (FGI_NONE on the other ranks). FGI_ECAPACITY on every rank
 *                           when any rank is out of detached handles (nothing applied)
 *   fgi_part_add_used       fgi_add_used for pairs of global slots (their current nodes); out_result
 *                           (FGI_USED_*) on every rank
 *   fgi_part_set_output     fgi_set_output for global slots; out_set on every rank
 *   fgi_part_invalidate_all fgi_invalidate_all
 *   fgi_part_run_batch      fgi_run_batch's steps (handles are global slots) applied in order; each
 *                           cascade is a partitioned wave
 *   fgi_part_prune          fgi_prune on this rank's rows (an all-gather of the current-node bitmap
 *                           decides the entries into other ranks' slots; no other collective)
 * fgi_part_local_run_batch / fgi_part_local_prune run the same on every rank of an in-process group
 * (fgi_part_init_local): the out arrays are merged (out_detached from each slot's owner; the results
 * every rank computes must agree), out_ids gets rank 0's ids, then rank 1's, ...; stats: p entries. */
fgi_status fgi_part_begin_compute(fgi_graph* g, uint32_t n, const uint32_t* slot, const uint64_t* version,
                                  const uint8_t* has_delay /*nullable*/, uint32_t* out_detached /*nullable*/,
                                  uint32_t* out_ids, uint64_t cap, uint64_t* out_n, fgi_wave_stats* stats);
fgi_status fgi_part_add_used(fgi_graph* g, uint32_t n, const uint32_t* dependant, const uint32_t* used,
                             uint32_t* out_result /*nullable*/);
fgi_status fgi_part_set_output(fgi_graph* g, uint32_t n, const uint32_t* slot, uint8_t* out_set /*nullable*/,
                               uint32_t* out_ids, uint64_t cap, uint64_t* out_n, fgi_wave_stats* stats);
fgi_status fgi_part_invalidate_all(fgi_graph* g, uint32_t* out_ids, uint64_t cap, uint64_t* out_n,
                                   fgi_wave_stats* stats);
fgi_status fgi_part_run_batch(fgi_graph* g, uint32_t n_steps, const fgi_step* steps, uint32_t* out_ids, uint64_t cap,
                              uint64_t* out_n, fgi_batch_stats* stats);
fgi_status fgi_part_prune(fgi_graph* g, fgi_prune_stats* stats);
fgi_status fgi_part_local_run_batch(fgi_graph* const* gs, uint32_t p, uint32_t n_steps, const fgi_step* steps,
                                    uint32_t* out_ids, uint64_t cap, uint64_t* out_n,
                                    fgi_batch_stats* stats /*p entries*/);
fgi_status fgi_part_local_prune(fgi_graph* const* gs, uint32_t p, fgi_prune_stats* stats /*p entries*/);
/* This rank's share of the flagged sets of the last fgi_part_* call that ran cascades (C-ABI 0.4): the
 * partitioned counterpart of fgi_last_wave_flagged and fgi_last_batch_flagged, from which a multi-GPU host
 * starts its invalidation-delay timers.
 * A call of one cascade (fgi_part_invalidate, fgi_part_begin_compute, fgi_part_set_output,
 * fgi_part_invalidate_all, each rank of fgi_part_local_invalidate) reports one run, out_step[i] = 0.
 * fgi_part_run_batch (each rank of fgi_part_local_run_batch) reports cascade after cascade in step order,
 * out_step[i] = the step's index, under fgi_last_batch_flagged's contract: a slot may appear under several
 * steps, and a begin_compute step's own slots are not listed under that step.
 * A cascade's set is fgi_last_wave_flagged's, restricted to the slots this rank owns: every owned slot whose
 * canonical state_flags gained FGI_F_INVALIDATE_ON_SET_OUTPUT and / or FGI_F_INVALIDATION_DELAY_STARTED
 * during the cascade and that the cascade did not invalidate, whatever the visit order and whichever rank
 * the visit came from. out_ids are global slot ids in the host's numbering (partition codes mapped back),
 * ascending within a step; out_flags[i] = the node's canonical state_flags right after that cascade.
 * Detached handles cannot occur: a partition's roots are slots, and no edge resolves to a detached node.
 * out_step and out_flags are nullable; out_ids NULL = count only; FGI_ECAPACITY with *out_n set if cap is
 * short. The cascades wait for nothing and copy nothing for this: the records stay on the device and the
 * rank's first call after them waits and copies once. No collective runs: each rank asks for itself, at
 * any time, in any order. Valid until this rank's next fgi_part_* call that runs a cascade. After
 * fgi_restore, and before any cascade has run: FGI_OK with 0 records. FGI_ENOTSUP on a graph that is not
 * partitioned; FGI_ESTATE on a poisoned graph. A partition that never held a Computing node or one with
 * hasDelay reports empty sets at no cost: its waves allocate and launch nothing for them (the records take
 * 16 bytes of device memory per local handle otherwise). */
fgi_status fgi_part_last_flagged(fgi_graph* g, uint32_t* out_step, uint32_t* out_ids, uint32_t* out_flags,
                                 uint64_t cap, uint64_t* out_n);
/* Frontier exchanges of a partition rank so far (full all-gathers, delta exchanges) and the bytes it
 * received through them (FGI_OPT_FRONT_EXCHANGE). */
fgi_status fgi_part_front_stats(fgi_graph* g, uint64_t* full, uint64_t* delta, uint64_t* bytes);
/* ncclGetVersion of the RCCL the engine's collectives are bound to, and the file it was loaded
 * from: /opt/rocm/lib/librccl.so.1 (or $FGI_RCCL_LIBRARY), opened by path with RTLD_LOCAL on first
 * use, so an RCCL the process loaded before (torch's bundled copy) is not the one bound. */
fgi_status fgi_rccl_info(int* version, char* path /*nullable*/, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* FGI_H */
