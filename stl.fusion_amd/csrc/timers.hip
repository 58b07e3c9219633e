// timers.hip — the delay timers in device memory (C-ABI 0.11): fgi_timers_open, _close,
// _set_delay, _set_now, _run_due, _next_due, _stats_get, _list, and the hooks the wave and mutation entry
// points call (timers_arm_records, timers_move, timers_drop_handles, timers_restore).
//
// Per boundary handle: a delay code (dly: 0 the graph's default, kCodeNever, else 1 + an index into the table
// of distinct delays, dtab) and the index of the handle's entry in the record pool (ent, FGI_NONE without one).
// The pool is a dense run [0, top) of 24-byte records {due, version, handle}; a dropped entry stays as a
// tombstone (handle FGI_NONE) until the next compaction. The pool exists twice: the due pass reads one copy
// and writes the entries it keeps into the other.
//   k_tm_arm    the arm rule over candidates (flagged records, or every handle): a candidate's node word is
//               read with its visit bit folded in; new entries take pool places with one atomic per wavefront
//               (ballot + rank among the lanes). ent[h] doubles as the handle's lock within a launch, so a
//               handle listed twice is armed once.
//   k_tm_due    one pass over the pool: entries not yet due are compacted into the other copy, due ones
//               leave; a due entry whose node still has its version and is Consistent with DelayStarted
//               goes to the fired list. The list is sorted on the device and becomes the roots of one wave.
//   k_tm_move   one lane per (slot, detached handle) pair of a displacement.
//   k_tm_min    the smallest due time of the pool.
// The pool never grows behind a wave: its capacity covers every handle that holds an entry or can come to hold
// one (the entries stored, the slots with a delay of their own and the detached handles, or every handle with a
// default delay) plus the tombstones, and is brought up to that by the calls that change the bound, all of
// which wait for the device anyway (tm_reserve).
// Everything is allocated by fgi_timers_open; a graph that never opens timers launches nothing here.
//
// Auto-invalidation (C-ABI 0.13: fgi_timers_auto_open, _set_auto_delay, _start_auto, _auto_stats_get, _list_ex, and
// the hook timers_arm_auto behind fgi_set_output_ex and a batch's SET_OUTPUT steps; per rank of a partition below):
// two more delay codes per handle (adl, tdl; the same dtab) and a kind per record (TimerRec.pad bit 0: auto).
//   k_tm_arm_auto   the auto arm rule over (handle, set code, transient) candidates; it ends in tm_store, as the
//                   delay arm rule does, where an entry of the same version takes the earlier due time and the
//                   union of the kinds if either side is auto.
// The due pass fires an auto entry on any Consistent node of its version; a moved auto entry is followed by the
// delay arm rule on the detached handle.
//
// Per rank of a partition (C-ABI 0.12: fgi_part_timers_open, _set_delay, _run_due, _fired_detached,
// fgi_part_local_timers_run_due, and the hook timers_arm_part): the table covers the rank's local handles, as
// fgi_dump_states and the rank's state view address them. Handle h < n_local is the host's slot base + h, whose
// node sits at engine index gc[base + h] - base when the partition has codes, else at h (fanout.hip's
// k_sub_insert, view.hip's view_label); the handles [n_local, ext_slots) of a short last rank never hold a node;
// a detached handle is its own engine index. A partition has no hub-first labels (K = 0, no s2l), so the move,
// drop, set-delay and min kernels, which touch a node only under a detached handle, serve a rank as they are.
//   k_tm_arm_part   k_tm_arm over a call's records in prec (the host's global slot in the high half, counted by
//                   pcur[0] on the device), or over every handle of the rank.
//   k_tm_due_part   k_tm_due with two fired lists: owned slots as global ids (the roots of the partitioned
//                   wave, after the ranks' lists are gathered) and detached handles (reported, not cascaded).
// A tick is a collective (fgi_part_timers_run_due): the verdicts, the counts and the sorted lists of all ranks
// travel through part_allgather_words and part_allgatherv, then one partitioned wave runs from all the roots.
//
// Auto-invalidation per rank (C-ABI 0.14: fgi_part_timers_auto_open, _set_auto_delay, _start_auto, _auto_stats_get,
// _list_ex, and the hook timers_arm_auto_part behind fgi_part_set_output_ex and a partition batch's SET_OUTPUT
// steps): the same adl / tdl over the rank's local handles and the same kind bit.
//   k_tm_arm_auto_part   k_tm_arm_auto over candidates named by the host's global slots: the local handle is
//                        slot - base, a slot of another rank is skipped, the node is found through the rank's map.
// A rank's due pass fires an auto entry on an owned slot into the tick's roots and one on a detached handle into
// the detached list, and counts both in kTFiredA; the move, drop and min kernels serve a rank as they are.
#include "fgi_internal.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <unordered_map>

namespace fgi {

struct TimerRec {
    unsigned long long due, version;
    uint32_t handle, pad;
};

struct Timers {
    uint64_t now = 0, default_delay = 0;
    uint32_t* dly = nullptr;               // [ext_handles] delay codes
    uint32_t* ent = nullptr;               // [ext_handles] pool index of the handle's entry
    TimerRec* rec[2] = {nullptr, nullptr}; // [cap] the pool (rec[0]) and the due pass's destination
    uint64_t cap = 0;
    unsigned long long* dtab = nullptr;    // [dtab_cap] distinct delays; code c > 0 names dtab[c - 1]
    uint64_t dtab_cap = 0;
    std::vector<uint64_t> dtab_h;
    std::unordered_map<uint64_t, uint32_t> dcode;
    unsigned long long* ctr = nullptr;     // device counters (kT*), ctr_h: their pinned copy as of the last wait
    unsigned long long* ctr_h = nullptr;
    uint32_t* fired = nullptr;             // [fired_cap] the due pass's fired handles, then sorted: [fired_cap, 2 fired_cap)
    uint64_t fired_cap = 0;
    uint8_t* imm = nullptr;                // [imm_cap] ones: the fired roots' `immediately`
    uint64_t imm_cap = 0;
    uint32_t* up = nullptr;                // uploads of the host-array calls
    uint64_t up_cap = 0;
    uint64_t holders = 0;                  // handles that hold an entry or can gain one (tm_reserve; never lowered)
    uint64_t tomb_ub = 0;                  // tombstones the pool may hold
    uint64_t runs = 0;
    double last_ms = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    // a partition rank's (the fired list then has a third part, [2 fired_cap, 3 fired_cap): the detached handles)
    bool part = false;
    uint32_t* groots = nullptr;            // [groots_cap] every rank's fired slots, gathered in rank order
    uint64_t groots_cap = 0;
    std::vector<uint32_t> fdet;            // the last tick's fired detached handles, ascending (fgi_part_timers_fired_detached)
    // auto-invalidation (fgi_timers_auto_open, fgi_part_timers_auto_open): null / false until then
    bool autos = false;
    uint64_t def_auto = 0, def_trans = 0;  // the graph's default AutoInvalidationDelay / TransientErrorInvalidationDelay
    uint32_t* adl = nullptr;               // [ext_handles] auto delay codes, coded as dly (the same dtab)
    uint32_t* tdl = nullptr;               // [ext_handles] transient-error delay codes
};

namespace {

constexpr int kTBlock = 256;
constexpr uint32_t kCodeNever = 0xFFFFFFFFu;
constexpr uint32_t kClaim = 0xFFFFFFFEu;   // ent[h] while a lane of the running launch works on h
// device counters
enum { kTTop = 0, kTArmed, kTFired, kTDropped, kTMoved, kTTomb, kTFail, kTNewTop, kTFiredN, kTCoded, kTMin, kTFiredD,
       kTArmedA, kTMerged, kTFiredA, kTCodedA, kTWords = 16 };
constexpr uint32_t kKindAuto = 1u;         // TimerRec.pad bit 0: the entry is (also) an auto-invalidation's

// what every kernel reads a node and the table through
struct TmTab {
    const unsigned long long* node;
    const uint32_t* vis;        // null: no unfolded visits
    const uint32_t* s2l;        // null: no hot labels
    uint32_t ext_slots, K, n_handles;
    uint32_t* dly;
    uint32_t* ent;
    TimerRec* rec;
    uint64_t cap;
    const unsigned long long* dtab;
    uint32_t n_dtab;
    unsigned long long* ctr;
    unsigned long long now, default_delay;
    uint32_t* adl;              // null: auto-invalidation is off
    uint32_t* tdl;
    unsigned long long def_auto, def_trans;
};

// How a handle finds its node: on a single device through the table's own K and s2l (TmOne), on a rank of a
// partition through the rank's range and the slot -> code table (TmPart; the file comment).
struct TmOne {};
struct TmPart {
    uint32_t base, n_local;
    const uint32_t* gc;         // null: no partition codes
};

// the node word of boundary handle h, its visit bit folded in (fanout.hip's k_sub_insert reads it the same way)
__device__ inline unsigned long long tm_word(const TmTab& a, const TmOne&, uint32_t h) {
    uint32_t l = h + a.K;
    if (a.s2l && h < a.ext_slots) {
        const uint32_t hot = a.s2l[h];
        if (hot != FGI_NONE) l = hot;
    }
    unsigned long long w = a.node[l];
    if (a.vis && ((a.vis[l >> 5] >> (l & 31)) & 1u)) w = visited_word(w);
    return w;
}
// a rank's local handle h < n_handles; 0 (no node) for the handles of a short last rank past its slots
__device__ inline unsigned long long tm_word(const TmTab& a, const TmPart& p, uint32_t h) {
    uint32_t l = h;
    if (h < a.ext_slots) {
        if (h >= p.n_local) return 0ull;
        if (p.gc) {
            l = p.gc[p.base + h] - p.base;
            if (l >= p.n_local) return 0ull;   // a code stays in its owner's range (k_sub_insert checks the same)
        }
    }
    unsigned long long w = a.node[l];
    if (a.vis && ((a.vis[l >> 5] >> (l & 31)) & 1u)) w = visited_word(w);
    return w;
}
__device__ inline bool tm_waiting(unsigned long long w) {
    return (w & kVMask) != 0 && word_state(w) == FGI_CONSISTENT && (w & kW_DS) != 0;
}
__device__ inline unsigned long long tm_decode(const TmTab& a, uint32_t c, unsigned long long dflt) {
    if (c == 0) return dflt;
    if (c == kCodeNever || c - 1 >= a.n_dtab) return FGI_TIMER_NEVER;
    return a.dtab[c - 1];
}
__device__ inline unsigned long long tm_delay(const TmTab& a, uint32_t h) { return tm_decode(a, a.dly[h], a.default_delay); }
// now + d, saturating
__device__ inline unsigned long long tm_due_at(const TmTab& a, unsigned long long d) {
    const unsigned long long due = a.now + d;
    return due < a.now || due == FGI_TIMER_NEVER ? FGI_TIMER_NEVER - 1 : due;
}

// what a fired handle is called in the wave's root list
__device__ inline uint32_t tm_root(const TmOne&, uint32_t h) { return h; }
__device__ inline uint32_t tm_root(const TmPart& p, uint32_t h) { return p.base + h; }   // an owned slot: the host's global id

// Stores (h, v, due, kind) for every lane with `want`: the common end of the delay arm rule (kind 0) and the auto
// arm rule (kind kKindAuto). An entry of another version at h is overwritten; one of the same version keeps its
// place and, if either it or the new one is an auto-invalidation's, takes the earlier due time and the union
// of the kinds (ConcurrentTimerSet.AddOrUpdateToEarlier; counted in kTMerged); two delay arms of one version
// leave the stored due time. Called by whole wavefronts.
__device__ inline void tm_store(const TmTab& a, bool want, uint32_t h, unsigned long long v, unsigned long long due, uint32_t kind,
                                uint32_t lane) {
    bool fresh = false, over = false, merged = false;
    if (want) {
        const uint32_t e = __hip_atomic_exchange(a.ent + h, kClaim, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (e == FGI_NONE) {
            fresh = true;
        } else if (e != kClaim) {   // (kClaim: another lane of this launch has h, and will leave the same entry)
            if (e < a.cap) {
                TimerRec& r = a.rec[e];
                if (r.version != v) {   // another version's entry: overwritten
                    r.version = v;
                    r.due = due;
                    r.pad = kind;
                    over = true;
                } else if (kind || (r.pad & kKindAuto)) {
                    if (due < r.due) r.due = due;
                    r.pad |= kind;
                    merged = true;
                }
            }
            __hip_atomic_store(a.ent + h, e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // the counters, one atomic per wavefront and counter (a recomputed graph overwrites an entry per item)
    const unsigned long long mo = __ballot(over), mm = __ballot(merged);
    if (lane == 0) {
        if (mo) {
            atomicAdd(a.ctr + kTArmed, (unsigned long long)__popcll(mo));
            atomicAdd(a.ctr + kTDropped, (unsigned long long)__popcll(mo));
            if (kind) atomicAdd(a.ctr + kTArmedA, (unsigned long long)__popcll(mo));
        }
        if (mm) atomicAdd(a.ctr + kTMerged, (unsigned long long)__popcll(mm));
    }
    const unsigned long long m = __ballot(fresh);
    if (!m) return;
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if ((int)lane == leader) base = atomicAdd(a.ctr + kTTop, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    bool stored = false;
    if (fresh) {
        const unsigned long long idx = base + __popcll(m & ((1ull << lane) - 1));
        if (idx < a.cap) {
            a.rec[idx] = TimerRec{due, v, h, kind};
            __hip_atomic_store(a.ent + h, (uint32_t)idx, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            stored = true;
        } else {   // never with the host's capacity bound: the call that reads the counters next fails
            __hip_atomic_store(a.ent + h, FGI_NONE, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            atomicAdd(a.ctr + kTFail, 1ull);
        }
    }
    const unsigned long long ms = __ballot(stored);
    if ((int)lane == leader && ms) {
        atomicAdd(a.ctr + kTArmed, (unsigned long long)__popcll(ms));
        if (kind) atomicAdd(a.ctr + kTArmedA, (unsigned long long)__popcll(ms));
    }
}

// The arm rule on candidate h of every lane for which cand holds. Called by whole wavefronts.
template <class M>
__device__ inline void tm_arm(const TmTab& a, const M& map, bool cand, uint32_t h, uint32_t lane) {
    bool want = false;
    unsigned long long v = 0, due = 0;
    if (cand && h < a.n_handles) {
        const unsigned long long w = tm_word(a, map, h);
        const unsigned long long d = tm_waiting(w) ? tm_delay(a, h) : 0ull;
        if (d != 0 && d != FGI_TIMER_NEVER) {
            want = true;
            v = w & kVMask;
            due = tm_due_at(a, d);
        }
    }
    tm_store(a, want, h, v, due, 0u, lane);
}

// Candidates: flagged records (rec != null: boundary handle << 32 | flags), else every handle below n_max.
// n = min(n_max, *n_dev). Wavefronts stride over runs of 64 candidates (wave-uniform trip count).
__global__ __launch_bounds__(kTBlock) void k_tm_arm(TmTab a, const unsigned long long* rec, uint64_t n_max,
                                                    const unsigned long long* n_dev) {
    uint64_t n = n_max;
    if (n_dev) {
        const unsigned long long c = *n_dev;
        if (c < n) n = c;
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t base = (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 64; base < n; base += nwaves * 64) {
        const uint64_t i = base + lane;
        const bool cand = i < n;
        const uint32_t h = !cand ? 0u : rec ? (uint32_t)(rec[i] >> 32) : (uint32_t)i;
        tm_arm(a, TmOne{}, cand, h, lane);
    }
}

// The auto arm rule (StartAutoInvalidation, Computed.cs:235-246) over n candidates. Item i is a candidate if its
// set code is 1 (code null: every item; 2: set with InvalidateOnSetOutput, Computed.cs:153-156 returns before
// StartAutoInvalidation; 0: not set). The node now at hs[i] must be Consistent; its delay is the transient-error
// one if tr[i] (tr nullable), else the auto one, read at src[i] (src nullable: at hs[i]). Wavefronts stride over
// runs of 64 candidates, as k_tm_arm's.
__global__ __launch_bounds__(kTBlock) void k_tm_arm_auto(TmTab a, uint64_t n, const uint32_t* hs, const uint32_t* src,
                                                         const uint8_t* code, const uint8_t* tr) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t base = (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 64; base < n; base += nwaves * 64) {
        const uint64_t i = base + lane;
        bool want = false;
        uint32_t h = 0;
        unsigned long long v = 0, due = 0;
        if (i < n && (!code || code[i] == 1)) {
            h = hs[i];
            const uint32_t s = src ? src[i] : h;
            if (h < a.n_handles && s < a.n_handles) {
                const unsigned long long w = tm_word(a, TmOne{}, h);
                if ((w & kVMask) != 0 && word_state(w) == FGI_CONSISTENT) {
                    const bool t = tr && tr[i];
                    const unsigned long long d = tm_decode(a, t ? a.tdl[s] : a.adl[s], t ? a.def_trans : a.def_auto);
                    if (d != 0 && d != FGI_TIMER_NEVER) {
                        want = true;
                        v = w & kVMask;
                        due = tm_due_at(a, d);
                    }
                }
            }
        }
        tm_store(a, want, h, v, due, kKindAuto, lane);
    }
}

// The due pass over the pool [0, top) (top = min(ctr[kTTop], cap)): see the file comment. dst: the other copy.
// On a rank of a partition (M = TmPart) a fired owned slot goes to `fired` as the host's global slot id and a
// fired detached handle to fired_det (counted by ctr[kTFiredD]), both of fired_cap entries. top, first,
// nwaves, lane: the pool's top, the wavefront's first run of 64 records, the launch's wavefronts and the lane.
template <class M>
__device__ __forceinline__ void tm_due(const TmTab& a, const M& m, TimerRec* dst, uint32_t* fired, uint32_t* fired_det,
                                       uint64_t fired_cap, uint64_t top, uint64_t first, uint64_t nwaves, uint32_t lane) {
    constexpr bool kPart = std::is_same<M, TmPart>::value;
    for (uint64_t base = first; base < top; base += nwaves * 64) {
        const uint64_t i = base + lane;
        TimerRec r{0, 0, FGI_NONE, 0};
        if (i < top) r = a.rec[i];
        const bool live = r.handle < a.n_handles;
        const bool is_due = live && r.due <= a.now;
        const bool keep = live && !is_due;
        bool fire = false;
        if (is_due) {
            const unsigned long long w = tm_word(a, m, r.handle);
            // an auto-invalidation's timer calls Invalidate(true) on any live computed (ComputedExt.cs:35)
            fire = (w & kVMask) != 0 && word_state(w) == FGI_CONSISTENT && ((w & kW_DS) != 0 || (r.pad & kKindAuto)) &&
                   (w & kVMask) == r.version;
            a.ent[r.handle] = FGI_NONE;
        }
        const bool fire_auto = fire && (r.pad & kKindAuto);   // (on a rank: owned slots and detached handles alike)
        bool fire_det = false;   // a rank's detached handle: no partitioned cascade reaches its node
        if constexpr (kPart) {
            fire_det = fire && r.handle >= a.ext_slots;
            fire = fire && !fire_det;
        }
        const unsigned long long mk = __ballot(keep), mf = __ballot(fire), md = __ballot(is_due && !fire && !fire_det);
        const unsigned long long ma = __ballot(fire_auto);
        unsigned long long mt = 0;
        if constexpr (kPart) mt = __ballot(fire_det);
        unsigned long long bk = 0, bf = 0, bt = 0;
        if (lane == 0) {
            if (mk) bk = atomicAdd(a.ctr + kTNewTop, (unsigned long long)__popcll(mk));
            if (mf) {
                bf = atomicAdd(a.ctr + kTFiredN, (unsigned long long)__popcll(mf));
                atomicAdd(a.ctr + kTFired, (unsigned long long)__popcll(mf));
            }
            if (mt) {
                bt = atomicAdd(a.ctr + kTFiredD, (unsigned long long)__popcll(mt));
                atomicAdd(a.ctr + kTFired, (unsigned long long)__popcll(mt));
            }
            if (md) atomicAdd(a.ctr + kTDropped, (unsigned long long)__popcll(md));
            if (ma) atomicAdd(a.ctr + kTFiredA, (unsigned long long)__popcll(ma));
        }
        bk = __shfl(bk, 0);
        bf = __shfl(bf, 0);
        if constexpr (kPart) bt = __shfl(bt, 0);
        const unsigned long long below = (1ull << lane) - 1;
        if (keep) {
            const unsigned long long idx = bk + __popcll(mk & below);   // < top <= cap
            dst[idx] = r;
            a.ent[r.handle] = (uint32_t)idx;
        }
        if (fire) {
            const unsigned long long idx = bf + __popcll(mf & below);
            if (idx < fired_cap) fired[idx] = tm_root(m, r.handle);
            else atomicAdd(a.ctr + kTFail, 1ull);
        }
        if (fire_det) {
            const unsigned long long idx = bt + __popcll(mt & below);
            if (idx < fired_cap) fired_det[idx] = r.handle;
            else atomicAdd(a.ctr + kTFail, 1ull);
        }
    }
}

__global__ __launch_bounds__(kTBlock) void k_tm_due(TmTab a, TimerRec* dst, uint32_t* fired, uint64_t fired_cap) {
    const unsigned long long t = a.ctr[kTTop];
    const uint64_t top = t < a.cap ? t : a.cap;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    tm_due(a, TmOne{}, dst, fired, nullptr, fired_cap, top, (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 64, nwaves, lane);
}

// behind the due pass: the compacted copy is the pool
__global__ void k_tm_commit(unsigned long long* ctr) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        ctr[kTTop] = ctr[kTNewTop];
        ctr[kTTomb] = 0;
    }
}

// pair i: the node that left slot from[i] lives on at to[i]. to[i] takes the slot's delays; the slot's entry
// moves with it, kind and all, if it is the node's (same version), else the arm rule runs on to[i]; it also runs
// behind a moved auto entry (the displacement has just started the node's delay: the earlier due time stays,
// ComputedRegistry.cs:91-96 -> Computed.cs:186-197). from[] distinct.
__global__ __launch_bounds__(kTBlock) void k_tm_move(TmTab a, uint32_t n, const uint32_t* from, const uint32_t* to) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    bool arm = false;
    uint32_t d = 0;
    if (i < n) {
        const uint32_t f = from[i];
        d = to[i];
        if (d != FGI_NONE && f != d && f < a.n_handles && d < a.n_handles) {
            a.dly[d] = a.dly[f];
            if (a.adl) {
                a.adl[d] = a.adl[f];
                a.tdl[d] = a.tdl[f];
            }
            const unsigned long long w = tm_word(a, TmOne{}, d);
            const uint32_t e = a.ent[f];
            if (e != FGI_NONE && e < a.cap && (w & kVMask) != 0 && a.rec[e].version == (w & kVMask)) {
                const uint32_t old = a.ent[d];   // a detached handle handed out anew has none: released ones drop theirs
                if (old != FGI_NONE && old < a.cap) {
                    a.rec[old].handle = FGI_NONE;
                    atomicAdd(a.ctr + kTTomb, 1ull);
                    atomicAdd(a.ctr + kTDropped, 1ull);
                }
                a.rec[e].handle = d;
                a.ent[d] = e;
                a.ent[f] = FGI_NONE;
                atomicAdd(a.ctr + kTMoved, 1ull);
                arm = (a.rec[e].pad & kKindAuto) != 0;
            } else {
                arm = true;
            }
        }
    }
    tm_arm(a, TmOne{}, arm, d, lane);
}

__global__ __launch_bounds__(kTBlock) void k_tm_drop(TmTab a, uint32_t n, const uint32_t* handles) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = handles[i];
    if (h >= a.n_handles) return;
    const uint32_t e = atomicExch(a.ent + h, FGI_NONE);   // a handle listed twice is dropped once
    if (e == FGI_NONE || e >= a.cap) return;
    a.rec[e].handle = FGI_NONE;
    atomicAdd(a.ctr + kTTomb, 1ull);
    atomicAdd(a.ctr + kTDropped, 1ull);
}

// handle[i] takes code[i]; ctr[kTCoded] gains the slots that got a code of their own less those that lost
// theirs (handles distinct within a launch). Detached handles are not counted: a move copies a code onto one
// without this kernel, and tm_reserve counts every one of them anyway.
__global__ __launch_bounds__(kTBlock) void k_tm_set_delay(uint32_t* dly, uint32_t n, const uint32_t* handle, const uint32_t* code,
                                                          uint32_t ext_slots, unsigned long long* ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t old = dly[handle[i]], c = code[i];
    dly[handle[i]] = c;
    if (handle[i] >= ext_slots) return;
    if (!old && c) atomicAdd(ctr + kTCoded, 1ull);
    if (old && !c) atomicAdd(ctr + kTCoded, ~0ull);   // - 1
}

// handle[i] takes the auto code ac[i] and the transient-error code tc[i] (each nullable: that code stays);
// ctr[kTCodedA] follows the slots that hold either code, as ctr[kTCoded] follows dly's.
__global__ __launch_bounds__(kTBlock) void k_tm_set_auto(uint32_t* adl, uint32_t* tdl, uint32_t n, const uint32_t* handle,
                                                         const uint32_t* ac, const uint32_t* tc, uint32_t ext_slots,
                                                         unsigned long long* ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = handle[i];
    const bool old = adl[h] || tdl[h];
    if (ac) adl[h] = ac[i];
    if (tc) tdl[h] = tc[i];
    const bool now = adl[h] || tdl[h];
    if (h >= ext_slots) return;
    if (!old && now) atomicAdd(ctr + kTCodedA, 1ull);
    if (old && !now) atomicAdd(ctr + kTCodedA, ~0ull);   // - 1
}

// ctr[kTMin] (set to FGI_TIMER_NONE first) = the smallest due time of the pool's entries
__global__ __launch_bounds__(kTBlock) void k_tm_min(const TimerRec* rec, uint64_t cap, uint32_t n_handles, unsigned long long* ctr) {
    const unsigned long long t = ctr[kTTop];
    const uint64_t top = t < cap ? t : cap;
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long m = FGI_TIMER_NONE;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < top; i += nthr) {
        const TimerRec r = rec[i];
        if (r.handle < n_handles && r.due < m) m = r.due;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(m, d);
        if (o < m) m = o;
    }
    if ((threadIdx.x & 63) == 0 && m != FGI_TIMER_NONE) atomicMin(ctr + kTMin, m);
}

// ---- a rank of a partition: behind the single-device kernels, which keep their places -------------------------
// k_tm_arm for a rank. Candidates: the call's flagged records (rec != null: the host's global slot << 32 | flags;
// a slot outside [base, base + n_local) is not the rank's and is skipped), else every local handle below n_max.
__global__ __launch_bounds__(kTBlock) void k_tm_arm_part(TmTab a, TmPart p, const unsigned long long* rec, uint64_t n_max,
                                                         const unsigned long long* n_dev) {
    uint64_t n = n_max;
    if (n_dev) {
        const unsigned long long c = *n_dev;
        if (c < n) n = c;
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t base = (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 64; base < n; base += nwaves * 64) {
        const uint64_t i = base + lane;
        bool cand = i < n;
        uint32_t h = 0;
        if (cand) {
            h = rec ? (uint32_t)(rec[i] >> 32) - p.base : (uint32_t)i;   // (a slot below base wraps past n_local)
            if (rec) cand = h < p.n_local;
        }
        tm_arm(a, p, cand, h, lane);
    }
}

// k_tm_arm_auto for a rank. Item i names the host's global slot slot[i]; its local handle is slot[i] - base (a slot
// below base wraps past n_local) and a slot of another rank is no candidate, nor is an item whose set code is
// not 1 (code nullable: every item). The node is read through the rank's map, the delay codes at the same local
// handle, the set code and the transient flag (tr nullable) by item. An item that is skipped only clears `want`:
// every lane of a wavefront reaches tm_store, and the trip count depends on the wavefront alone.
__global__ __launch_bounds__(kTBlock) void k_tm_arm_auto_part(TmTab a, TmPart p, uint64_t n, const uint32_t* slot,
                                                              const uint8_t* code, const uint8_t* tr) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t base = (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 64; base < n; base += nwaves * 64) {
        const uint64_t i = base + lane;
        bool want = false;
        uint32_t h = 0;
        unsigned long long v = 0, due = 0;
        if (i < n && (!code || code[i] == 1)) {
            const uint32_t l = slot[i] - p.base;
            if (l < p.n_local && l < a.n_handles) {
                const unsigned long long w = tm_word(a, p, l);
                if ((w & kVMask) != 0 && word_state(w) == FGI_CONSISTENT) {
                    const bool t = tr && tr[i];
                    const unsigned long long d = tm_decode(a, t ? a.tdl[l] : a.adl[l], t ? a.def_trans : a.def_auto);
                    if (d != 0 && d != FGI_TIMER_NEVER) {
                        want = true;
                        h = l;
                        v = w & kVMask;
                        due = tm_due_at(a, d);
                    }
                }
            }
        }
        tm_store(a, want, h, v, due, kKindAuto, lane);
    }
}

__global__ __launch_bounds__(kTBlock) void k_tm_due_part(TmTab a, TmPart p, TimerRec* dst, uint32_t* fired, uint32_t* fired_det,
                                                         uint64_t fired_cap) {
    const unsigned long long t = a.ctr[kTTop];
    const uint64_t top = t < a.cap ? t : a.cap;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    tm_due(a, p, dst, fired, fired_det, fired_cap, top, (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 64, nwaves, lane);
}

inline uint32_t tgrid(uint64_t n) { return (uint32_t)std::min<uint64_t>(1024, std::max<uint64_t>(1, (n + kTBlock - 1) / kTBlock)); }

TmTab tm_tab(const fgi_graph* g) {
    const Timers* t = g->tim;
    TmTab a{};
    a.node = reinterpret_cast<const unsigned long long*>(g->node);
    a.vis = g->v_dirty && !g->vis_stale ? g->vis_bm : nullptr;
    a.s2l = g->lbl_hot ? g->s2l : nullptr;
    a.ext_slots = g->ext_slots;
    a.K = g->lbl_K;
    a.n_handles = g->ext_handles;
    a.dly = t->dly;
    a.ent = t->ent;
    a.rec = t->rec[0];
    a.cap = t->cap;
    a.dtab = t->dtab;
    a.n_dtab = (uint32_t)t->dtab_h.size();
    a.ctr = t->ctr;
    a.now = t->now;
    a.default_delay = t->default_delay;
    a.adl = t->autos ? t->adl : nullptr;
    a.tdl = t->autos ? t->tdl : nullptr;
    a.def_auto = t->def_auto;
    a.def_trans = t->def_trans;
    return a;
}

// a rank's handle map (the file comment)
TmPart tm_part(fgi_graph* g) {
    PartView pv{};
    part_view(g, &pv);
    return TmPart{pv.base, pv.n_local, g->lbl_perm ? (const uint32_t*)g->pg_gc : nullptr};
}

// the arm rule over every handle the graph holds (fgi_timers_open, fgi_part_timers_open on a populated graph)
void tm_arm_all(fgi_graph* g) {
    const Timers* t = g->tim;
    const uint64_t n = g->ext_handles;
    if (t->part)
        hipLaunchKernelGGL(k_tm_arm_part, dim3(tgrid(n)), dim3(kTBlock), 0, g->stream, tm_tab(g), tm_part(g),
                           (const unsigned long long*)nullptr, n, (const unsigned long long*)nullptr);
    else
        hipLaunchKernelGGL(k_tm_arm, dim3(tgrid(n)), dim3(kTBlock), 0, g->stream, tm_tab(g), (const unsigned long long*)nullptr, n,
                           (const unsigned long long*)nullptr);
}

// the counters back on the host (one wait). A pool that overflowed lost entries: the host's bound was wrong.
fgi_status tm_sync(fgi_graph* g, const char* what) {
    Timers* t = g->tim;
    FGI_HIP(g, hipGetLastError());
    FGI_HIP(g, hipMemcpyAsync(t->ctr_h, t->ctr, kTWords * 8, hipMemcpyDeviceToHost, g->stream));
    FGI_HIP(g, hipStreamSynchronize(g->stream));
    if (t->ctr_h[kTFail])
        return set_err(g, FGI_ESTATE, "%s: the timer pool of %llu records overflowed (%llu entries lost)", what,
                       (unsigned long long)t->cap, (unsigned long long)t->ctr_h[kTFail]);
    return FGI_OK;
}
inline uint64_t tm_top(const Timers* t) { return std::min<uint64_t>(t->ctr_h[kTTop], t->cap); }
inline uint64_t tm_stored(const Timers* t) { return tm_top(t) - std::min<uint64_t>(t->ctr_h[kTTomb], tm_top(t)); }

// The pool's capacity covers every entry and tombstone it can come to hold before a call that waits next looks
// (the file comment): cap >= holders + tomb_ub. The pool's places [0, top) are its entries and its tombstones:
// an entry takes a new place only when its handle had none (an overwrite and a move reuse the place), a dropped
// one leaves a tombstone (at most tomb_ub), and places come back only in a due pass, which leaves the entries
// alone. A handle holds at most one entry, so the entries never outnumber P = the handles that hold one now or
// can gain one: with a default delay any handle, else the slots with a delay code of their own and the
// detached handles (a move copies the slot's code onto one). A slot that lost its code keeps its entry until
// that comes due, so it stays in P by its entry, not by its code; the most codes there ever were is no bound
// once codes pass from one set of slots to another. Without a default delay P gains members only in
// fgi_timers_set_delay, whose last wait knows |P| <= stored + coded slots + detached handles; everything else
// (waves, moves, releases, due passes, fgi_restore) only moves entries within P or takes members out.
// `holders` is the largest such value seen, so it is never lowered between two due passes.
// On a rank of a partition every term is the rank's own: ext_handles and ext_slots are its local handles and
// slots, n_detached its detached handles, and ctr[kTCoded] counts only slots the rank owns (fgi_part_timers_
// set_delay uploads no other), so the argument holds per rank with no word from another rank. The tick's wave
// arms behind a due pass that only took entries out, and the arm behind a batch runs after the batch's moves,
// each of which ended in tm_reserve.
// Grows by copying; the caller's next kernel arguments are built afterwards.
fgi_status tm_reserve(fgi_graph* g) {
    Timers* t = g->tim;
    auto finite = [](uint64_t d) { return d != 0 && d != FGI_TIMER_NEVER; };
    // (an auto or transient-error default lets any handle's node gain an entry, as a default delay does)
    const bool every = finite(t->default_delay) || (t->autos && (finite(t->def_auto) || finite(t->def_trans)));
    const uint64_t holders = every ? g->ext_handles : std::min<uint64_t>(g->ext_handles, t->holders);
    const uint64_t need = holders + t->tomb_ub;
    if (t->cap >= need && t->rec[0]) return FGI_OK;
    const uint64_t want = std::max<uint64_t>({need, 2 * t->cap, 1024});
    if (want >= kClaim) return set_err(g, FGI_ENOMEM, "the timer pool holds at most 2^32 - 3 records");
    DevOwn<TimerRec> r0, r1;   // until they are installed
    if (hipMalloc(reinterpret_cast<void**>(&r0.p), want * sizeof(TimerRec)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&r1.p), want * sizeof(TimerRec)) != hipSuccess)
        return set_err(g, FGI_ENOMEM, "a timer pool of %llu records", (unsigned long long)want);
    if (t->rec[0]) {
        FGI_TRY(tm_sync(g, "growing the timer pool"));
        const uint64_t top = tm_top(t);
        if (top) FGI_HIP(g, hipMemcpyAsync(r0.p, t->rec[0], top * sizeof(TimerRec), hipMemcpyDeviceToDevice, g->stream));
        FGI_HIP(g, hipStreamSynchronize(g->stream));
    }
    dfree(t->rec[0]);
    dfree(t->rec[1]);
    t->rec[0] = r0.release();
    t->rec[1] = r1.release();
    t->cap = want;
    return FGI_OK;
}

// host words to the upload buffer (several arrays of n u32 each, back to back)
fgi_status tm_upload(fgi_graph* g, uint64_t arrays, uint64_t n) {
    Timers* t = g->tim;
    return grow(g, &t->up, &t->up_cap, std::max<uint64_t>(arrays * n, 4096), "the timers' upload");
}

// what every entry point of the section but open and stats checks first
fgi_status tm_usable(fgi_graph* g, const char* what) {
    if (g->failed) return set_err(g, FGI_ESTATE, "%s: the graph is poisoned; fgi_restore or fgi_destroy", what);
    if (!g->tim) return set_err(g, FGI_ESTATE, "%s: the graph's timers are not open (fgi_timers_open)", what);
    hipSetDevice(g->device);
    if (g->aw[0].busy || g->aw[1].busy) FGI_TRY(drain_async(g));
    return FGI_OK;
}

}  // namespace

fgi_status timers_arm_records(fgi_graph* g, const unsigned long long* rec, uint64_t n_max, const unsigned long long* n_dev) {
    if (!timers_on(g) || !n_max) return FGI_OK;
    hipLaunchKernelGGL(k_tm_arm, dim3(tgrid(n_max)), dim3(kTBlock), 0, g->stream, tm_tab(g), rec, n_max, n_dev);
    FGI_HIP(g, hipGetLastError());
    return FGI_OK;
}

fgi_status timers_arm_part(fgi_graph* g) {
    if (!timers_on(g) || !g->tim->part || !g->flag_gate || !g->prec || !g->pcur || g->pflg_runs.empty()) return FGI_OK;
    hipLaunchKernelGGL(k_tm_arm_part, dim3(tgrid(g->prec_cap)), dim3(kTBlock), 0, g->stream, tm_tab(g), tm_part(g),
                       (const unsigned long long*)g->prec, g->prec_cap, (const unsigned long long*)g->pcur);
    FGI_HIP(g, hipGetLastError());
    return FGI_OK;
}

fgi_status timers_move(fgi_graph* g, uint32_t n, const uint32_t* from, const uint32_t* to) {
    if (!timers_on(g) || !n) return FGI_OK;
    Timers* t = g->tim;
    hipStream_t s = g->stream;
    FGI_TRY(flush_vis(g));
    FGI_TRY(tm_upload(g, 2, n));
    FGI_HIP(g, hipMemcpyAsync(t->up, from, (size_t)n * 4, hipMemcpyHostToDevice, s));
    FGI_HIP(g, hipMemcpyAsync(t->up + n, to, (size_t)n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_tm_move, dim3((n + kTBlock - 1) / kTBlock), dim3(kTBlock), 0, s, tm_tab(g), n,
                       (const uint32_t*)t->up, (const uint32_t*)(t->up + n));
    // a moved entry may have overwritten a tombstone-to-be; the host arrays are the caller's: consumed when this returns
    t->tomb_ub += n;
    FGI_TRY(tm_sync(g, "moving a displaced node's timer"));
    t->tomb_ub = t->ctr_h[kTTomb];
    return tm_reserve(g);
}

bool timers_auto_on(const fgi_graph* g) { return g->tim && g->tim->autos; }

fgi_status timers_arm_auto(fgi_graph* g, uint32_t n, const uint32_t* handle, const uint32_t* src, const uint8_t* code_dev,
                           const uint8_t* code_host, const uint8_t* transient, bool wait) {
    if (!timers_auto_on(g) || !n) return FGI_OK;
    Timers* t = g->tim;
    hipStream_t s = g->stream;
    FGI_TRY(flush_vis(g));
    // the upload: handles | delay sources | set codes (bytes) | transient flags (bytes)
    const uint64_t bw = ((uint64_t)n + 3) / 4;
    FGI_TRY(tm_upload(g, 1, 2 * (uint64_t)n + 2 * bw));
    uint32_t* dh = t->up;
    uint32_t* ds = t->up + n;
    uint8_t* dc = reinterpret_cast<uint8_t*>(t->up + 2 * (uint64_t)n);
    uint8_t* dt = reinterpret_cast<uint8_t*>(t->up + 2 * (uint64_t)n + bw);
    FGI_HIP(g, hipMemcpyAsync(dh, handle, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (src) FGI_HIP(g, hipMemcpyAsync(ds, src, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (!code_dev && code_host) FGI_HIP(g, hipMemcpyAsync(dc, code_host, n, hipMemcpyHostToDevice, s));
    if (transient) FGI_HIP(g, hipMemcpyAsync(dt, transient, n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_tm_arm_auto, dim3(tgrid(n)), dim3(kTBlock), 0, s, tm_tab(g), (uint64_t)n, (const uint32_t*)dh,
                       src ? (const uint32_t*)ds : (const uint32_t*)nullptr,
                       code_dev ? code_dev : code_host ? (const uint8_t*)dc : (const uint8_t*)nullptr,
                       transient ? (const uint8_t*)dt : (const uint8_t*)nullptr);
    if (!wait) {
        FGI_HIP(g, hipGetLastError());
        return FGI_OK;
    }
    return tm_sync(g, "arming auto-invalidation timers");
}

fgi_status timers_arm_auto_part(fgi_graph* g, uint32_t n, const uint32_t* slot_dev, const uint8_t* code_dev,
                                const uint8_t* transient_dev) {
    if (!timers_auto_on(g) || !g->tim->part || !n) return FGI_OK;
    hipLaunchKernelGGL(k_tm_arm_auto_part, dim3(tgrid(n)), dim3(kTBlock), 0, g->stream, tm_tab(g), tm_part(g), (uint64_t)n,
                       slot_dev, code_dev, transient_dev);
    FGI_HIP(g, hipGetLastError());
    return FGI_OK;
}

fgi_status timers_wait(fgi_graph* g) {
    if (!timers_on(g)) return FGI_OK;
    return tm_sync(g, "arming auto-invalidation timers");
}

fgi_status timers_drop_handles(fgi_graph* g, uint32_t n, const uint32_t* handles) {
    if (!timers_on(g) || !n) return FGI_OK;
    Timers* t = g->tim;
    hipStream_t s = g->stream;
    FGI_TRY(tm_upload(g, 1, n));
    FGI_HIP(g, hipMemcpyAsync(t->up, handles, (size_t)n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_tm_drop, dim3((n + kTBlock - 1) / kTBlock), dim3(kTBlock), 0, s, tm_tab(g), n, (const uint32_t*)t->up);
    FGI_TRY(tm_sync(g, "dropping a released handle's timer"));
    t->tomb_ub = t->ctr_h[kTTomb];
    return tm_reserve(g);
}

fgi_status timers_restore(fgi_graph* g) {
    if (!timers_on(g)) return FGI_OK;
    Timers* t = g->tim;
    hipStream_t s = g->stream;
    hipSetDevice(g->device);
    FGI_HIP(g, hipMemcpyAsync(t->ctr_h, t->ctr, kTWords * 8, hipMemcpyDeviceToHost, s));
    FGI_HIP(g, hipStreamSynchronize(s));
    t->ctr_h[kTDropped] += tm_stored(t);   // every entry is dropped
    t->ctr_h[kTTop] = t->ctr_h[kTTomb] = t->ctr_h[kTFail] = 0;
    t->tomb_ub = 0;
    t->fdet.clear();
    FGI_HIP(g, hipMemcpyAsync(t->ctr, t->ctr_h, kTWords * 8, hipMemcpyHostToDevice, s));
    FGI_HIP(g, hipMemsetAsync(t->ent, 0xFF, (size_t)g->ext_handles * 4, s));
    FGI_HIP(g, hipStreamSynchronize(s));
    return FGI_OK;
}

void timers_destroy(fgi_graph* g) {
    Timers* t = g->tim;
    if (!t) return;
    void* dev[] = {t->dly, t->ent, t->rec[0], t->rec[1], t->dtab, t->ctr, t->fired, t->imm, t->up, t->groots, t->adl, t->tdl};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    if (t->ctr_h) (void)hipHostFree(t->ctr_h);
    for (hipEvent_t e : t->ev)
        if (e) (void)hipEventDestroy(e);
    delete t;
    g->tim = nullptr;
}

}  // namespace fgi

using namespace fgi;

extern "C" {

// fgi_timers_open and fgi_part_timers_open (part: a rank of a partition)
static fgi_status tm_open(fgi_graph* g, const fgi_timers_config* cfg, bool part, const char* what) {
    if (!g || !cfg || cfg->struct_size < sizeof(fgi_timers_config)) return FGI_EINVAL;
    if (g->failed) return set_err(g, FGI_ESTATE, "%s: the graph is poisoned; fgi_restore or fgi_destroy", what);
    if (!part && (g->part || g->world > 1))
        return set_err(g, FGI_ENOTSUP, "fgi_timers_open: the delay timers serve a single device, not a partition "
                                       "(fgi_part_timers_open)");
    if (part && !g->part)
        return set_err(g, FGI_ENOTSUP, "fgi_part_timers_open: not a partitioned graph (fgi_timers_open)");
    if (g->tim) return set_err(g, FGI_ESTATE, "%s: the graph's timers are open", what);
    hipSetDevice(g->device);
    if (g->aw[0].busy || g->aw[1].busy) FGI_TRY(drain_async(g));
    Timers* t = new Timers();
    g->tim = t;
    t->part = part;
    t->now = cfg->now;
    t->default_delay = cfg->default_delay;
    hipStream_t s = g->stream;
    if (hipMalloc(reinterpret_cast<void**>(&t->dly), (size_t)g->ext_handles * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&t->ent), (size_t)g->ext_handles * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&t->ctr), kTWords * 8) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&t->ctr_h), kTWords * 8, hipHostMallocDefault) != hipSuccess ||
        hipEventCreate(&t->ev[0]) != hipSuccess || hipEventCreate(&t->ev[1]) != hipSuccess) {
        timers_destroy(g);
        return set_err(g, FGI_ENOMEM, "the timer table of %u handles", g->ext_handles);
    }
    memset(t->ctr_h, 0, kTWords * 8);
    fgi_status st = hip_check(g, hipMemsetAsync(t->dly, 0, (size_t)g->ext_handles * 4, s), "hipMemsetAsync");
    if (st == FGI_OK) st = hip_check(g, hipMemsetAsync(t->ent, 0xFF, (size_t)g->ext_handles * 4, s), "hipMemsetAsync");
    if (st == FGI_OK) st = hip_check(g, hipMemsetAsync(t->ctr, 0, kTWords * 8, s), "hipMemsetAsync");
    if (st == FGI_OK) st = tm_reserve(g);
    if (st == FGI_OK) st = flush_vis(g);
    // a populated graph: every node already Consistent with DelayStarted, in one pass over the handles
    if (st == FGI_OK && g->nodes_written) {
        tm_arm_all(g);
        st = tm_sync(g, what);
    }
    if (st != FGI_OK) timers_destroy(g);
    return st;
}

fgi_status fgi_timers_open(fgi_graph* g, const fgi_timers_config* cfg) { return tm_open(g, cfg, false, "fgi_timers_open"); }

fgi_status fgi_timers_close(fgi_graph* g) {
    if (!g) return FGI_EINVAL;
    FGI_TRY(tm_usable(g, "fgi_timers_close"));
    FGI_HIP(g, hipStreamSynchronize(g->stream));
    timers_destroy(g);
    return FGI_OK;
}

// delay[i] as a code of the table of distinct delays, which is uploaded again if it gained a delay
static fgi_status tm_encode(fgi_graph* g, const char* what, uint32_t n, const uint64_t* delay, std::vector<uint32_t>& code) {
    Timers* t = g->tim;
    code.resize(n);
    const size_t known = t->dtab_h.size();
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t d = delay[i];
        if (d == 0 || d == FGI_TIMER_NEVER) {
            code[i] = d ? kCodeNever : 0u;
            continue;
        }
        auto it = t->dcode.find(d);
        if (it == t->dcode.end()) {
            if (t->dtab_h.size() + 2 >= kClaim) return set_err(g, FGI_ENOMEM, "%s: too many distinct delays", what);
            t->dtab_h.push_back(d);
            it = t->dcode.emplace(d, (uint32_t)t->dtab_h.size()).first;
        }
        code[i] = it->second;
    }
    hipStream_t s = g->stream;
    if (t->dtab_h.size() != known) {   // the table of distinct delays, whole (it is short: one entry per compute method)
        if (t->dtab_cap < t->dtab_h.size()) FGI_HIP(g, hipStreamSynchronize(s));   // its readers are done before it is replaced
        FGI_TRY(grow(g, &t->dtab, &t->dtab_cap, std::max<uint64_t>(2 * t->dtab_h.size(), 64), "the timers' delay table"));
        FGI_HIP(g, hipMemcpyAsync(t->dtab, t->dtab_h.data(), t->dtab_h.size() * 8, hipMemcpyHostToDevice, s));
    }
    return FGI_OK;
}

// handle[i] (distinct, in range) takes delay[i]: what fgi_timers_set_delay and fgi_part_timers_set_delay share
static fgi_status tm_set_delay(fgi_graph* g, const char* what, uint32_t n, const uint32_t* handle, const uint64_t* delay) {
    Timers* t = g->tim;
    std::vector<uint32_t> code;
    FGI_TRY(tm_encode(g, what, n, delay, code));
    hipStream_t s = g->stream;
    FGI_TRY(tm_upload(g, 2, n));
    FGI_HIP(g, hipMemcpyAsync(t->up, handle, (size_t)n * 4, hipMemcpyHostToDevice, s));
    FGI_HIP(g, hipMemcpyAsync(t->up + n, code.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_tm_set_delay, dim3((n + kTBlock - 1) / kTBlock), dim3(kTBlock), 0, s, t->dly, n, (const uint32_t*)t->up,
                       (const uint32_t*)(t->up + n), g->ext_slots, t->ctr);
    FGI_TRY(tm_sync(g, what));
    // the entries stored now (a slot that lost its code may hold one), the coded slots, the detached handles
    // (and the slots with an auto or transient-error code: counted apart, so a slot with both kinds counts twice)
    t->holders = std::max<uint64_t>(t->holders, tm_stored(t) + t->ctr_h[kTCoded] + t->ctr_h[kTCodedA] + g->n_detached);
    return tm_reserve(g);
}

fgi_status fgi_timers_set_delay(fgi_graph* g, uint32_t n, const uint32_t* handle, const uint64_t* delay) {
    if (!g || (n && (!handle || !delay))) return FGI_EINVAL;
    if (g->part)
        return set_err(g, FGI_ENOTSUP, "fgi_timers_set_delay: a partition's slots are global ids (fgi_part_timers_set_delay)");
    FGI_TRY(tm_usable(g, "fgi_timers_set_delay"));
    for (uint32_t i = 0; i < n; ++i)
        if (handle[i] >= g->ext_handles)
            return set_err(g, FGI_EINVAL, "fgi_timers_set_delay: handle %u out of range at %u", handle[i], i);
    if (!n) return FGI_OK;
    {
        std::vector<uint32_t> sorted(handle, handle + n);
        std::sort(sorted.begin(), sorted.end());
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end()) return set_err(g, FGI_EINVAL, "fgi_timers_set_delay: handle %u listed twice", *dup);
    }
    return tm_set_delay(g, "fgi_timers_set_delay", n, handle, delay);
}

fgi_status fgi_timers_set_now(fgi_graph* g, uint64_t now) {
    if (!g) return FGI_EINVAL;
    FGI_TRY(tm_usable(g, "fgi_timers_set_now"));
    if (now < g->tim->now)
        return set_err(g, FGI_EINVAL, "fgi_timers_set_now: %llu is before the clock (%llu)", (unsigned long long)now,
                       (unsigned long long)g->tim->now);
    g->tim->now = now;
    return FGI_OK;
}

// The due pass at the clock t->now and its wait; the fired list sorted ascending at t->fired + t->fired_cap
// (*n_fired entries: handles, or on a rank the host's global slot ids). On a rank the fired detached handles,
// ascending, are left in t->fdet. A pool without entries launches nothing.
static fgi_status tm_due_pass(fgi_graph* g, const char* what, uint64_t* n_fired) {
    Timers* t = g->tim;
    *n_fired = 0;
    t->fdet.clear();
    const uint64_t top = tm_top(t);
    if (!top) return FGI_OK;
    hipStream_t s = g->stream;
    FGI_TRY(flush_vis(g));
    if (t->fired_cap < top) {
        dfree(t->fired);
        t->fired_cap = 0;
        FGI_TRY(dmalloc(g, &t->fired, (t->part ? 3 : 2) * t->cap));
        t->fired_cap = t->cap;
    }
    FGI_HIP(g, hipMemsetAsync(t->ctr + kTNewTop, 0, 2 * 8, s));   // kTNewTop, kTFiredN
    if (t->part) FGI_HIP(g, hipMemsetAsync(t->ctr + kTFiredD, 0, 8, s));
    FGI_HIP(g, hipEventRecord(t->ev[0], s));
    if (t->part)
        hipLaunchKernelGGL(k_tm_due_part, dim3(tgrid(top)), dim3(kTBlock), 0, s, tm_tab(g), tm_part(g), t->rec[1], t->fired,
                           t->fired + 2 * t->fired_cap, t->fired_cap);
    else
        hipLaunchKernelGGL(k_tm_due, dim3(tgrid(top)), dim3(kTBlock), 0, s, tm_tab(g), t->rec[1], t->fired, t->fired_cap);
    hipLaunchKernelGGL(k_tm_commit, dim3(1), dim3(64), 0, s, t->ctr);
    FGI_HIP(g, hipEventRecord(t->ev[1], s));
    std::swap(t->rec[0], t->rec[1]);
    t->tomb_ub = 0;
    FGI_TRY(tm_sync(g, what));
    float ms = 0;
    t->last_ms = hipEventElapsedTime(&ms, t->ev[0], t->ev[1]) == hipSuccess ? ms : 0.0;
    const uint64_t n = std::min<uint64_t>(t->ctr_h[kTFiredN], t->fired_cap);
    if (n > 0xFFFFFFFFull) return set_err(g, FGI_ECAPACITY, "%s: %llu roots", what, (unsigned long long)n);
    if (n) {   // ascending: the roots of one wave
        Tmp tt;
        size_t tb = 0;
        uint32_t* roots = t->fired + t->fired_cap;
        FGI_HIP(g, rocprim::radix_sort_keys(nullptr, tb, t->fired, roots, (size_t)n, 0, 32, s));
        void* tmp;
        FGI_TRY(tmalloc(g, tt, reinterpret_cast<char**>(&tmp), tb));
        FGI_HIP(g, rocprim::radix_sort_keys(tmp, tb, t->fired, roots, (size_t)n, 0, 32, s));
    }
    if (t->part) {   // few: a displaced node whose timer ran out before its host released it
        const uint64_t nd = std::min<uint64_t>(t->ctr_h[kTFiredD], t->fired_cap);
        t->fdet.resize(nd);
        if (nd) {
            FGI_HIP(g, hipMemcpyAsync(t->fdet.data(), t->fired + 2 * t->fired_cap, nd * 4, hipMemcpyDeviceToHost, s));
            FGI_HIP(g, hipStreamSynchronize(s));
            std::sort(t->fdet.begin(), t->fdet.end());
        }
    }
    *n_fired = n;
    return FGI_OK;
}

// the fired roots' `immediately` flags: n ones
static fgi_status tm_ones(fgi_graph* g, uint64_t n) {
    Timers* t = g->tim;
    if (t->imm_cap >= n) return FGI_OK;
    FGI_TRY(grow(g, &t->imm, &t->imm_cap, std::max<uint64_t>(n, 4096), "the fired roots' flags"));
    FGI_HIP(g, hipMemsetAsync(t->imm, 1, t->imm_cap, g->stream));
    return FGI_OK;
}

fgi_status fgi_timers_run_due(fgi_graph* g, uint64_t now, uint32_t* out_ids, uint64_t cap, uint64_t* out_n, uint64_t* out_fired,
                              fgi_wave_stats* stats) {
    if (!g) return FGI_EINVAL;
    if (out_n) *out_n = 0;
    if (out_fired) *out_fired = 0;
    if (g->part)   // never the single-device wave on a rank
        return set_err(g, FGI_ENOTSUP, "fgi_timers_run_due: a partition's tick is a collective (fgi_part_timers_run_due)");
    FGI_TRY(tm_usable(g, "fgi_timers_run_due"));
    Timers* t = g->tim;
    if (now < t->now)
        return set_err(g, FGI_EINVAL, "fgi_timers_run_due: %llu is before the clock (%llu)", (unsigned long long)now,
                       (unsigned long long)t->now);
    FGI_TRY(tm_sync(g, "fgi_timers_run_due"));
    t->now = now;
    uint64_t n_fired = 0;
    FGI_TRY(tm_due_pass(g, "fgi_timers_run_due", &n_fired));
    if (out_fired) *out_fired = n_fired;
    if (!n_fired) return FGI_OK;
    hipStream_t s = g->stream;
    // the fired handles ascending: the roots of one wave, every one `immediately`
    uint32_t* roots = t->fired + t->fired_cap;
    FGI_TRY(tm_ones(g, n_fired));
    ++t->runs;
    FGI_TRY(run_wave(g, (uint32_t)n_fired, roots, t->imm, stats, true, out_ids ? WaveOut::kIds : WaveOut::kCount));
    const uint64_t n = g->last_wave_n;
    if (out_n) *out_n = n;
    if (!out_ids) return FGI_OK;
    if (n > cap) return FGI_ECAPACITY;   // the wave has run: fgi_last_wave_ids
    FGI_TRY(ensure_ids(g));
    if (n) FGI_HIP(g, hipMemcpyAsync(out_ids, g->inv_cur ? g->inv_cur : g->inv, n * 4, hipMemcpyDeviceToHost, s));
    FGI_HIP(g, hipStreamSynchronize(s));
    return FGI_OK;
}

fgi_status fgi_timers_next_due(fgi_graph* g, uint64_t* out_due, uint64_t* out_stored) {
    if (!g || !out_due) return FGI_EINVAL;
    *out_due = FGI_TIMER_NONE;
    if (out_stored) *out_stored = 0;
    FGI_TRY(tm_usable(g, "fgi_timers_next_due"));
    Timers* t = g->tim;
    hipStream_t s = g->stream;
    FGI_HIP(g, hipMemsetAsync(t->ctr + kTMin, 0xFF, 8, s));
    // (the grid follows the capacity: the count is on the device)
    hipLaunchKernelGGL(k_tm_min, dim3(tgrid(std::min<uint64_t>(t->cap, 1ull << 16))), dim3(kTBlock), 0, s,
                       (const TimerRec*)t->rec[0], t->cap, g->ext_handles, t->ctr);
    FGI_TRY(tm_sync(g, "fgi_timers_next_due"));
    *out_due = t->ctr_h[kTMin];
    if (out_stored) *out_stored = tm_stored(t);
    return FGI_OK;
}

fgi_status fgi_timers_stats_get(fgi_graph* g, fgi_timer_stats* out) {
    if (!g || !out) return FGI_EINVAL;
    memset(out, 0, sizeof(*out));
    if (!g->tim) return FGI_OK;
    FGI_TRY(tm_usable(g, "fgi_timers_stats_get"));
    FGI_TRY(tm_sync(g, "fgi_timers_stats_get"));
    const Timers* t = g->tim;
    out->stored = tm_stored(t);
    out->armed = t->ctr_h[kTArmed];
    out->fired = t->ctr_h[kTFired];
    out->dropped = t->ctr_h[kTDropped];
    out->moved = t->ctr_h[kTMoved];
    out->runs = t->runs;
    out->last_kernel_ms = t->last_ms;
    return FGI_OK;
}

// fgi_timers_list and fgi_timers_list_ex (kind nullable)
static fgi_status tm_list(fgi_graph* g, const char* what, uint32_t* handle, uint64_t* version, uint64_t* due, uint8_t* kind,
                          uint64_t cap, uint64_t* out_n) {
    if (!g) return FGI_EINVAL;
    if (out_n) *out_n = 0;
    FGI_TRY(tm_usable(g, what));
    FGI_TRY(tm_sync(g, what));
    const Timers* t = g->tim;
    const uint64_t top = tm_top(t);
    std::vector<TimerRec> recs(top);
    if (top) {
        FGI_HIP(g, hipMemcpyAsync(recs.data(), t->rec[0], top * sizeof(TimerRec), hipMemcpyDeviceToHost, g->stream));
        FGI_HIP(g, hipStreamSynchronize(g->stream));
    }
    recs.erase(std::remove_if(recs.begin(), recs.end(), [&](const TimerRec& r) { return r.handle >= g->ext_handles; }), recs.end());
    std::sort(recs.begin(), recs.end(), [](const TimerRec& a, const TimerRec& b) { return a.handle < b.handle; });
    if (out_n) *out_n = recs.size();
    if (!handle && !version && !due && !kind) return FGI_OK;
    if (recs.size() > cap)
        return set_err(g, FGI_ECAPACITY, "%s: %llu entries, the buffers hold %llu", what, (unsigned long long)recs.size(),
                       (unsigned long long)cap);
    for (size_t i = 0; i < recs.size(); ++i) {
        if (handle) handle[i] = recs[i].handle;
        if (version) version[i] = recs[i].version;
        if (due) due[i] = recs[i].due;
        if (kind) kind[i] = (uint8_t)(recs[i].pad & kKindAuto);
    }
    return FGI_OK;
}

fgi_status fgi_timers_list(fgi_graph* g, uint32_t* handle, uint64_t* version, uint64_t* due, uint64_t cap, uint64_t* out_n) {
    return tm_list(g, "fgi_timers_list", handle, version, due, nullptr, cap, out_n);
}

// ---- auto-invalidation (C-ABI 0.13) -------------------------------------------------------------------------

// what the calls of the section check first: never on a partition, then open timers on a usable graph
static fgi_status tm_auto_usable(fgi_graph* g, const char* what, bool need_auto) {
    if (g->part || g->world > 1)
        return set_err(g, FGI_ENOTSUP, "%s: auto-invalidation timers serve a single device, not a partition", what);
    FGI_TRY(tm_usable(g, what));
    if (need_auto && !g->tim->autos)
        return set_err(g, FGI_ESTATE, "%s: auto-invalidation is not open (fgi_timers_auto_open)", what);
    return FGI_OK;
}

// handles in range and distinct
static fgi_status tm_check_handles(fgi_graph* g, const char* what, uint32_t n, const uint32_t* handle) {
    for (uint32_t i = 0; i < n; ++i)
        if (handle[i] >= g->ext_handles) return set_err(g, FGI_EINVAL, "%s: handle %u out of range at %u", what, handle[i], i);
    std::vector<uint32_t> sorted(handle, handle + n);
    std::sort(sorted.begin(), sorted.end());
    const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
    if (dup != sorted.end()) return set_err(g, FGI_EINVAL, "%s: handle %u listed twice", what, *dup);
    return FGI_OK;
}

// what fgi_timers_auto_open and fgi_part_timers_auto_open share, on open timers
static fgi_status tm_auto_open(fgi_graph* g, const char* what, const fgi_timers_auto_config* cfg) {
    Timers* t = g->tim;
    if (t->autos) return set_err(g, FGI_ESTATE, "%s: auto-invalidation is open", what);
    hipStream_t s = g->stream;
    DevOwn<uint32_t> a, b;   // until they are installed
    if (hipMalloc(reinterpret_cast<void**>(&a.p), (size_t)g->ext_handles * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&b.p), (size_t)g->ext_handles * 4) != hipSuccess)
        return set_err(g, FGI_ENOMEM, "the auto-invalidation delays of %u handles", g->ext_handles);
    FGI_HIP(g, hipMemsetAsync(a.p, 0, (size_t)g->ext_handles * 4, s));
    FGI_HIP(g, hipMemsetAsync(b.p, 0, (size_t)g->ext_handles * 4, s));
    FGI_HIP(g, hipStreamSynchronize(s));
    t->adl = a.release();
    t->tdl = b.release();
    t->def_auto = cfg->default_auto_delay;
    t->def_trans = cfg->default_transient_delay;
    t->autos = true;
    return tm_reserve(g);
}

fgi_status fgi_timers_auto_open(fgi_graph* g, const fgi_timers_auto_config* cfg) {
    if (!g || !cfg || cfg->struct_size < sizeof(fgi_timers_auto_config)) return FGI_EINVAL;
    FGI_TRY(tm_auto_usable(g, "fgi_timers_auto_open", false));
    return tm_auto_open(g, "fgi_timers_auto_open", cfg);
}

// handle[i] (distinct, in range) takes auto_delay[i] and transient_delay[i] (each nullable): what
// fgi_timers_set_auto_delay and fgi_part_timers_set_auto_delay share
static fgi_status tm_set_auto_delay(fgi_graph* g, const char* what, uint32_t n, const uint32_t* handle, const uint64_t* auto_delay,
                                    const uint64_t* transient_delay) {
    if (!n || (!auto_delay && !transient_delay)) return FGI_OK;
    Timers* t = g->tim;
    std::vector<uint32_t> ac, tc;
    if (auto_delay) FGI_TRY(tm_encode(g, what, n, auto_delay, ac));
    if (transient_delay) FGI_TRY(tm_encode(g, what, n, transient_delay, tc));
    hipStream_t s = g->stream;
    FGI_TRY(tm_upload(g, 3, n));
    FGI_HIP(g, hipMemcpyAsync(t->up, handle, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (auto_delay) FGI_HIP(g, hipMemcpyAsync(t->up + n, ac.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (transient_delay) FGI_HIP(g, hipMemcpyAsync(t->up + 2 * (size_t)n, tc.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_tm_set_auto, dim3((n + kTBlock - 1) / kTBlock), dim3(kTBlock), 0, s, t->adl, t->tdl, n,
                       (const uint32_t*)t->up, auto_delay ? (const uint32_t*)(t->up + n) : (const uint32_t*)nullptr,
                       transient_delay ? (const uint32_t*)(t->up + 2 * (size_t)n) : (const uint32_t*)nullptr, g->ext_slots, t->ctr);
    FGI_TRY(tm_sync(g, what));
    t->holders = std::max<uint64_t>(t->holders, tm_stored(t) + t->ctr_h[kTCoded] + t->ctr_h[kTCodedA] + g->n_detached);
    return tm_reserve(g);
}

fgi_status fgi_timers_set_auto_delay(fgi_graph* g, uint32_t n, const uint32_t* handle, const uint64_t* auto_delay,
                                     const uint64_t* transient_delay) {
    const char* const what = "fgi_timers_set_auto_delay";
    if (!g || (n && !handle)) return FGI_EINVAL;
    FGI_TRY(tm_auto_usable(g, what, true));
    FGI_TRY(tm_check_handles(g, what, n, handle));
    return tm_set_auto_delay(g, what, n, handle, auto_delay, transient_delay);
}

fgi_status fgi_timers_start_auto(fgi_graph* g, uint32_t n, const uint32_t* handle, const uint8_t* transient) {
    const char* const what = "fgi_timers_start_auto";
    if (!g || (n && !handle)) return FGI_EINVAL;
    FGI_TRY(tm_auto_usable(g, what, true));
    FGI_TRY(tm_check_handles(g, what, n, handle));
    return timers_arm_auto(g, n, handle, nullptr, nullptr, nullptr, transient);
}

fgi_status fgi_timers_auto_stats_get(fgi_graph* g, fgi_timer_auto_stats* out) {
    if (!g || !out) return FGI_EINVAL;
    memset(out, 0, sizeof(*out));
    if (g->part || g->world > 1)
        return set_err(g, FGI_ENOTSUP, "fgi_timers_auto_stats_get: auto-invalidation timers serve a single device, not a partition");
    if (!g->tim || !g->tim->autos) return FGI_OK;
    FGI_TRY(tm_usable(g, "fgi_timers_auto_stats_get"));
    FGI_TRY(tm_sync(g, "fgi_timers_auto_stats_get"));
    const Timers* t = g->tim;
    out->armed_auto = t->ctr_h[kTArmedA];
    out->merged = t->ctr_h[kTMerged];
    out->fired_auto = t->ctr_h[kTFiredA];
    return FGI_OK;
}

fgi_status fgi_timers_list_ex(fgi_graph* g, uint32_t* handle, uint64_t* version, uint64_t* due, uint8_t* kind, uint64_t cap,
                              uint64_t* out_n) {
    if (!g) return FGI_EINVAL;
    if (out_n) *out_n = 0;
    if (g->part || g->world > 1)
        return set_err(g, FGI_ENOTSUP, "fgi_timers_list_ex: auto-invalidation timers serve a single device, not a partition");
    return tm_list(g, "fgi_timers_list_ex", handle, version, due, kind, cap, out_n);
}

// ---- per rank of a partition (C-ABI 0.12) ------------------------------------------------------------------

fgi_status fgi_part_timers_open(fgi_graph* g, const fgi_timers_config* cfg) { return tm_open(g, cfg, true, "fgi_part_timers_open"); }

fgi_status fgi_part_timers_set_delay(fgi_graph* g, uint32_t n, const uint32_t* slot, const uint64_t* delay) {
    if (!g || (n && (!slot || !delay))) return FGI_EINVAL;
    PartView pv{};
    if (!g->part || !part_view(g, &pv))
        return set_err(g, FGI_ENOTSUP, "fgi_part_timers_set_delay: not a partitioned graph (fgi_timers_set_delay)");
    FGI_TRY(tm_usable(g, "fgi_part_timers_set_delay"));
    for (uint32_t i = 0; i < n; ++i)
        if (slot[i] >= pv.n_global)
            return set_err(g, FGI_EINVAL, "fgi_part_timers_set_delay: slot %u of %u at %u", slot[i], pv.n_global, i);
    if (!n) return FGI_OK;
    {
        std::vector<uint32_t> sorted(slot, slot + n);
        std::sort(sorted.begin(), sorted.end());
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end()) return set_err(g, FGI_EINVAL, "fgi_part_timers_set_delay: slot %u listed twice", *dup);
    }
    // the rank's share, as its local handles (a slot below base wraps past n_local)
    std::vector<uint32_t> h;
    std::vector<uint64_t> d;
    for (uint32_t i = 0; i < n; ++i)
        if (slot[i] - pv.base < pv.n_local) {
            h.push_back(slot[i] - pv.base);
            d.push_back(delay[i]);
        }
    if (h.empty()) return FGI_OK;
    return tm_set_delay(g, "fgi_part_timers_set_delay", (uint32_t)h.size(), h.data(), d.data());
}

fgi_status fgi_part_timers_run_due(fgi_graph* g, uint64_t now, uint32_t* out_ids, uint64_t cap, uint64_t* out_n,
                                   uint64_t* out_fired, uint64_t* out_fired_detached, fgi_wave_stats* stats) {
    const char* const what = "fgi_part_timers_run_due";
    if (!g) return FGI_EINVAL;
    if (out_n) *out_n = 0;
    if (out_fired) *out_fired = 0;
    if (out_fired_detached) *out_fired_detached = 0;
    PartView pv{};
    if (!g->part || !part_view(g, &pv)) return set_err(g, FGI_ENOTSUP, "%s: not a partitioned graph (fgi_timers_run_due)", what);
    hipSetDevice(g->device);
    Timers* t = g->tim;
    // Agreement first: every rank's verdict and its `now` travel with the call's first collective, so a tick
    // that any rank refuses removes no entry anywhere and every rank returns the same status.
    enum : uint64_t { kOk = 0, kClosed, kPoisoned, kClock };
    const uint64_t mine[2] = {g->failed ? kPoisoned : !t ? kClosed : now < t->now ? kClock : kOk, now};
    uint64_t all[8 * 2];
    FGI_TRY(part_allgather_words(g, mine, 2, all));
    for (uint32_t q = 0; q < pv.world; ++q)
        if (all[2 * q] == kClosed || all[2 * q] == kPoisoned)
            return set_err(g, FGI_ESTATE, "%s: rank %u %s", what, q,
                           all[2 * q] == kClosed ? "has not opened its timers (fgi_part_timers_open)"
                                                 : "is poisoned; fgi_restore or fgi_destroy");
    for (uint32_t q = 0; q < pv.world; ++q) {
        if (all[2 * q] == kClock)
            return set_err(g, FGI_EINVAL, "%s: %llu is before the clock of rank %u", what, (unsigned long long)now, q);
        if (all[2 * q + 1] != all[1])
            return set_err(g, FGI_EINVAL, "%s: rank %u ticks at %llu, rank 0 at %llu", what, q, (unsigned long long)all[2 * q + 1],
                           (unsigned long long)all[1]);
    }
    // the due pass on the rank's own pool; its outcome and the count of its roots travel together, so a rank
    // whose pass failed takes every rank out of the call before the lists move
    uint64_t n_mine = 0;
    auto pass = [&]() -> fgi_status {
        if (g->aw[0].busy || g->aw[1].busy) FGI_TRY(drain_async(g));
        FGI_TRY(tm_sync(g, what));
        t->now = now;
        return tm_due_pass(g, what, &n_mine);
    };
    const fgi_status ps = pass();
    const uint64_t cnt[2] = {(uint64_t)ps, n_mine};
    FGI_TRY(part_allgather_words(g, cnt, 2, all));
    if (ps != FGI_OK) return ps;
    uint64_t bytes[8], total = 0;
    for (uint32_t q = 0; q < pv.world; ++q) {
        if (all[2 * q] != FGI_OK) return set_err(g, FGI_ESTATE, "%s: the due pass of rank %u failed", what, q);
        bytes[q] = all[2 * q + 1] * 4;
        total += all[2 * q + 1];
    }
    const uint64_t n_det = t->fdet.size();
    if (out_fired) *out_fired = n_mine + n_det;
    if (out_fired_detached) *out_fired_detached = n_det;
    if (!total) return FGI_OK;   // no wave: every rank's last-wave results stay
    if (total > pv.n_global) return set_err(g, FGI_EDEVICE, "%s: %llu roots of %u slots", what, (unsigned long long)total, pv.n_global);
    // Ranks own contiguous ranges of the host's numbering, so the ranks' ascending lists in rank order are the
    // ascending global root list, the same on every rank
    FGI_TRY(grow(g, &t->groots, &t->groots_cap, std::max<uint64_t>(total, 4096), "the gathered timer roots"));
    FGI_TRY(tm_ones(g, total));
    FGI_TRY(part_allgatherv(g, t->fired + t->fired_cap, bytes, t->groots));
    ++t->runs;
    // one partitioned wave, every root `immediately`: mapped to codes, marked, driven and armed (at `now`) as
    // fgi_part_invalidate's
    FGI_TRY(fgi_part_invalidate(g, (uint32_t)total, t->groots, t->imm, nullptr, stats));
    return fgi_part_last_wave_ids(g, out_ids, cap, out_n);   // a short cap: FGI_ECAPACITY, the wave has run
}

fgi_status fgi_part_timers_fired_detached(fgi_graph* g, uint32_t* out_handles, uint64_t cap, uint64_t* out_n) {
    if (!g) return FGI_EINVAL;
    if (out_n) *out_n = 0;
    if (!g->part) return set_err(g, FGI_ENOTSUP, "fgi_part_timers_fired_detached: not a partitioned graph");
    FGI_TRY(tm_usable(g, "fgi_part_timers_fired_detached"));
    const std::vector<uint32_t>& f = g->tim->fdet;
    if (out_n) *out_n = f.size();
    if (!out_handles) return FGI_OK;
    if (f.size() > cap)
        return set_err(g, FGI_ECAPACITY, "fgi_part_timers_fired_detached: %llu handles, the buffer holds %llu",
                       (unsigned long long)f.size(), (unsigned long long)cap);
    if (!f.empty()) memcpy(out_handles, f.data(), f.size() * 4);
    return FGI_OK;
}

fgi_status fgi_part_local_timers_run_due(fgi_graph* const* gs, uint32_t p, uint64_t now, uint64_t* out_fired,
                                         uint64_t* out_fired_detached, fgi_wave_stats* stats) {
    return part_local_run(gs, p, [&](uint32_t r) {
        return fgi_part_timers_run_due(gs[r], now, nullptr, 0, nullptr, out_fired ? out_fired + r : nullptr,
                                       out_fired_detached ? out_fired_detached + r : nullptr, stats ? stats + r : nullptr);
    });
}

// ---- auto-invalidation per rank of a partition (C-ABI 0.14) -------------------------------------------------

// what the calls of the section check first: a rank of a partition, then open timers on a usable graph
static fgi_status tm_part_auto_usable(fgi_graph* g, const char* what, bool need_auto, PartView* pv) {
    if (!g->part || !part_view(g, pv))
        return set_err(g, FGI_ENOTSUP, "%s: not a partitioned graph (a single device has the fgi_timers_* call)", what);
    FGI_TRY(tm_usable(g, what));
    if (need_auto && !g->tim->autos)
        return set_err(g, FGI_ESTATE, "%s: auto-invalidation is not open (fgi_part_timers_auto_open)", what);
    return FGI_OK;
}

// global slots in range and distinct
static fgi_status tm_check_slots(fgi_graph* g, const char* what, const PartView& pv, uint32_t n, const uint32_t* slot) {
    for (uint32_t i = 0; i < n; ++i)
        if (slot[i] >= pv.n_global) return set_err(g, FGI_EINVAL, "%s: slot %u of %u at %u", what, slot[i], pv.n_global, i);
    std::vector<uint32_t> sorted(slot, slot + n);
    std::sort(sorted.begin(), sorted.end());
    const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
    if (dup != sorted.end()) return set_err(g, FGI_EINVAL, "%s: slot %u listed twice", what, *dup);
    return FGI_OK;
}

fgi_status fgi_part_timers_auto_open(fgi_graph* g, const fgi_timers_auto_config* cfg) {
    if (!g || !cfg || cfg->struct_size < sizeof(fgi_timers_auto_config)) return FGI_EINVAL;
    PartView pv{};
    FGI_TRY(tm_part_auto_usable(g, "fgi_part_timers_auto_open", false, &pv));
    return tm_auto_open(g, "fgi_part_timers_auto_open", cfg);
}

fgi_status fgi_part_timers_set_auto_delay(fgi_graph* g, uint32_t n, const uint32_t* slot, const uint64_t* auto_delay,
                                          const uint64_t* transient_delay) {
    const char* const what = "fgi_part_timers_set_auto_delay";
    if (!g || (n && !slot)) return FGI_EINVAL;
    PartView pv{};
    FGI_TRY(tm_part_auto_usable(g, what, true, &pv));
    FGI_TRY(tm_check_slots(g, what, pv, n, slot));
    // the rank's share, as its local handles (a slot below base wraps past n_local)
    std::vector<uint32_t> h;
    std::vector<uint64_t> ad, td;
    for (uint32_t i = 0; i < n; ++i)
        if (slot[i] - pv.base < pv.n_local) {
            h.push_back(slot[i] - pv.base);
            if (auto_delay) ad.push_back(auto_delay[i]);
            if (transient_delay) td.push_back(transient_delay[i]);
        }
    return tm_set_auto_delay(g, what, (uint32_t)h.size(), h.data(), auto_delay ? ad.data() : nullptr,
                             transient_delay ? td.data() : nullptr);
}

fgi_status fgi_part_timers_start_auto(fgi_graph* g, uint32_t n, const uint32_t* slot, const uint8_t* transient) {
    const char* const what = "fgi_part_timers_start_auto";
    if (!g || (n && !slot)) return FGI_EINVAL;
    PartView pv{};
    FGI_TRY(tm_part_auto_usable(g, what, true, &pv));
    FGI_TRY(tm_check_slots(g, what, pv, n, slot));
    if (!n) return FGI_OK;
    // the whole list goes up: the kernel skips the slots of other ranks, and their transient flags with them
    Timers* t = g->tim;
    hipStream_t s = g->stream;
    const uint64_t bw = ((uint64_t)n + 3) / 4;
    FGI_TRY(tm_upload(g, 1, (uint64_t)n + bw));
    uint8_t* dt = reinterpret_cast<uint8_t*>(t->up + n);
    FGI_HIP(g, hipMemcpyAsync(t->up, slot, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (transient) FGI_HIP(g, hipMemcpyAsync(dt, transient, n, hipMemcpyHostToDevice, s));
    FGI_TRY(timers_arm_auto_part(g, n, t->up, nullptr, transient ? dt : nullptr));
    return tm_sync(g, what);
}

fgi_status fgi_part_timers_auto_stats_get(fgi_graph* g, fgi_timer_auto_stats* out) {
    if (!g || !out) return FGI_EINVAL;
    memset(out, 0, sizeof(*out));
    if (!g->part) return set_err(g, FGI_ENOTSUP, "fgi_part_timers_auto_stats_get: not a partitioned graph (fgi_timers_auto_stats_get)");
    if (!g->tim || !g->tim->autos) return FGI_OK;
    FGI_TRY(tm_usable(g, "fgi_part_timers_auto_stats_get"));
    FGI_TRY(tm_sync(g, "fgi_part_timers_auto_stats_get"));
    const Timers* t = g->tim;
    out->armed_auto = t->ctr_h[kTArmedA];
    out->merged = t->ctr_h[kTMerged];
    out->fired_auto = t->ctr_h[kTFiredA];
    return FGI_OK;
}

fgi_status fgi_part_timers_list_ex(fgi_graph* g, uint32_t* handle, uint64_t* version, uint64_t* due, uint8_t* kind, uint64_t cap,
                                   uint64_t* out_n) {
    if (!g) return FGI_EINVAL;
    if (out_n) *out_n = 0;
    if (!g->part) return set_err(g, FGI_ENOTSUP, "fgi_part_timers_list_ex: not a partitioned graph (fgi_timers_list_ex)");
    return tm_list(g, "fgi_part_timers_list_ex", handle, version, due, kind, cap, out_n);
}

}  // extern "C"
