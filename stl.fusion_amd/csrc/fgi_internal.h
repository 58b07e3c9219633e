// fgi_internal.h — device data layout and shared helpers of the fgi engine (gfx950 only).
//
// HBM layout, one entry per handle h in [0, n_slots + n_detached):
//   node[h]    u64  packed node word: bits 0-55 version (LTag; 0 = no node), bits 56-57
//                   ConsistencyState, bit 58 InvalidateOnSetOutput, bit 59 InvalidationDelayStarted,
//                   bit 60 hasDelay. One 64-bit CAS checks the version and moves the state.
//   row_off[h] u64  start of h's `_usedBy` row in the edge pool
//   row_len[h] u32  entries in the row (logical length is 0 once the node is Invalidated)
//   row_cap[h] u32  reserved entries (appends go in place while len < cap)
//   used_cnt[h]u32  |_used| of the node (forward links created while it was Computing)
// Edge pool (structure of arrays, rows are contiguous runs):
//   pool_col[p] u32 dependant slot (ComputedInput of the `_usedBy` entry)
//   pool_tag[p] u64 dependant version at capture time (LTag of the `_usedBy` entry)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/fgi.h"
#include "../../include/fgi_variants.h"

// Measurement variants (make variant-all -> libfgi_variants.so): the fused waves, the probe summary and
// the cooperative launch of streaming cascades, each measured slower than the shipping paths on MI355X
// (DESIGN.md §3, §7b). The shipping library leaves them out: their options return FGI_ENOTSUP.
#ifndef FGI_VARIANTS
#define FGI_VARIANTS 0
#endif

namespace fgi {

constexpr uint64_t kVMask = (1ull << 56) - 1;
constexpr int kStateShift = 56;
constexpr uint64_t kStateBits = 3ull << kStateShift;
constexpr uint64_t kW_IOSO = 1ull << 58;
constexpr uint64_t kW_DS = 1ull << 59;
constexpr uint64_t kW_HasDelay = 1ull << 60;
constexpr uint64_t kW_Computing = 0ull;
constexpr uint64_t kW_Consistent = 1ull << kStateShift;
constexpr uint64_t kW_Invalidated = 2ull << kStateShift;

__host__ __device__ inline uint32_t word_state(uint64_t w) { return (uint32_t)((w >> kStateShift) & 3u); }
__host__ __device__ inline bool word_is_current(uint64_t w) {
    return (w & kVMask) != 0 && word_state(w) != FGI_INVALIDATED;
}

// Host-visible state_flags <-> node word (canonical flags, fgi.h)
__host__ __device__ inline uint32_t word_to_flags(uint64_t w) {
    if ((w & kVMask) == 0) return 0;
    uint32_t st = word_state(w);
    uint32_t f = st;
    if (st == FGI_COMPUTING) {
        if (w & kW_IOSO) f |= FGI_F_INVALIDATE_ON_SET_OUTPUT;
        if (w & kW_DS) f |= FGI_F_INVALIDATION_DELAY_STARTED;
    } else if (st == FGI_CONSISTENT) {
        if (w & kW_DS) f |= FGI_F_INVALIDATION_DELAY_STARTED;
    }
    if (w & kW_HasDelay) f |= FGI_F_HAS_DELAY;
    return f;
}
__host__ __device__ inline uint64_t flags_to_word(uint64_t version, uint32_t f) {
    uint64_t w = (version & kVMask) | ((uint64_t)(f & 3u) << kStateShift);
    if (f & FGI_F_INVALIDATE_ON_SET_OUTPUT) w |= kW_IOSO;
    if (f & FGI_F_INVALIDATION_DELAY_STARTED) w |= kW_DS;
    if (f & FGI_F_HAS_DELAY) w |= kW_HasDelay;
    return w;
}

// The node word after a (non-immediate) visit: canonical, flags of an Invalidated node cleared
// (wave.hip's visits; view.hip reads unfolded visits through it).
__host__ __device__ inline unsigned long long visited_word(unsigned long long w) {
    if ((w & kVMask) == 0) return w;
    const uint32_t st = word_state(w);
    if (st == FGI_COMPUTING) return w | kW_IOSO;
    if (st == FGI_CONSISTENT)
        return (w & kW_HasDelay) ? (w | kW_DS) : ((w & (kVMask | kW_HasDelay)) | kW_Invalidated);
    return w;
}

// splitmix64 finaliser
__host__ __device__ inline uint64_t sm64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__host__ __device__ inline uint64_t synth_version(uint64_t seed, uint32_t slot) {
    return (sm64(seed ^ (uint64_t)slot) & ((1ull << 55) - 1)) | 1ull;
}

// R-MAT edge i of a (scale, seed) graph (oracle/synth.cpp): per level l,
// u = sm64(sm64(seed) ^ (i << 6 | l)) >> 11 against 0.57 / 0.76 / 0.95 * 2^53, endpoints scrambled by
// a bijection of [0, 2^scale)
__host__ __device__ inline uint32_t rmat_scramble(uint64_t x, uint32_t scale, uint64_t seed) {
    const uint64_t mask = (scale >= 64) ? ~0ull : ((1ull << scale) - 1);
    const uint64_t k1 = sm64(seed ^ 0xA5A5A5A5A5A5A5A5ull) | 1ull;
    const uint64_t k2 = sm64(seed ^ 0x5A5A5A5A5A5A5A5Aull) | 1ull;
    const uint64_t c = sm64(seed ^ 0x0123456789ABCDEFull);
    const uint32_t s1 = (scale + 1) / 2, s2 = scale / 2 ? scale / 2 : 1;
    x = (x * k1) & mask;
    x ^= x >> s1;
    x = (x + c) & mask;
    x = (x * k2) & mask;
    x ^= x >> s2;
    return (uint32_t)x;
}
__host__ __device__ inline void rmat_edge(uint64_t i, uint32_t scale, uint64_t seed, uint32_t* src, uint32_t* dst) {
    const uint64_t one = 1ull << 53;
    const uint64_t tA = one / 100 * 57, tAB = one / 100 * 76, tABC = one / 100 * 95;
    const uint64_t ks = sm64(seed);
    uint64_t s = 0, d = 0;
    for (uint32_t l = 0; l < scale; ++l) {
        const uint64_t u = sm64(ks ^ ((i << 6) | l)) >> 11;
        const uint64_t bit = 1ull << (scale - 1 - l);
        if (u >= tA) {
            if (u < tAB) d |= bit;
            else if (u < tABC) s |= bit;
            else {
                s |= bit;
                d |= bit;
            }
        }
    }
    *src = rmat_scramble(s, scale, seed);
    *dst = rmat_scramble(d, scale, seed);
}
// stale edge of the churn workloads (configs[3]): tag = version + 1
__host__ __device__ inline bool synth_stale(uint32_t stale_pct, uint64_t stale_seed, uint32_t src, uint32_t dst) {
    return stale_pct && (sm64(stale_seed ^ sm64(((uint64_t)src << 32) | dst)) % 100) < stale_pct;
}

// ---- wave bookkeeping -------------------------------------------------------------------------
constexpr int kRing = 64;               // per-level counters live in a ring (deep waves roll over)
constexpr int kBlock = 256;             // threads per block for the traversal kernels
constexpr int kEPT = 8;                 // edges per thread per chunk (largest chunk)
constexpr int kChunk = kBlock * kEPT;   // edges per expand chunk (largest chunk)
constexpr int kFine = 256;              // edges per fine chunk of the chunk map (cstart granularity);
                                        // a push level expands chunks of 1..kEPT fine chunks
constexpr uint32_t kStatBlocks = 8192;  // per-block statistics rows (grid limit of the hot kernels: 268M slots pull)
constexpr int kStatCols = 8;
constexpr int kPullTile = 1024;         // slots per pull tile (one block iteration of a pull level)
// A pull candidate's record (16 B, fgi_graph::cand and the survivor buffers): words x and y below, then
// the two list heads. x = slot relative to its pull block's first slot (15 bits: a block owns at most
// 32 tiles) | tail flag (the list has more than two entries) << 15 | low 16 bits of the row length << 16;
// y = high 4 bits of the row length | offset of the candidate's tail run from its block's base in
// fgi_graph::trun, in words << 4. A row length of kRecLenEsc or more is stored as kRecLenEsc (read
// row_len[slot] instead); a run at kRecNoOff words or more is stored as kRecNoOff (locate the list through
// uin_len / uin_off instead).
constexpr uint32_t kRecSlotBits = 15;
constexpr uint32_t kRecLenEsc = (1u << 20) - 1;
constexpr uint32_t kRecOffBits = 28;                      // FGI_OPT_RUN_OFFSET_BITS lowers the limit (tests)
constexpr uint32_t kRecNoOff = (1u << kRecOffBits) - 1;
__host__ __device__ inline void rec_encode(uint32_t rel, bool tail, uint32_t row_len, uint64_t run_off, uint64_t off_limit,
                                           uint32_t& x, uint32_t& y) {
    const uint32_t rl = row_len < kRecLenEsc ? row_len : kRecLenEsc;
    const uint32_t ro = (tail && run_off < off_limit && run_off < kRecNoOff) ? (uint32_t)run_off : kRecNoOff;
    x = rel | (tail ? 1u << kRecSlotBits : 0u) | (rl << 16);
    y = (rl >> 16) | (ro << 4);
}
struct CandRec {
    uint32_t rel;       // slot - the block's first slot
    bool tail;          // the list has more than two entries
    uint32_t row_len;   // kRecLenEsc: read row_len[slot]
    uint32_t run_off;   // kRecNoOff: no inline offset
};
__host__ __device__ inline CandRec rec_decode(uint32_t x, uint32_t y) {
    return CandRec{x & ((1u << kRecSlotBits) - 1), ((x >> kRecSlotBits) & 1u) != 0, (x >> 16) | ((y & 15u) << 16), y >> 4};
}
constexpr int kDoneGroups = 16;         // two-level completion counters (last-block epilogues)
constexpr int kDoneStride = 16;         // 128 B apart
#ifndef FGI_FINAL_BLOCKS
#define FGI_FINAL_BLOCKS 1024               // measurement builds: make variant-grid FINAL=<blocks> WPB=<words> INIT=<blocks>
#endif
#ifndef FGI_FINAL_WPB
#define FGI_FINAL_WPB 256
#endif
#ifndef FGI_INIT_BLOCKS
#define FGI_INIT_BLOCKS 2048
#endif
constexpr uint32_t kFinalBlocks = FGI_FINAL_BLOCKS; // grid of the final collect (invalidated bitmap -> list)
constexpr uint32_t kFinalWpb = FGI_FINAL_WPB;       // fewest 64-bit bitmap words per final-collect block
constexpr uint32_t kInitBlocks = FGI_INIT_BLOCKS;   // grid of k_wave_init
#ifndef FGI_SPIN_WAIT
#define FGI_SPIN_WAIT 1                     // measurement builds: make variant-nospin (stream synchronisation)
#endif
#ifndef FGI_HOT
#define FGI_HOT 524288                  // measurement builds: make variant-hot HOT=<n> (a multiple of 256)
#endif
constexpr uint32_t kHot = FGI_HOT;      // most hot list heads (pull probes through a snapshot of kHot / 8 B)
#ifndef FGI_LDS_HOT
#define FGI_LDS_HOT 4096                // measurement builds: make variant-ldshot LDSHOT=<words>
#endif
// hot snapshot words a pull block keeps in LDS (16 KB): 4,096 against 2,048 measured -1% on configs[1]
// and -2% on configs[2] with hub-first labels; 8,192 pulls faster still but its lower occupancy makes
// the push levels 4x slower (round 5, profiles/r12i_ldshot_ab.txt)
constexpr uint32_t kLdsHot = FGI_LDS_HOT;
// fewest hot heads: 8 KB, or what the LDS copy holds (a graph's count: build_candidates, hot_count)
#ifdef FGI_HOT_MIN
constexpr uint32_t kHotMin = FGI_HOT_MIN;   // measurement builds (variant-cpl HOTMIN=)
#else
constexpr uint32_t kHotMin = kLdsHot * 32 > 65536 ? kLdsHot * 32 : 65536;
#endif
// resident k_level blocks per CU: LDS-bound once the LDS snapshot passes 8 KB (160 KB per CU)
#ifdef FGI_LEVEL_OCC
constexpr uint32_t kLevelOcc = FGI_LEVEL_OCC;   // measurement builds (variant-cpl)
#else
constexpr uint32_t kLevelOcc = kLdsHot <= 2048 ? 5 : kLdsHot <= 4096 ? 4 : 3;
#endif
constexpr int kAccCount = 8;            // batch accumulators (fgi_run_batch; run_wave_coop's acc)
// A batch's abort word (fgi_run_batch): reason << 32 | (step + 1). kAbortBarrier: a cascade's grid
// barrier timed out (no step index; the graph is poisoned until fgi_restore).
constexpr unsigned long long kAbortDetach = 1, kAbortPool = 2, kAbortBarrier = 3;
constexpr int kAccBarrierIdx = 7;       // acc[7]: a cascade's grid barrier timed out
// grid-barrier arrival counters (g->gbar, monotonic, a multiple of the grid size between launches):
// word 0 k_wave_coop's (streaming cascades), word kGbarFused k_wave_fused's (their grids differ)
constexpr int kGbarWords = 32, kGbarFused = 16;

// Record sink of a batch's cascades (fgi_last_batch_flagged). A cascade of k_wave_coop
// appends one record per node it only flags: boundary handle << 32 | canonical state_flags (k_flag_list's
// format). rec == nullptr: no sink (the graph cannot flag, or the wave is no batch's). The cursor counts
// every record of the batch, also those past cap, which are not written. A batch's cascades run one after
// the other on one stream, so a cascade's records are the run [cursor at its start, cursor at its end).
// A cascade records in two places: its `immediately` roots before its first grid barrier, its fold behind
// its last one; nothing in between. So one thread publishes the boundary for free while the levels run:
// mark: the step's word, set after the first barrier to 1 + the cursor (then: this cascade's start + its
//   immediate roots' records); it stays 0 if the launch finds no roots or the batch aborted, which
//   records nothing;
// imm_n: the step's count of immediate roots' records.
// The cascade's run starts at mark - 1 - imm_n and ends where the next cascade that ran starts (the last
// one: at the cursor the batch's results bring back).
struct RecSink {
    unsigned long long* rec = nullptr;   // [cap]
    unsigned long long* cur = nullptr;
    uint64_t cap = 0;
    const uint32_t* l2s = nullptr;       // hot label -> slot (labels below K); a cold label l is handle l - K
    uint32_t K = 0;
    unsigned long long* mark = nullptr;
    unsigned long long* imm_n = nullptr;
};

// Per-level counters. The producers of level L's frontier (roots, push emits, received targets)
// reserve list space with ONE packed 64-bit atomic on `ft` (frontier entries << 32 | edges): the
// returned value is both the entry index and the exclusive edge offset (escan) of the reserving
// batch, so the frontier list comes out already scanned. The last block of each producer kernel
// unpacks ft into F / T (a pull level sums its per-block counts instead).
struct LevelCtr {
    unsigned long long F;       // frontier entries (expandable = invalidated with |row| > 0)
    unsigned long long T;       // edges of the frontier (sum of row lengths)
    unsigned long long ft;      // packed reservation counter (F << 32 | T)
    unsigned long long pull;    // 1 if this level runs bottom-up (pull)
    unsigned long long w;       // pull level L-1: its winners (the frontier count before rows)
    unsigned long long mult;    // push: fine chunks per expand chunk
    unsigned long long npull;   // pull levels of the wave before this one (which candidate list to read)
    unsigned long long sum;     // pull level: 1 if k_collect built the nonzero-word summary for its probes
    unsigned long long want;    // 1 if the automatic choice (Beamer's rules) is pull, whatever the level ran
                                // as (a level the host pinned to push, push-only options): the next wave's
                                // launch plan (run_wave's left-out collects) learns from it
};

// A level's frontier totals: a push producer leaves them packed in ft (the single engine does not
// unpack them: the next kernel and the host read ft directly, which saves the producer's last-block
// hand-off; a partition's producers unpack them into F / T for the all-reduce), a pull level's last
// block writes F / T (ft stays 0). F == 0 means no frontier entry, and then T == 0 too.
__host__ __device__ inline uint64_t lvl_F(const LevelCtr& c) { return c.F ? c.F : (c.ft >> 32); }
__host__ __device__ inline uint64_t lvl_T(const LevelCtr& c) { return c.F ? c.T : (c.ft & 0xFFFFFFFFull); }

struct WaveCtr {
    unsigned long long inv;         // invalidated handles of the wave (V_inv; the final collect)
    unsigned long long e_match;
    unsigned long long n_flagged;
    unsigned long long root_inv;    // winners of the roots kernel
    unsigned long long pull_surv;   // pull: candidates still unvisited after their level (written forward)
    unsigned long long pull_edges;  // pull: dependency entries examined
    unsigned long long pull_live;   // pull: slots not yet dead when scanned
    unsigned long long pull_win;    // pull: nodes invalidated by pull levels
    unsigned long long pull_scan;   // pull: slots scanned (bitmap reads), summed over pull levels
    unsigned long long pull_tail;   // pull: candidates whose head dependency missed (list scanned)
    unsigned long long root_flagged;  // flag-only visits of the roots kernel
    // fused waves (run_wave): the head / tail kernels run the small push levels inside
    // one launch each; k_level launches in between run the pull levels (and push levels too large for
    // the fused grid), each reading its level from here
    unsigned long long cur;         // the next level to run
    unsigned long long mid_base;    // the level of the round's first k_level launch (mid index 0)
    unsigned long long phase;       // kPhaseDone once the final count has run
    unsigned long long broken;      // a fused kernel's grid barrier timed out
    unsigned long long n_levels;    // device-side totals of the wave: non-empty levels,
    unsigned long long e_trav;      //   their frontier edges (E_trav),
    unsigned long long f_total;     //   their frontier entries,
    unsigned long long n_pull;      //   pull levels,
    unsigned long long push_edges;  //   edges / entries of the push levels run inside the fused kernels
    unsigned long long push_f;
    unsigned long long n_mid;       //   levels run by k_level launches
    unsigned long long mid_kind[16];  // per k_level launch of the round (mid index): 0 nothing, 1 push, 2 pull
    unsigned long long mid_push_edges;  // edges / entries of the push levels run by k_level launches
    unsigned long long mid_push_f;
    unsigned long long t0;          // device wall clock at k_wave_init (a wave's kernel span without events)
    unsigned long long t_max;       // the wave's largest level, in edges (level-group waves: tail_account)
    unsigned long long pull_pushed; // levels the automatic choice would pull that a tail ran as push (async `all`)
    LevelCtr lvl[kRing];
};
constexpr unsigned long long kPhaseDone = 1;
constexpr uint32_t kPlanMax = 48;   // levels of a planned partitioned wave
constexpr int kMidMax = 16;         // k_level launches per round of a fused wave

// per-wave accounting of a partitioned wave
struct PartWave {
    std::chrono::steady_clock::time_point t0;
    uint64_t n_roots = 0, levels = 0, e_trav = 0, f_total = 0, sent = 0, expand_launches = 0;
    uint64_t push_edges = 0, push_f = 0, pull_launches = 0, pull_levels = 0;
    double expand_ms = 0, pull_ms = 0;
    bool pulled = false;
};

// FGI_OPT_FUSED bits: fused waves on; tests: no mid-pair prediction (every k_level level found by an
// extra round), every push level as a k_level launch, every push level in the fused grid
constexpr int kFusedOn = 1, kFusedNoPredict = 2, kFusedMidPush = 4, kFusedTailPush = 8;
// Fused waves are off by default: on MI355X they measured slower than the level groups (DESIGN.md
// §3: a grid barrier's cache maintenance costs what a launch does, and the fused grid runs the push
// levels' dependent round trips with fewer blocks). FGI_FUSED=1 in the environment turns them on.
inline int fused_default() {
#if FGI_VARIANTS
    const char* e = getenv("FGI_FUSED");
    return (e && e[0] == '1') ? kFusedOn : 0;
#else
    return 0;
#endif
}

// ---- cross-block hand-off shared by the kernels' last-block epilogues (wave.hip, graph.hip) ---------
// Block-uniform: true in the block that arrives last at this launch's completion counter, over the
// blocks [0, G) taking part. The counter is two-level (one word serialises near 88 atomics/us,
// MI355X_MICROARCH.md "dequeue"): block b counts into group b % kDoneGroups, the last block of a group
// into the top word; the last block resets every word for the next launch. Agent-scope atomic RMWs are
// performed at the coherence point shared by the XCDs, so what the last block must see has to be
// performed before its block arrives:
//   kDrainAll = false: the block's hand-off values are written by thread 0 (or by atomics whose result
//     a thread waited for); wave 0 drains its own memory counter before the arrival (the traversal
//     kernels: one wave's wait, not every wave's, sits on their critical path);
//   kDrainAll = true: any wave may have issued returnless atomics the last block reads (a batch's
//     classify counts, the overflow-row list): every wave drains its vector-memory counter (returnless
//     atomics included, gfx9 counts them in vmcnt) before the block's barrier, and the arrivals are
//     acquire-release at agent scope.
template <bool kDrainAll>
__device__ inline bool last_block_arrive(unsigned long long* done, uint64_t G) {
    __shared__ bool s_last;
    if (kDrainAll) __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        constexpr int kOrd = kDrainAll ? __ATOMIC_ACQ_REL : __ATOMIC_RELAXED;
        const uint32_t grp = blockIdx.x % kDoneGroups;
        const uint64_t gsize = (G - grp + kDoneGroups - 1) / kDoneGroups;
        const unsigned long long t =
            __hip_atomic_fetch_add(done + (1 + grp) * kDoneStride, 1ull, kOrd, __HIP_MEMORY_SCOPE_AGENT);
        bool last = false;
        if (t == gsize - 1) {
            const uint64_t ng = G < (uint64_t)kDoneGroups ? G : (uint64_t)kDoneGroups;
            last = __hip_atomic_fetch_add(done, 1ull, kOrd, __HIP_MEMORY_SCOPE_AGENT) == ng - 1;
        }
        s_last = last;
    }
    __syncthreads();
    const bool last = s_last;
    if (last && threadIdx.x <= (uint32_t)kDoneGroups)
        __hip_atomic_exchange(done + threadIdx.x * kDoneStride, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return last;
}

// ---- host-side graph object -------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// The host-memory state view (fgi_state_view_open; view.hip). Six bit planes over the
// boundary's handles (kViewPlanes x words 64-bit words, plane p at word p * words), kept twice: on the
// device (dev), where the update kernels change them with atomics and mark what they changed in a dirty
// bitmap (one bit per plane word), and in fine-grained host memory (host), where the flush kernel copies
// the dirty words. host[kViewPlanes * words] is the view's sequence word, written by the host alone.
constexpr uint32_t kViewPlanes = 6;
enum { kVpRegistered = 0, kVpConsistent, kVpComputing, kVpIoso, kVpDelayStarted, kVpHasDelay };
struct View {
    bool open = false;
    uint64_t words = 0;                    // 64-bit words per plane
    unsigned long long* host = nullptr;    // [kViewPlanes * words + 8]
    unsigned long long* dev = nullptr;     // [kViewPlanes * words]
    unsigned long long* dirty = nullptr;   // [dirty_words] bit p * words + x: dev word x of plane p differs from host
    uint64_t dirty_words = 0;
    unsigned long long* pub_dev = nullptr; // words the flush kernels copied so far
    uint64_t pub_base = 0;                 // words the full builds copied
    uint64_t updates = 0, full_builds = 0, extra_waits = 0;
    // a partition rank's view (fgi_part_state_view_open): its first slot and its owned slots (else 0, 0)
    uint32_t part_base = 0, part_n_local = 0;
    // fgi_part_run_batch: its steps leave the view alone (view_on is false) and list the rank's boundary
    // handles they changed here; the batch refreshes them once, behind itself, from the post-batch words
    bool deferred = false;
    std::vector<uint32_t> pending;
};
// A partition rank's wave with codes (k_view_part_wave) gathers from n_local / kPartViewGatherDen invalidated
// handles on and scatters below (FGI_OPT_PART_VIEW_PATH pins either)
constexpr uint32_t kPartViewGatherDen = 16;

// Host roots on their way to the device: n roots (4 B each), then their `immediately` bytes at cap * 4, in
// one pinned and one device buffer of cap * 5 bytes, moved by two copies on the graph's stream. The owner
// sees to it that the previous call's copies have been consumed before it stages again.
struct RootStage {
    char* h = nullptr;   // pinned
    char* d = nullptr;
    uint64_t cap = 0;
    // imm nullable (*imm_dev is then null); nothing waits
    fgi_status stage(fgi_graph* g, uint32_t n, const uint32_t* roots, const uint8_t* imm, uint32_t** roots_dev, uint8_t** imm_dev);
    void release();
};

// A partition rank's last wave in the host's numbering (part_out.hip): the bitmap over the
// rank's boundary handles (bit h = global slot base + h, as the state view's planes) and the ascending
// global ids made from it, both on the device, each made at most once per wave; and the staging of
// fgi_part_invalidate_host's roots. Everything is allocated at first use and grown by need.
struct PartOut {
    unsigned long long* bits = nullptr;   // [bits_cap] device
    uint64_t bits_cap = 0;
    uint32_t* ids = nullptr;              // [ids_cap] device
    uint64_t ids_cap = 0;
    unsigned long long* bsum = nullptr;   // [bsum_cap] per-block popcounts, scanned in place; then the total
    uint64_t bsum_cap = 0;
    bool bits_valid = false, ids_valid = false;   // of the rank's last wave (part_out_mark clears them)
    RootStage roots;                      // fgi_part_invalidate_host's
};
enum { kPoutNone = 0, kPoutWave = 1, kPoutOther = 2 };
// With codes, a wave's host-order bitmap is gathered from n_local / kPartIdsGatherDen invalidated slots on
// and scattered from the wave's list below (FGI_OPT_PART_IDS_PATH pins either). Measured at 524,288 slots per
// rank (profiles/part_ids_ab.txt): the two tie at n_local / 256 and the gather wins above.
constexpr uint32_t kPartIdsGatherDen = 256;

// The subscription table of the replica fan-out (fanout.hip), over boundary handles.
// rec: 16-byte records chained from head[h] (FGI_NONE ends a chain); has: bit h set = head[h] != FGI_NONE.
// Free records: the stack fstack[0, free_n) and the never-used range [bump, cap). The host mirrors both
// counts from numbers the calls read back anyway (stored, delivered, dropped), so no kernel keeps a cursor.
// pcnt[p]: live entries of peer p. The last fan-out's lists stay on the device (out_*) for the repeat calls.
struct SubRec {
    unsigned long long call;
    uint32_t peer, next;
};
enum { kCascNone = 0, kCascWave = 1, kCascAsync = 2, kCascBatch = 3 };
struct Fanout {
    uint32_t* head = nullptr;              // [ext_handles]
    unsigned long long* has = nullptr;     // [words]
    uint64_t words = 0;
    SubRec* rec = nullptr;                 // [cap]
    uint32_t* fstack = nullptr;            // [cap]
    uint64_t cap = 0, bump = 0, free_n = 0;
    unsigned long long* pcnt = nullptr;    // [FGI_MAX_PEERS]
    unsigned long long* ctr = nullptr;     // [8] device counters of a call; ctr_h: pinned copy
    unsigned long long* ctr_h = nullptr;
    uint32_t* tcnt = nullptr;              // [tiles][n_peers] per-tile counts, scanned per peer in place
    uint64_t tcnt_cap = 0;
    unsigned long long* tot = nullptr;     // [FGI_MAX_PEERS] a fan-out's entries per peer
    unsigned long long* off = nullptr;     // [FGI_MAX_PEERS + 1] the last fan-out's peer offsets
    unsigned long long* out_call = nullptr;
    uint32_t* out_hnd = nullptr;
    uint64_t out_cap = 0;
    uint32_t* ids = nullptr;               // fgi_fanout_ids' upload
    uint64_t ids_cap = 0;
    unsigned long long* bits = nullptr;    // [words] the invalidated set as a bitmap when the wave kept none
    uint64_t made_serial = 0;              // casc_serial (a partition rank: pout_serial) the lists were made for (0: none)
    uint32_t made_peers = 0;
    uint64_t made_n = 0;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // 4, 5: a rank's source (fgi_part_last_wave_fanout)
    uint64_t live = 0, delivered = 0, dropped = 0, fanouts = 0, from_list = 0, from_bits = 0;
    double last_ms = 0;
};

struct Timers;   // the delay timers in device memory (timers.hip)

}  // namespace fgi

struct fgi_graph {
    int device = 0;
    int n_cu = 256;                    // compute units of the device (queried once at create)
    hipStream_t stream = nullptr;
    // Internal handle space (labels). n_slots / n_handles count the engine's labels:
    // K hot labels [0, K) for the heaviest slots, then label K + x for every other slot or detached
    // handle x (the labels K + x of hot slots stay empty). ext_slots / ext_handles are the boundary's
    // counts (fgi_config.n_slots, + n_detached). K = 0 (labels are the handles) unless the graph uses
    // hub-first labels.
    uint32_t n_slots = 0, n_detached = 0, n_handles = 0;
    uint32_t ext_slots = 0, ext_handles = 0;
    uint32_t lbl_K = 0;                // label capacity of the hot prefix (a multiple of kFoldTile)
    uint32_t lbl_hot = 0;              // hot labels in use (<= lbl_K), set at the first bulk edge load
    int opt_labels = 0;                // fgi_config.labels: 0 auto, 1 always, -1 never
    bool lbl_done = false;             // the hot set has been chosen (first bulk edge load)
    bool nodes_written = false;        // node words were written since create (note_words): at labels, if any
    // Partition codes: a partition renumbers the slots within each rank's range, heaviest
    // first, so that the all-gathered invalidated bitmap the pull levels probe holds every rank's hubs in a
    // compact run at the start of its range. Ownership is unchanged (a slot's code lies in its owner's
    // range). Every fgi_part_* entry point and every query maps slots <-> codes; the engine runs on codes.
    bool lbl_perm = false;
    uint32_t* pg_gc = nullptr;         // [n_global] slot -> code (device)
    uint32_t* pg_ig = nullptr;         // [n_global] code -> slot (device)
    std::vector<uint32_t> pg_gc_h, pg_ig_h;   // host copies
    uint64_t pg_hash = 0;               // of the slot -> code table (0: no codes); every rank's must agree
    uint32_t* s2l = nullptr;           // [ext_slots] hot label of a slot, FGI_NONE if cold
    uint32_t* l2s = nullptr;           // [lbl_K] slot of a hot label
    uint32_t* fold_start = nullptr;    // [fold_tiles + 1][lbl_ncls] first hot label of class c at slots >= t * kFoldTile
    uint16_t* fold_off = nullptr;      // [lbl_hot] per tile, its hot labels in (class, slot) order: slot - tile base
    uint32_t* fold_base = nullptr;     // [fold_tiles + 1] each tile's first entry in fold_off
    uint32_t lbl_ncls = 0, fold_tiles = 0;
    unsigned long long* xbm = nullptr; // [ext words] the wave's invalidated set over the boundary's handles
    unsigned long long* fold_status = nullptr;   // [fold tiles, >= kStats] per-tile counts of the final collect
    int rank = 0, world = 1;

    // node table
    uint64_t* node = nullptr;
    uint64_t* row_off = nullptr;
    uint32_t* row_len = nullptr;
    uint32_t* row_cap = nullptr;
    uint32_t* used_cnt = nullptr;
    uint32_t* home = nullptr;          // [n_detached]: home slot of a detached handle
    std::vector<uint32_t> free_detached;  // host free list of detached handles
    std::vector<uint8_t> seen_slots;      // host scratch, a byte per slot, all-zero between uses (slot-repeat checks)
    // device temporaries (Tmp), kept for reuse (same stream, so reuse is ordered after the previous
    // user) instead of a hipMalloc + hipFree (an implicit device sync) per call
    std::vector<std::pair<size_t, void*>> tmp_cache;
    size_t tmp_cached = 0;

    // edge pool
    uint32_t* pool_col = nullptr;
    uint64_t* pool_tag = nullptr;
    uint64_t pool_cap = 0;             // entries
    uint64_t pool_top = 0;             // bump pointer (host mirror of device counter)
    unsigned long long* pool_top_dev = nullptr;
    uint64_t pool_epoch = 0;           // bumped on compaction (invalidates snapshots)

    // wave workspace
    uint32_t* inv = nullptr;           // [n_handles] invalidated handles of the last wave (ascending)
    uint32_t* fr_off[2] = {nullptr, nullptr};  // frontier lists: row offsets (pool positions < 2^32)
    uint32_t* fr_len[2] = {nullptr, nullptr};
    uint64_t* escan[2] = {nullptr, nullptr};   // exclusive edge offset of every frontier entry
    uint32_t* cstart[2] = {nullptr, nullptr};  // fine chunk -> frontier entry holding its first edge
    uint64_t cstart_cap = 0;
    unsigned long long* bsum = nullptr;  // [8][kStatBlocks] per-block sums / prefixes of the epilogues
    unsigned long long* done = nullptr;  // completion counters of the last-block epilogues
    fgi::WaveCtr* ctr = nullptr;
    unsigned long long* gbar = nullptr;   // [kGbarWords] grid-barrier counters (k_wave_coop, k_wave_fused)
    unsigned long long* blk_stats = nullptr;   // [kStatBlocks][kStatCols] per-block wave statistics
    fgi::WaveCtr* ctr_host = nullptr;  // pinned
    // fine-grained host memory the wave's publish kernel writes: the counters, then a sequence word
    // (ctr_pub[kPubWords]) the host spins on instead of a stream synchronisation (run_wave)
    unsigned long long* ctr_pub = nullptr;
    uint64_t pub_seq = 0;
    int wall_khz = 0;                   // device wall-clock rate (WaveCtr::t0 and the publish time)
    uint64_t last_pub_t = 0;            // the last publish_wait's device wall-clock stamp
    unsigned long long* red_pub = nullptr;   // fine-grained host words of the partition's all-reduce results
    uint32_t* roots_buf = nullptr;     // staging for host roots
    uint8_t* imm_buf = nullptr;
    uint64_t roots_cap = 0;
    uint64_t last_wave_n = 0;
    // asynchronous waves (fgi_invalidate_async / fgi_wave_wait): at most two in flight (tickets t and
    // t + 1), each with its own published counters (apub[t % 2]) and id buffer (inv for even tickets,
    // inv_alt for odd ones); inv_cur is the id list of the last wave a caller waited for
    struct AsyncWave {
        uint64_t ticket = 0, seq = 0;
        uint64_t n_inv = 0;            // V_inv, once waited for
        uint32_t n_roots = 0;
        bool busy = false, imm = false, timing = false;
        bool flg = false;              // the wave queued the flagged-set post-pass (flag_gate was on)
        int group = 0;
        std::chrono::steady_clock::time_point t0;
    };
    AsyncWave aw[2];
    unsigned long long* apub[2] = {nullptr, nullptr};
    uint64_t apub_seq = 0;
    uint64_t next_ticket = 1;
    uint32_t* inv_alt = nullptr;
    uint32_t* inv_cur = nullptr;
    // fgi_invalidate_async_host: per ticket parity, the roots staged in pinned memory and their device copy
    fgi::RootStage ar[2];
    bool lists_wanted = false;         // a wave met a frontier heavy enough to pull (async waves build lists first)
    bool ids_valid = false;            // inv holds the last wave's list (else ensure_ids rebuilds it)
    int last_levels = 4;               // non-empty levels of the last wave (sizes the first level group)
    int last_head = 4;                 // levels up to the last one the tail cannot run (pull, or large push)
    std::vector<uint8_t> last_dirs;    // the last synchronous wave's levels: 1 pull, 0 push (k_collect grids)
    int last_mid = 3;                  // k_level launches the last fused wave needed (its mid pairs)
    int fused_per_cu = 0;              // resident k_wave_fused blocks per CU (0: not queried yet)
    bool coop_warm = false;            // a cooperative launch has run (coop_warm)

    // Visit bitmap over handles: bit h set = node h was visited by a wave since the
    // last fold. A visit's effect is a pure function of the node word, and every second visit is a
    // no-op, so the pair (node word, visit bit) is the node's state; one atomicOr decides the first
    // visitor. fold() applies the bits to the words before any mutation or state query.
    uint32_t* vis_bm = nullptr;
    // fgi_restore swaps in a clean second visit bitmap instead of leaving the clear to the next wave's init
    // kernel; the next wave's list kernel clears the swapped-out one (spare_dirty) as it goes
    uint32_t* vis_spare = nullptr;
    bool spare_dirty = false;
    // the last level-group wave left its counters, statistics and invalidated bitmap zeroed (its final
    // kernels and publish did, WaveEnd): the next wave runs without k_wave_init
    bool wave_clean = false;
    // A count-only synchronous wave (run_wave without an id destination) keeps its invalidated bitmap until
    // the next wave starts (ensure_ids, the bits download and xbm read it) and leaves everything else
    // zeroed: wave_kept. Only run_wave honours it, by swapping in the clean second bitmap inv_spare (same
    // size as inv_bm, hot-heads tail included; allocated by a single-device graph's first count-only
    // wave); that wave's end kernel clears the swapped-out one (inv_spare_dirty). Every other driver sees
    // wave_clean == false and starts with k_wave_init.
    bool wave_kept = false;
    uint32_t* inv_spare = nullptr;
    bool inv_spare_dirty = false;
    bool v_dirty = false;              // vis_bm may hold set bits
    bool vis_stale = false;            // fgi_restore left vis_bm's clearing to the next wave (flush_vis)
    bool coop_clean = false;           // wave counters, statistics and bitmaps clear (a cooperative wave left them so)
    // Expandable-class bitmap (Consistent, no delay: a first visit invalidates and expands), built
    // from the node words; pull levels read it instead of the words (2 MB vs 128 MB at 16M slots).
    uint32_t* cls_bm = nullptr;
    bool cls_valid = false;
    bool words_dirty = true;           // node words changed since the snapshot
    // Flagged sets (fgi_last_wave_flagged / fgi_wave_wait_flagged). flag_gate: the graph may
    // hold a Computing node or one with hasDelay, the only nodes a visit can flag without invalidating
    // (set by fgi_register_nodes / fgi_begin_compute / a batch's begin_compute steps, restored with the
    // snapshot). While it is off no wave launches anything for the flagged set and every set is empty.
    // flg_bm is the flaggable-class bitmap beside cls_bm: bit h set = a non-immediate first visit of h
    // would only set a flag (first_visit == 2 on h's canonical word, its visit bit folded in). A wave's
    // flagged set is vis_bm & flg_bm & ~inv_bm; the post-pass (k_flag_list) lists it and clears the bits
    // it found, so a node is reported once although vis_bm keeps its bit until the next fold.
    bool flag_gate = false, snap_flag_gate = false;
    uint32_t* flg_bm = nullptr;        // [bm_words], allocated when the gate first opens
    bool flg_valid = false;            // flg_bm matches the node words and visit bits (cleared with cls_valid)
    unsigned long long* flg_out[2] = {nullptr, nullptr};   // [n_handles] per ticket parity (synchronous waves: 0):
                                       // boundary handle << 32 | canonical state_flags, unordered
    unsigned long long* flg_cnt = nullptr;   // [2] entries in flg_out[k]
    int flg_last = -1;                 // the last call's set: -1 empty, 0 / 1 flg_out[k], -2 a batch's (bflg_runs)
    std::vector<uint32_t> flg_drop;    // boundary slots the last call replaced (fgi_begin_compute): not in its set
    bool flg_arm_later = false;        // fgi_begin_compute: the cascade's records arm behind the install, not the post-pass
    // Invalidated bitmap: bit h set = node h was invalidated by this wave. It is the frontier of a
    // pull level: every node invalidated before the previous level already had all its dependants
    // visited, so "an invalidated parent" and "a parent in the previous level's frontier" select
    // the same unvisited slots. Multi-GPU: all-gathered into front_global.
    uint32_t* inv_bm = nullptr;
    uint64_t bm_words = 0;             // words per bitmap (even: pull levels store 64-bit words)

    // dependency-list cache for pull levels: for slot d, the handles whose `_usedBy` row holds
    // (d, version(d)) (= the reference's d._used). Rebuilt from the rows when stale.
    uint64_t* uin_off = nullptr;
    uint32_t* uin_len = nullptr;
    uint32_t* uin_src = nullptr;
    uint64_t* uin_head = nullptr;      // [n_slots] the list's first two entries (lo | hi << 32, FGI_NONE
                                       // if absent), probed first: lists are ordered by the number of
                                       // dependencies of each entry, the ones a wave reaches earliest
    uint32_t* uin_more = nullptr;      // bitmap: the list has more than two entries
    uint64_t uin_cap = 0;
    // Per pool position: the entry was live (tag == its dependant's version) when the dependency lists
    // were built. Versions change only through mutations (mut_epoch) and entries move only through
    // compaction (pool_epoch), so while both are unchanged an entry is live iff its bit is set and its
    // dependant is current: fgi_prune then reads this bitmap and a bitmap of current nodes (2 MB at 16 M
    // slots, L2-resident) instead of gathering every dependant's 8-byte node word.
    unsigned long long* pool_live = nullptr;
    uint64_t pool_live_cap = 0;              // positions covered
    uint64_t pl_mut_epoch = 0, pl_pool_epoch = ~0ull;
    // Pull candidates: the slots with a non-empty dependency list, grouped by the
    // pull block owning their tile range (segment [cand_seg[b], cand_seg[b + 1]), slot order), as
    // (slot, list heads, row length | more-than-two-entries bit << 31). A pull level reads the
    // static list (first pull of a wave) or the survivors of the previous pull level, and writes its
    // own survivors (still unvisited) into the other survivor buffer at the same segment bases.
    // One 16-byte entry per candidate: rec_encode's two words, head 0, head 1.
    uint4* cand = nullptr;
    uint32_t* cand_seg = nullptr;      // [pull grid + 1]
    // Tail runs: for each pull block, for each of its candidates with more than two list entries, in
    // candidate order: [list length, entry 2, entry 3, ...] — what a queued candidate's scan reads, found
    // from the record's offset alone (block b's runs start at run_seg[b]). Built with the candidates.
    uint32_t* trun = nullptr;
    uint64_t trun_cap = 0;
    uint64_t* run_seg = nullptr;       // [pull grid + 1]
    uint32_t* wl = nullptr;            // [n_slots] a pull level's expandable winners, per block at cand_seg
    // Hot heads: the (at most kHot) handles that head the most lists get a rank; candidate entries
    // name them by a bit index past the bitmap's end (hot_w0), where a pull level finds a snapshot of their
    // invalidated bits taken before the level (8 KB: L1-resident) instead of the whole bitmap.
    uint32_t* hot_id = nullptr;        // [kHot] rank -> handle (FGI_NONE past n_hot)
    uint32_t n_hot = 0;
    uint64_t hot_w0 = 0;               // the snapshot's first word in the bitmap a pull level probes
                                       // (inv_bm, or a partition's front_global): kHot / 32 words
                                       // allocated past its end; a hot head's code is 32 * hot_w0 + rank
    uint4* sv[2] = {nullptr, nullptr};
    uint32_t* sv_cnt[2] = {nullptr, nullptr};   // [pull grid] survivors per block
    uint64_t cand_cap = 0;
    uint32_t cand_grid = 0;            // pull grid the segments were built for (0 = none)
    uint64_t uin_epoch = 0;            // mut_epoch the cache was built at (0 = never)
    uint64_t mut_epoch = 1;            // changes on every mutation of rows or versions
    uint64_t epoch_counter = 1;
    uint64_t snap_mut_epoch = 0;

    // options (fgi_set_option)
    int opt_dead_filter = 1;
    int opt_defrag_pct = 60;
    int opt_part_coll = 0;             // FGI_OPT_PART_COLLECTIVES
    int opt_front_exchange = 0;        // FGI_OPT_FRONT_EXCHANGE: 0 auto, 1 full all-gather, 2 delta
    uint64_t stale_est = 0;            // entries waves made stale since the last prune (fgi_prune_step)
    uint32_t prune_cursor = 0;         // next handle of fgi_prune_step's walk
    int opt_direction = 0;
    int opt_pull_alpha = 28;           // profiles/r2y_direction_sweep.jsonl: 28 beats 14 on configs[0] (-6%) and [1] (-1%)
    int opt_pull_tpb = 0;             // pull tiles per block (0: from the CU count; tests)
    int opt_hot_heads = 0;            // FGI_OPT_HOT_HEADS: cap on the hot heads (0: by graph size)
    int opt_run_off_bits = (int)fgi::kRecOffBits;  // FGI_OPT_RUN_OFFSET_BITS: runs past 2^bits words take the uin_off path
    // probe summary: one bit per 64-bit word of the invalidated bitmap (set iff the word is nonzero),
    // built before a pull level while few words can be nonzero, so cold head and tail probes that
    // would miss are answered from an L2-resident table (FGI_OPT_PROBE_SUMMARY)
    uint32_t* sum_bm = nullptr;
    int64_t opt_sum_min = -1;         // fewest 64-bit bitmap words for a summary (-1: never; measured
                                      // slower on configs[2])
    int opt_pull_beta = 32;           // after a pull, pull again while the frontier exceeds n / beta
    int opt_level_timing = 1;         // HIP events around each level's k_level launch (statistics)
    int opt_fused = fgi::fused_default();  // FGI_OPT_FUSED (kFused* bits)

    // generic scratch (sorts, batches)
    void* scratch = nullptr;
    size_t scratch_bytes = 0;
    unsigned long long* misc_dev = nullptr;   // small device counters [16]
    unsigned long long* misc_host = nullptr;  // pinned [16]

    // snapshot
    uint64_t* snap_node = nullptr;
    uint64_t* snap_row_off = nullptr;
    uint32_t* snap_row_len = nullptr;
    uint32_t* snap_row_cap = nullptr;
    uint32_t* snap_used = nullptr;
    uint64_t snap_epoch = ~0ull;
    uint32_t* snap_home = nullptr;           // [n_detached]
    std::vector<uint32_t> snap_free_detached;

    // A failed streaming batch (a cascade's grid barrier timed out) left the graph half-applied: every
    // entry point but fgi_restore / fgi_destroy / fgi_last_error / fgi_set_option returns FGI_ESTATE
    // until fgi_restore brings back the snapshot (graph.hip, usable()).
    bool failed = false;
    int coop_per_cu = 0;                     // resident k_wave_coop blocks per CU on this graph's device
    uint32_t fault_block = 0;                // FGI_OPT_FAULT_INJECT: block + 1 of a cascade that skips a barrier
    uint32_t fault_skip = 0;                 // ... after this many more cascade launches
    uint32_t fault_tail_block = 0;           // FGI_OPT_FAULT_INJECT_TAIL: the same for a wave tail (k_wave_tail)
    uint32_t fault_tail_skip = 0;

    // timing
    std::vector<hipEvent_t> ev;        // pairs around expand launches
    // streaming batches (fgi_run_batch): pinned host staging + its device copy, the ids output
    char* bst_h = nullptr;
    char* bst_d = nullptr;
    size_t bst_cap = 0;
    uint32_t* bout = nullptr;
    uint64_t bout_cap = 0;
    uint64_t batch_ids_hint = 0;       // the previous batch's id count (sizes the copy made with the results)
    // The flagged sets of the last batch's cascades (fgi_last_batch_flagged), valid while
    // flg_last == -2. brec: the records the cascades wrote (16 B per handle, allocated by the first batch on
    // a graph that can flag). bflg_runs: per cascade that ran to its end, in step order, its record run and
    // where the staging (bst_h) keeps a begin_compute step's slots (dropped from its run). bflg_step /
    // bflg_set: the accessor's result, made on its first call after the batch (one copy, sorted per run).
    unsigned long long* brec = nullptr;
    uint64_t brec_cap = 0;
    struct BatchRun {
        uint32_t step = 0, n_drop = 0;
        size_t drop_off = 0;           // the step's slots in bst_h (n_drop of them; begin_compute only)
        uint64_t lo = 0, hi = 0;       // records [lo, hi) of brec
    };
    std::vector<BatchRun> bflg_runs;
    std::vector<uint32_t> bflg_step;   // the accessor's cache: step, then handle << 32 | state_flags
    std::vector<uint64_t> bflg_set;
    bool bflg_read = false;
    std::vector<hipEvent_t> batch_ev;  // fgi_run_batch per-cascade timing events (pairs)
    hipEvent_t ev_w0 = nullptr, ev_w1 = nullptr;

    // multi-GPU
    void* part = nullptr;
    fgi::PartWave pw;
    // planned partitioned waves (run_part_wave): the directions of the previous wave's levels (1 pull),
    // the key they were learnt under, and whether the pull lists were ready then
    std::vector<uint8_t> part_plan;
    uint64_t part_plan_key = 0;
    bool part_plan_pull = false;
    int opt_part_plan = 1;             // FGI_OPT_PART_PLAN

    std::string err;

    // (behind every older member: their places in the struct stay what they were)
    // The flagged sets of a partition's last call that ran cascades (fgi_part_last_flagged):
    // this rank's share. Every cascade of the call (run_part_wave) queues k_flag_list's partition
    // instantiation behind its last final collect; it appends to prec (global slot << 32 | canonical
    // state_flags) through one device cursor, pcur[0], which the call clears once and no cascade resets.
    // After cascade k's post-pass the cursor is copied to pcur[1 + k] on the device, so run k is the
    // records [pcur[k], pcur[1 + k]) (pcur[0] read as 0). Nothing waits: the accessor downloads the cursor,
    // the marks and the records on its first call, sorts each run, drops a begin_compute step's own slots
    // (PartRun::drop, host numbering) and caches the result. pflg_batch: fgi_part_run_batch is running,
    // which opened the call itself (part_flagged_begin) and numbers the cascades by pflg_step.
    unsigned long long* prec = nullptr;
    uint64_t prec_cap = 0;
    unsigned long long* pcur = nullptr;   // [pcur_cap]: the cursor, then a mark per cascade
    uint64_t pcur_cap = 0;
    struct PartRun {
        uint32_t step = 0;
        std::vector<uint32_t> drop;    // sorted
    };
    std::vector<PartRun> pflg_runs;
    std::vector<uint32_t> pflg_steps;  // the accessor's cache: step, then global slot << 32 | state_flags
    std::vector<uint64_t> pflg_set;
    bool pflg_read = false, pflg_batch = false;
    uint32_t pflg_step = 0;
    fgi::View* view = nullptr;         // the host-memory state view (null until fgi_state_view_open)
    int opt_part_view_path = 0;        // FGI_OPT_PART_VIEW_PATH: 0 by the wave's count, 1 scatter, 2 gather
    // A partition rank's last wave in the host's numbering (part_out.hip; fgi_part_last_wave_ids / _bits,
    // fgi_part_wave_ids_dev). pout_kind: what the rank's last call that ran cascades was
    // (kPoutNone: none since create or fgi_restore; kPoutWave: one wave, whose result the accessors make on
    // demand; kPoutOther: a mutation or a batch, which report ids through their own out_ids). pout: the
    // buffers, null until an accessor or fgi_part_invalidate_host first needs them. pout_serial counts
    // part_out_mark's calls: fgi_part_last_wave_fanout makes its lists once per serial (Fanout::made_serial).
    fgi::PartOut* pout = nullptr;
    int pout_kind = 0;
    uint64_t pout_serial = 0;
    int opt_part_ids_path = 0;         // FGI_OPT_PART_IDS_PATH: 0 by the wave's count, 1 scatter, 2 gather
    // Replica fan-out (fanout.hip). fan: the subscription table, null until the first
    // fgi_subscribe. casc_serial counts the calls that ran cascades (and fgi_restore), casc_kind says what
    // the last one was (kCasc*): fgi_last_wave_fanout makes its lists once per serial, from a kCascWave only.
    fgi::Fanout* fan = nullptr;
    uint64_t casc_serial = 0;
    int casc_kind = 0;
    int opt_fanout_path = 0;           // FGI_OPT_FANOUT_PATH: 0 by what the wave left, 1 id list, 2 bitmap, 3 (measurement) a rank's bitmap renumbered whole
    bool tmp_poison = false;           // FGI_TMP_POISON=1: every temporary is handed out filled with 0xA5
    fgi::Timers* tim = nullptr;        // the delay timers (timers.hip), null until fgi_timers_open / fgi_part_timers_open
};

// ---- internal entry points shared between translation units ----------------------------------
namespace fgi {
// ---- hub-first labels (labels.hip) ----
constexpr uint32_t kFoldTile = 65536;            // slots per fold tile (1,024 bitmap words; offsets fit 16 bits)
constexpr uint32_t kFoldWords = kFoldTile / 64;
constexpr uint32_t kLabelAutoSlots = 1u << 25;   // auto: graphs whose bitmap outgrows one XCD's L2 (4 MB)
constexpr uint32_t kClassPerOctave = 8;          // weight classes per octave of (dependencies + 1)
constexpr uint32_t kLabelClasses = 33 * kClassPerOctave;
constexpr uint32_t kMaxHotClasses = 256;        // hot classes (one per thread of a fold block)
// hot-prefix capacity of a graph of n boundary slots (0: the graph keeps labels = handles)
uint32_t labels_capacity(uint32_t n_slots, int opt);
// boundary handle x -> label (x < ext_handles) and back, on the device (in place; no-ops with K = 0)
fgi_status labels_map_in(fgi_graph* g, uint32_t* dev, uint64_t n);
fgi_status labels_map_out(fgi_graph* g, uint32_t* dev, uint64_t n);
// both halves of edge keys (used << 32 | dependant), boundary -> labels / labels -> boundary
fgi_status labels_map_keys(fgi_graph* g, uint64_t* keys, uint64_t m);
fgi_status labels_unmap_keys(fgi_graph* g, uint64_t* keys, uint64_t m);
// first bulk edge load (keys in boundary handles): choose the hot set from the keys' dependants and
// move the node words already registered to their labels. No-op unless the graph wants labels and has
// not chosen them yet.
fgi_status labels_choose(fgi_graph* g, const uint64_t* keys, uint64_t m);
// ---- partition codes (part.hip) ----
// whether a partition of n_global slots renumbers its slots (fgi_config.labels / FGI_LABELS, auto from 2^25)
bool part_codes_wanted(const fgi_graph* g, uint32_t n_global);
// global slots -> codes (host arrays, into out; returns the array to use: `in` itself without codes)
const uint32_t* part_codes_in(const fgi_graph* g, uint64_t n, const uint32_t* in, std::vector<uint32_t>& out);
// a partition's local handles (owned slots base + h, h < n_local; detached handles unchanged) <-> the
// engine's local indices, in place on the device (out: engine -> boundary), or one on the host
fgi_status part_codes_local(fgi_graph* g, uint32_t* dev, uint64_t n, bool out);
uint32_t part_code_local_h(const fgi_graph* g, uint32_t h, bool out);
// a global code -> its slot on the host (ids and dependants leaving the engine)
inline uint32_t part_slot_of(const fgi_graph* g, uint32_t code) {
    return (g->lbl_perm && code < g->pg_ig_h.size()) ? g->pg_ig_h[code] : code;
}
// the words of a fold tile's slots: per hot class, the hot labels of the tile's slots, or none
struct FoldArgs {
    const uint32_t* l2s;           // null: no hot labels (the bitmap of handles is the labels' own)
    const uint32_t* fold_start;
    const uint16_t* off;           // fold_off / fold_base (fgi_graph)
    const uint32_t* base;
    uint32_t ncls, tiles;          // fold_start is [tiles + 1][ncls]
    uint32_t K;                    // cold label of handle x: K + x
    unsigned long long* xbm;       // out: the invalidated set over boundary handles
    uint32_t exp;                  // measurement only (FGI_FOLD_EXP, results wrong): 1 no hot labels, 2 no cold copy, 4 no chunks, 8 no staging
};
// active (xbm set) iff the graph has a hot-label prefix (K > 0): the boundary's bitmap is then the
// labels' one shifted by K, ORed with the hot labels' bits at their slots
inline FoldArgs fold_args(const fgi_graph* g) {
    static const uint32_t exp = [] {
        const char* e = getenv("FGI_FOLD_EXP");
        return e && *e ? (uint32_t)atoi(e) : 0u;
    }();
    return FoldArgs{g->lbl_hot ? g->l2s : nullptr, g->fold_start, g->fold_off, g->fold_base, g->lbl_hot ? g->lbl_ncls : 0u,
                    g->fold_tiles, g->lbl_K, g->lbl_K ? g->xbm : nullptr, exp};
}

fgi_status set_err(fgi_graph* g, fgi_status st, const char* fmt, ...);
fgi_status hip_check(fgi_graph* g, hipError_t e, const char* what);
fgi_status ensure_scratch(fgi_graph* g, size_t bytes);
fgi_status ensure_pool(fgi_graph* g, uint64_t entries);
fgi_status ensure_cstart(fgi_graph* g, uint64_t total_edges);
// Run one cascade wave from `n_roots` device-resident roots. Fills stats (nullable).
// ext_roots: the roots are boundary handles (the entry points' own arrays), mapped to labels by the
// roots kernel; internal callers pass labels.
// out: what the caller hands back from this call. kIds: the wave writes the ascending id list itself.
// kCount / kBits: the wave only counts (its bitmap stays in device memory) and the list is made on demand
// (ensure_ids); the two differ only in the variant build's fused waves, which list unless kBits.
enum class WaveOut { kIds, kCount, kBits };
fgi_status run_wave(fgi_graph* g, uint32_t n_roots, const uint32_t* roots_dev, const uint8_t* imm_dev,
                    fgi_wave_stats* stats, bool ext_roots = false, WaveOut out = WaveOut::kIds);
// The last single-device wave's invalidated list in g->inv (rebuilt from the invalidated bitmap if
// the wave ran in bitmap mode).
fgi_status ensure_ids(fgi_graph* g);
// Build rows from device edge keys (src << 32 | dst) + optional tags; pool must be empty.
// Consumes `keys`/`tags` buffers (they may be overwritten). If tags == nullptr the tag of each
// edge is synth_version(ver_seed, dst) (+1 if stale by hash).
// src_base / dst_base translate partition-local ids to global ones (multi-GPU): keys hold
// (local used handle << 32 | global dependant slot); tags and the stale hash use global ids.
fgi_status build_rows_from_keys(fgi_graph* g, uint64_t m, uint64_t* keys, uint64_t* tags,
                                uint64_t ver_seed, uint32_t stale_pct, uint64_t stale_seed,
                                uint32_t src_base = 0, uint32_t dst_base = 0);
// Existing live rows + m new entries given as host arrays (keys: used handle << 32 | dependant id).
fgi_status load_rows(fgi_graph* g, uint64_t m, const uint64_t* host_keys, const uint64_t* host_tags, uint32_t src_base,
                     uint32_t dst_base);
// Build the pull dependency-list cache if the graph changed since it was built.
fgi_status ensure_in_lists(fgi_graph* g);
// Copy the first two entries of every slot's list into uin_head, then (re)build the pull
// candidate segments (wave.hip).
// orders every dependency list by weight[entry], descending (graph.hip)
fgi_status sort_in_lists(fgi_graph* g, uint64_t total, const uint32_t* weight, uint32_t n_weight);
fgi_status build_in_heads(fgi_graph* g);
fgi_status build_candidates(fgi_graph* g);
// Pull geometry of a graph: blocks of a pull level and the tiles each owns (0 blocks: the graph is
// too large to pull on one device; its waves push).
void pull_geometry(const fgi_graph* g, uint32_t* grid, uint32_t* tpb);
// Record a mutation of rows or versions (invalidates the dependency-list cache).
inline void touch(fgi_graph* g) { g->mut_epoch = ++g->epoch_counter; }
// Record a change of node words (class bitmap rebuilt before the next wave; restore copies words).
inline void note_words(fgi_graph* g) {
    g->cls_valid = false;
    g->flg_valid = false;
    g->words_dirty = true;
    g->nodes_written = true;
}
// Apply the visit bitmap to the node words and clear it (wave.hip). Every entry point that reads or
// mutates node words outside a wave calls it first.
fgi_status fold(fgi_graph* g);
fgi_status flush_vis(fgi_graph* g);
bool coop_launch_mode();                 // FGI_COOP_LAUNCH=1: streaming waves as cooperative launches
fgi_status coop_warm(fgi_graph* g);   // first cooperative launch of the graph's process, outside timed spans   // fgi_restore's deferred visit-bitmap clear, before any use but a wave's init
#if FGI_PROBE
void print_coop_probe();
#endif
// A push-only wave in one launch (k_wave_coop), without host synchronisation (streaming batches):
// device-resident roots (n_max, or *n_dev of them), ids appended at out[*out_n ..), totals added to
// acc[0..6] (waves, levels, invalidated, E_trav, E_match, flagged, frontier entries; acc[7] set if a
// grid barrier timed out); nothing
// happens if *abort (nullable) is set when the wave starts. sink (nullable): the nodes the wave only flags
// are appended there (RecSink).
fgi_status run_wave_coop(fgi_graph* g, uint32_t n_max, const uint32_t* roots_dev, const uint8_t* imm_dev,
                         const unsigned long long* n_dev, uint32_t* out, unsigned long long* out_n,
                         unsigned long long* acc, unsigned long long* abort, const RecSink* sink = nullptr);
// Asynchronous waves (wave.hip): queue a wave and return (ticket), wait for one (and every earlier
// one), wait for all in flight. Every entry point but fgi_restore, fgi_set_option and the async calls
// themselves drains first (usable()).
fgi_status run_wave_async(fgi_graph* g, uint32_t n_roots, const uint32_t* roots_dev, const uint8_t* imm_dev,
                          uint64_t* ticket);
fgi_status wave_wait(fgi_graph* g, uint64_t ticket, uint64_t* out_n, const uint32_t** ids_dev, fgi_wave_stats* stats);
// the same wave from roots in host memory: staged through the ticket parity's pinned buffer
fgi_status run_wave_async_host(fgi_graph* g, uint32_t n_roots, const uint32_t* roots, const uint8_t* imm, uint64_t* ticket);
fgi_status drain_async(fgi_graph* g);
// Rebuild the expandable-class bitmap if node words changed (wave.hip); with flag_gate, the flaggable one too.
fgi_status ensure_cls(fgi_graph* g);
// The flagged set of ticket parity k's last wave (k < 0: empty), sorted by handle, without `drop` (sorted
// boundary slots): packed handle << 32 | state_flags. Waits for the graph's stream unless `blocking_copy`
// (an asynchronous ticket already waited for: a copy on the null stream lets later waves run on).
fgi_status read_flagged(fgi_graph* g, int k, bool blocking_copy, std::vector<uint64_t>* out);
// Pull tiles of a level over n slots with `grid` blocks.
__host__ __device__ inline uint64_t pull_iters(uint64_t n, uint32_t grid) { return (n + (uint64_t)grid * kPullTile - 1) / ((uint64_t)grid * kPullTile); }
// ---- the host-memory state view (view.hip) ----
// Everything below but view_on is a no-op returning FGI_OK while no view is open; the queueing calls
// launch on the graph's stream and do not wait.
inline bool view_on(const fgi_graph* g) { return g->view && g->view->open && !g->view->deferred; }
// a partitioned batch is running with a view open: its steps list what they changed (View::pending)
inline bool view_deferred(const fgi_graph* g) { return g->view && g->view->open && g->view->deferred; }
// the view's sequence word: odd from a call's first launch that may touch the view ...
void view_begin(fgi_graph* g);
// ... even again once the view is exact (no asynchronous wave in flight)
void view_end(fgi_graph* g);
// every plane from the node words and the unfolded visit bits (one pass over the handles), copied to the host
fgi_status view_rebuild(fgi_graph* g);
// a wave's invalidated bitmap (g->inv_bm, over labels) cleared out of `consistent` and `delay_started`
fgi_status view_wave(fgi_graph* g);
// the same for a partition rank's wave (its own inv_bm, over engine indices): k_view_wave without codes,
// k_view_part_wave with them
fgi_status view_part_wave(fgi_graph* g);
// the planes' bits of listed handles from their node words (and unfolded visit bits). kind: kViewHandles
// u32 boundary handles, kViewLabels u32 labels (a partition: the rank's engine indices), kViewRecords u64
// flagged records (handle << 32 | flags; a partition: global slot << 32 | flags), kViewCodes u32 global
// engine ids of a partition (the ones this rank owns are refreshed).
// The list holds n entries, or *n_dev of them if that is less (n_dev nullable). FGI_NONE entries are skipped.
enum { kViewHandles = 0, kViewLabels = 1, kViewRecords = 2, kViewCodes = 3 };
fgi_status view_refresh(fgi_graph* g, int kind, const void* list_dev, uint64_t n, const unsigned long long* n_dev = nullptr);
// the same for a host list of boundary handles (uploaded on the stream)
fgi_status view_refresh_host(fgi_graph* g, const uint32_t* handles, uint64_t n);
// the dirty words to the host planes, system-scope fenced
fgi_status view_flush(fgi_graph* g);
// flush, wait for the stream (counted in extra_waits), and end the update
fgi_status view_commit(fgi_graph* g);
void view_destroy(fgi_graph* g);

// ---- multi-GPU partition (part.hip) ----
// Release multi-GPU resources.
fgi_status part_destroy(fgi_graph* g);
struct PartView {
    uint32_t rank, world;
    uint32_t base, n_local, n_global, block;   // this rank owns [base, base + n_local); block = ceil(N/world)
    uint64_t* ver_all;          // [n_global] replica of every node's version (immutable during a wave)
    uint32_t* sent_bm;          // [n_global bits] remote targets already sent in this wave
    uint64_t sent_words;
    uint32_t* send_buf;         // [world][block] outgoing target ids per owner
    uint32_t* recv_buf;         // [world * block] incoming, concatenated
    unsigned long long* send_cnt;   // [world + 2] device counters (targets per owner, then next F, T)
    uint32_t* front_global;     // [n_global bits] all-gathered invalidated bitmap (pull levels)
    uint64_t front_words_global;
    unsigned long long* scratch_u64;
};
bool part_view(fgi_graph* g, PartView* v);
// Exchange this level's messages over the partition's transport (RCCL, host collectives or an in-process
// group): the per-owner counts and the rank's next-level {F, T} by an all-gather of words, which the host
// waits for (glob = {sum F, sum T, sum sent}), the payload by the transport's variable-size exchange,
// stream-ordered. Returns the number of target ids received (concatenated at recv_buf) and sent.
fgi_status part_exchange(fgi_graph* g, uint64_t* n_recv, uint64_t* n_sent, uint64_t* glob);
// src[0, words) of device memory into the fine-grained host buffer dst (words + 2 long), the host
// spinning on the sequence word dst[words]; dst[words + 1] = the publish's device wall-clock stamp
// (wave.hip). wall_ms: milliseconds between two such stamps (WaveCtr::t0 is one).
fgi_status publish_wait(fgi_graph* g, hipStream_t s, const unsigned long long* src, uint32_t words, unsigned long long* dst);
float wall_ms(fgi_graph* g, uint64_t t0, uint64_t t1);
// Sum of count (1..kPartRedMax) device u64 over all ranks, returned on the host.
fgi_status part_allreduce_sum(fgi_graph* g, const unsigned long long* dev_val, uint64_t* out,
                              uint32_t count = 1);
// The invalidated bitmap of all ranks' slots into front_global before a pull level, stream-ordered: every
// rank's words all-gathered, or only the changed ones (FGI_OPT_FRONT_EXCHANGE; the host waits for their count)
fgi_status part_allgather_front(fgi_graph* g);
// zero front_global at a wave's start (the delta exchange's baseline)
fgi_status part_front_reset(fgi_graph* g);
// Planned waves (run_part_wave): the full frontier all-gather and the fixed-size bucket all-to-all,
// stream-ordered (no host synchronisation), and the buffers they move.
constexpr uint32_t kPartRedMax = 160;   // words of one all-reduce (part_allreduce_sum)
struct PartBuckets {
    uint32_t C;                        // words per peer: count, then up to C - 1 target ids
    uint32_t* send;                    // [world][C]
    uint32_t* recv;                    // [world][C]
    unsigned long long* cur;           // [world] the next send_buf id to pack per owner
    unsigned long long* red;           // [kPartRedMax] device all-reduce source
};
fgi_status part_allgather_front_full(fgi_graph* g);
uint64_t part_plan_key(const fgi_graph* g);
fgi_status part_alltoall_async(fgi_graph* g);
PartBuckets part_buckets(fgi_graph* g);
// FGI_OPT_PART_BUCKET: words per peer of the planned waves' buckets (0: all that is allocated)
fgi_status part_set_bucket(fgi_graph* g, int64_t words);
// Partitioned mutations (graph.hip): a u32 array summed over the ranks in place (synchronises); the
// current-node bitmaps of the partitioned prune (this rank's, every rank's all-gathered); the
// dependency-entry store's append from device arrays.
fgi_status part_allreduce_u32(fgi_graph* g, uint32_t* dev, uint64_t n);
fgi_status part_cur_buffers(fgi_graph* g, unsigned long long** local, unsigned long long** all, uint64_t* w64);
fgi_status part_allgather_cur(fgi_graph* g);
fgi_status part_store_in_dev(fgi_graph* g, const uint64_t* keys, const uint64_t* tags, uint64_t m);
// the dependency entries whose used end is one of the global slots listed (host, any order) die:
// their node was displaced while it stayed current (Computing, or a delayed invalidation pending)
fgi_status part_kill_used(fgi_graph* g, std::vector<uint32_t> slots);
// frontier exchanges of each kind so far and the bytes this rank received through them
fgi_status part_front_stats(fgi_graph* g, uint64_t* full, uint64_t* delta, uint64_t* bytes);
// Rebuild a partition's pull lists from its dependency-entry store if rows or versions changed.
fgi_status part_ensure_lists(fgi_graph* g);
// Partitioned wave over global root ids (wave.hip): run_part_wave drives the phases below.
fgi_status run_part_wave(fgi_graph* g, uint32_t n_roots, const uint32_t* roots_dev, const uint8_t* imm_dev,
                         fgi_wave_stats* stats);
// Opens a partitioned call's flagged records (fgi_part_last_flagged): forgets the previous call's, and on a
// graph that can flag sizes the record buffer for 2 * (n_handles + extra) records and `cascades` marks
// and clears the cursor. run_part_wave opens a call of one cascade itself; fgi_part_run_batch opens its
// own (pflg_batch) with its begin_compute entries as `extra`.
fgi_status part_flagged_begin(fgi_graph* g, uint64_t cascades, uint64_t extra);
// ---- a partitioned wave's result in the host's numbering (part_out.hip) ----
// What this rank's call that runs a cascade is (kPout*), said before the cascade starts (kPoutOther) and
// again once one wave's result stands (kPoutWave); the previous wave's bitmap and ids are forgotten.
// Touches host fields only.
inline void part_out_mark(fgi_graph* g, int kind) {
    g->pout_kind = kind;
    ++g->pout_serial;   // the rank's fan-out lists of the wave before are forgotten too (fanout.hip)
    if (g->pout) g->pout->bits_valid = g->pout->ids_valid = false;
}
// n host roots (global slots) and their `immediately` bytes (nullable) through the graph's pinned buffer
// into its device copies, on the graph's stream; nothing waits
fgi_status part_out_stage_roots(fgi_graph* g, uint32_t n, const uint32_t* roots, const uint8_t* imm, uint32_t** roots_dev,
                                uint8_t** imm_dev);
// the last wave's bitmap over the rank's boundary handles / its ascending global ids, on the device
// (queued on the graph's stream; part_out_ids waits for its count check, and for the copy of the list to
// host_copy if that is given)
fgi_status part_out_bits(fgi_graph* g, const unsigned long long** bits_dev, uint64_t* words);
fgi_status part_out_ids(fgi_graph* g, const uint32_t** ids_dev, uint32_t* host_copy);
void part_out_destroy(fgi_graph* g);
// ---- replica fan-out (fanout.hip) ----
// A call that runs cascades says so before it starts (fgi_restore: kCascNone): the previous wave's fan-out
// lists are forgotten. Touches host fields only.
inline void fanout_note(fgi_graph* g, int kind) {
    ++g->casc_serial;
    g->casc_kind = kind;
}
// whether the graph holds subscriptions (everything below is a no-op returning FGI_OK otherwise)
inline bool fanout_live(const fgi_graph* g) { return g->fan && g->fan->live; }
// the entries of from[i] move to to[i] (boundary handles, host arrays; to[i] == FGI_NONE: nothing moves)
fgi_status fanout_move(fgi_graph* g, uint32_t n, const uint32_t* from, const uint32_t* to);
// the entries of the listed boundary handles (host array) are dropped
fgi_status fanout_drop_handles(fgi_graph* g, uint32_t n, const uint32_t* handles);
void fanout_destroy(fgi_graph* g);
// ---- delay timers (timers.hip) ----
// whether the graph's timers are open (everything below is a no-op returning FGI_OK otherwise)
inline bool timers_on(const fgi_graph* g) { return g->tim != nullptr; }
// the arm rule over flagged records (boundary handle << 32 | flags) on the device: n_max of them, or *n_dev
// if that is less (n_dev nullable). Queued on the graph's stream; nothing waits.
fgi_status timers_arm_records(fgi_graph* g, const unsigned long long* rec, uint64_t n_max, const unsigned long long* n_dev);
// a rank of a partition (fgi_part_timers_open): the arm rule over the records the call's cascades left in prec,
// counted by pcur[0] on the device, on the states the call left. Called once behind the call's last cascade and
// its moves by every fgi_part_* entry point that runs cascades; queued on the rank's stream, nothing waits. A
// no-op when the call ran no cascade or the rank cannot flag.
fgi_status timers_arm_part(fgi_graph* g);
// displaced nodes: the entry (from[i], the version of the node now at to[i]) moves to to[i], else the arm
// rule runs on to[i]; to[i] takes from[i]'s delay (boundary handles, host arrays, from[] distinct; to[i] ==
// FGI_NONE: nothing happens)
fgi_status timers_move(fgi_graph* g, uint32_t n, const uint32_t* from, const uint32_t* to);
// the entries of the listed boundary handles (host array) are dropped
fgi_status timers_drop_handles(fgi_graph* g, uint32_t n, const uint32_t* handles);
// fgi_restore: every entry is dropped; the clock and the delays stay
fgi_status timers_restore(fgi_graph* g);
void timers_destroy(fgi_graph* g);
// auto-invalidation (C-ABI 0.13): whether fgi_timers_auto_open was called on the graph's open timers
bool timers_auto_on(const fgi_graph* g);
// The auto arm rule over n candidates, queued behind whatever the stream holds, then one wait (the host arrays
// are the caller's: consumed when this returns) unless wait is false: then the host arrays stay as they are until
// the caller's timers_wait. Candidate i is handle[i] (boundary handle, host; FGI_NONE: none)
// if its set code is 1 (code_dev, a device array, or code_host; both null: every item is a candidate; 2 = set
// with InvalidateOnSetOutput, 0 = not set: no candidate). src (host, nullable): the handle whose delay codes
// item i reads, where that is not handle[i] (a batch's node that a later step moved). transient (host,
// nullable): item i picks the transient-error delay.
fgi_status timers_arm_auto(fgi_graph* g, uint32_t n, const uint32_t* handle, const uint32_t* src, const uint8_t* code_dev,
                           const uint8_t* code_host, const uint8_t* transient, bool wait = true);
// The same rule on a rank of a partition with auto open (fgi_part_timers_auto_open; else a no-op), queued on the
// rank's stream: nothing waits, nothing is copied. Every array is the device's: item i names the host's global
// slot slot_dev[i] (a slot of another rank is skipped), code_dev[i] is its set code (nullable: every item is a
// candidate), transient_dev[i] its transient flag (nullable).
fgi_status timers_arm_auto_part(fgi_graph* g, uint32_t n, const uint32_t* slot_dev, const uint8_t* code_dev,
                                const uint8_t* transient_dev);
// waits for what the timers' hooks queued and reads their counters
fgi_status timers_wait(fgi_graph* g);
// ---- sharded loads (shard.hip) ----
// Their collectives, over the partition's transport (part.hip, PartComm): host words (at most kShardWords
// per rank) all-gathered on the host; device byte ranges with per-peer counts, all-gathered (src[0,
// bytes[rank]) of every rank in rank order at dst) or exchanged (src + soff[q], sbytes[q] bytes, to rank q;
// rbytes[q] bytes from rank q at dst + roff[q]; a range may be empty). Each returns with the data in place.
constexpr uint32_t kShardWords = 24;
fgi_status part_allgather_words(fgi_graph* g, const uint64_t* mine, uint32_t words, uint64_t* all);
fgi_status part_allgatherv(fgi_graph* g, const void* src, const uint64_t* bytes, void* dst);
fgi_status part_alltoallv(fgi_graph* g, const void* src, const uint64_t* soff, const uint64_t* sbytes, void* dst,
                          const uint64_t* roff, const uint64_t* rbytes);
uint32_t* part_weight(fgi_graph* g);   // [n_global] live dependencies per slot (code order once codes exist)
// the first bulk load of a partition that wants codes; the choice (weight_dev: [n_global] by slot, left in code
// order); the pull lists rebuilt from the dependency-entry store
bool part_codes_now(fgi_graph* g);
fgi_status part_codes_choose(fgi_graph* g, uint32_t* weight_dev);
fgi_status part_rebuild_lists(fgi_graph* g);
// fn(rank) on one host thread per rank of the in-process group gs[0, P)
fgi_status part_local_run(fgi_graph* const* gs, uint32_t P, const std::function<fgi_status(uint32_t)>& fn);
// load_rows from device arrays (left untouched)
fgi_status load_rows_dev(fgi_graph* g, uint64_t m, const uint64_t* dev_keys, const uint64_t* dev_tags, uint32_t src_base,
                         uint32_t dst_base);
}  // namespace fgi

#define FGI_HIP(g, call)                                                   \
    do {                                                                   \
        hipError_t _e = (call);                                            \
        if (_e != hipSuccess) return fgi::hip_check((g), _e, #call);       \
    } while (0)
#define FGI_TRY(call)                          \
    do {                                       \
        fgi_status _s = (call);                \
        if (_s != FGI_OK) return _s;           \
    } while (0)

// ---- device memory of a call and of the graph -----------------------------------------
namespace fgi {
template <class T>
fgi_status dmalloc(fgi_graph* g, T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
    if (e != hipSuccess) return hip_check(g, e, "hipMalloc");
    return FGI_OK;
}

template <class T>
void dfree(T*& p) {
    if (p) hipFree(p);
    p = nullptr;
}

// a fresh device allocation until its owner takes it (buffers that grow by copying)
template <class T>
struct DevOwn {
    T* p = nullptr;
    DevOwn() = default;
    DevOwn(const DevOwn&) = delete;
    DevOwn& operator=(const DevOwn&) = delete;
    ~DevOwn() { dfree(p); }
    T* release() {
        T* q = p;
        p = nullptr;
        return q;
    }
};

// An owned (pointer, capacity) pair that grows by replacement: the contents are not kept. `what` names
// the buffer in the error ("the fan-out's tile counts").
template <class T>
fgi_status grow(fgi_graph* g, T** p, uint64_t* cap, uint64_t need, const char* what) {
    if (*cap >= need && (*p || !need)) return FGI_OK;
    dfree(*p);
    *cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(p), need * sizeof(T)) != hipSuccess) {
        *p = nullptr;
        return set_err(g, FGI_ENOMEM, "%s (%llu entries)", what, (unsigned long long)need);
    }
    *cap = need;
    return FGI_OK;
}

// Device temporaries of one ABI call. Small ones (power-of-two size classes up to kTmpKeepMax,
// kTmpKeepTotal in all) go back to the graph's cache when their scope ends (or at reset()); every user
// of a temporary runs on the graph's stream, so a later reuse is ordered after it. A request above
// kTmpKeepMax never enters the cache and is allocated at its exact size. A block's contents are
// undefined: FGI_TMP_POISON=1 (read at fgi_create) fills every block handed out with 0xA5 bytes.
constexpr size_t kTmpKeepMax = 64ull << 20;
constexpr size_t kTmpKeepTotal = 512ull << 20;
void tmp_release(fgi_graph* g, void* p, size_t bytes);
void tmp_drain(fgi_graph* g);
struct Tmp {
    fgi_graph* g = nullptr;
    void* p = nullptr;
    size_t bytes = 0;
    Tmp() = default;
    Tmp(Tmp&& o) noexcept : g(o.g), p(o.p), bytes(o.bytes) { o.p = nullptr; }
    Tmp& operator=(const Tmp&) = delete;
    void reset() {
        if (p) tmp_release(g, p, bytes);
        p = nullptr;
        bytes = 0;
    }
    ~Tmp() { reset(); }
};
fgi_status tmp_take(fgi_graph* g, Tmp& t, size_t bytes);
template <class T>
fgi_status tmalloc(fgi_graph* g, Tmp& t, T** p, size_t count) {
    *p = nullptr;
    FGI_TRY(tmp_take(g, t, (count ? count : 1) * sizeof(T)));
    *p = reinterpret_cast<T*>(t.p);
    return FGI_OK;
}

inline void RootStage::release() {
    if (h) (void)hipHostFree(h);
    h = nullptr;
    dfree(d);
    cap = 0;
}
inline fgi_status RootStage::stage(fgi_graph* g, uint32_t n, const uint32_t* roots, const uint8_t* imm, uint32_t** roots_dev,
                                   uint8_t** imm_dev) {
    if (cap < n || !h) {
        release();
        const uint64_t c = n > 4096 ? n : 4096;
        if (hipHostMalloc(reinterpret_cast<void**>(&h), c * 5, hipHostMallocDefault) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&d), c * 5) != hipSuccess) {
            release();
            return set_err(g, FGI_ENOMEM, "the staging of %u host roots", n);
        }
        cap = c;
    }
    *roots_dev = reinterpret_cast<uint32_t*>(d);
    *imm_dev = nullptr;
    if (!n) return FGI_OK;
    memcpy(h, roots, (size_t)n * 4);
    FGI_HIP(g, hipMemcpyAsync(d, h, (size_t)n * 4, hipMemcpyHostToDevice, g->stream));
    if (imm) {
        memcpy(h + cap * 4, imm, n);
        FGI_HIP(g, hipMemcpyAsync(d + cap * 4, h + cap * 4, n, hipMemcpyHostToDevice, g->stream));
        *imm_dev = reinterpret_cast<uint8_t*>(d + cap * 4);
    }
    return FGI_OK;
}
}  // namespace fgi
