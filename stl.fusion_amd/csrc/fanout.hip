// fanout.hip — the replica fan-out on the device (C-ABI 0.9): fgi_subscribe,
// fgi_last_wave_fanout, fgi_fanout_ids, fgi_unsubscribe_peer, fgi_sub_stats_get; and per rank of a partition
// (C-ABI 0.10): fgi_part_subscribe, fgi_part_last_wave_fanout, fgi_part_fanout_ids, fgi_part_fanout_detached,
// fgi_part_unsubscribe_peer, over the rank's own handles, sources and outputs in the host's numbering.
//
// The table (fgi::Fanout) chains 16-byte records {call id, peer, next} from a head per boundary handle, with
// a has-entries bitmap beside it. A fan-out joins it with an invalidated set given as a bitmap over boundary
// handles or as an ascending handle list, and returns the call ids grouped by peer, within a peer by
// ascending handle, with no sort:
//   k_fo_count   one wavefront per tile (a run of bitmap words, or of list entries): the tile's entries per
//                peer in an LDS histogram, written tile-major
//   k_fo_scan    one wavefront per peer: its counts over the tiles to their exclusive scan, and its total
//   k_fo_offs    one block: the peers' totals to peer_off
//   k_fo_write   the tiles again: a tile's cursor per peer is peer_off[p] + its scanned count. The entries of
//                64 handles are staged in LDS in handle order and emitted 64 at a time; the rank among lanes
//                with the same peer comes from a ballot loop over the distinct peers present. What is
//                delivered is unlinked, and record i of the output goes to the free stack at free_n + i.
//   k_fo_probe   a partition rank with codes: inv & has in handle order, probed from the subscribed handles
// No kernel waits on another block, and every chain walk is capped at the pool size: a longer chain sets an
// error word and the call fails with FGI_ESTATE.
// Everything is allocated at the first fgi_subscribe; a graph that never subscribes launches nothing here.
#include "fgi_internal.h"

#include <algorithm>
#include <cstring>

namespace fgi {
namespace {

constexpr int kFBlock = 256;          // threads per block of the element-wise kernels
constexpr uint32_t kFoStage = 512;    // entries staged in LDS per round of k_fo_write
constexpr uint32_t kFoMaxTiles = 4096;
constexpr uint64_t kFoMaxCounts = 1ull << 22;   // tiles x peers of the count table (16 MB)
// device counters of a call (Fanout::ctr)
enum { kCStored = 0, kCDropped = 1, kCErrChain = 2, kCErrPeer = 3, kCErrOut = 4, kCWords = 8 };

struct SubArgs {
    uint32_t n;
    const uint32_t* handle;
    const uint32_t* peer;
    const unsigned long long* call;
    uint32_t* result;
    const unsigned long long* node;
    const uint32_t* vis;        // null: no unfolded visits
    const uint32_t* s2l;        // null: no hot labels
    uint32_t ext_slots, K;
    uint32_t* head;
    unsigned long long* has;
    SubRec* rec;
    const uint32_t* fstack;
    uint64_t free_n, bump, cap;
    unsigned long long* pcnt;
    unsigned long long* ctr;
    // a partition rank (fgi_part_subscribe): handle[] holds global slots, of which the rank owns
    // [base, base + n_local); gc: slot -> code, null without partition codes. No partition: all zero.
    bool part;
    uint32_t base, n_local;
    const uint32_t* gc;
};

// One entry per thread. The node's state is its word and its visit bit: nothing is folded.
// A stored entry takes record number i of the call (one atomic per wavefront): the free stack's top first,
// then the never-used range; the host checked that n records are there.
// On a partition rank the entry's handle is slot - base and its node sits at engine index gc[slot] - base
// (view.hip's view_label); an entry of a slot the rank does not own writes its result and takes no record.
__global__ __launch_bounds__(kFBlock) void k_sub_insert(SubArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    bool store = false;
    uint32_t h = 0, p = 0;
    if (i < a.n) {
        h = a.handle[i];
        p = a.peer[i];
        uint32_t l = h + a.K;
        bool owned = true;
        if (a.part) {   // (a partition has no hub-first labels, part_alloc drops them: K = 0, no s2l, as view_label)
            const uint32_t slot = h;
            h = slot - a.base;
            owned = h < a.n_local;   // (a slot below base wraps past n_local)
            l = h;
            if (owned && a.gc) {
                l = a.gc[slot] - a.base;
                owned = l < a.n_local;   // a code stays in its owner's range (part_out.hip checks the same)
            }
        } else if (a.s2l && h < a.ext_slots) {
            const uint32_t hot = a.s2l[h];
            if (hot != FGI_NONE) l = hot;
        }
        if (owned) {
            unsigned long long w = a.node[l];
            if (a.vis && ((a.vis[l >> 5] >> (l & 31)) & 1u)) w = visited_word(w);
            store = (w & kVMask) != 0 && word_state(w) != FGI_INVALIDATED;
        }
        if (a.result) a.result[i] = !owned ? FGI_SUB_NOT_OWNED : store ? FGI_SUB_ADDED : FGI_SUB_INVALIDATED;
    }
    const unsigned long long m = __ballot(store);
    if (!m) return;
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if ((int)lane == leader) base = atomicAdd(a.ctr + kCStored, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    if (!store) return;
    const uint64_t k = base + __popcll(m & ((1ull << lane) - 1));
    const uint64_t r64 = k < a.free_n ? a.fstack[a.free_n - 1 - k] : a.bump + (k - a.free_n);
    if (r64 >= a.cap) {   // never with the host's capacity check
        atomicAdd(a.ctr + kCErrOut, 1ull);
        return;
    }
    const uint32_t r = (uint32_t)r64;
    const uint32_t old = atomicExch(a.head + h, r);
    a.rec[r] = SubRec{a.call[i], p, old};
    atomicOr(a.has + (h >> 6), 1ull << (h & 63));
    atomicAdd(a.pcnt + p, 1ull);
}

// What the count and write passes share. Bitmap source: tile t covers words [t * per, (t + 1) * per) of
// inv & has. List source: entries [t * per, (t + 1) * per) of ids, per a multiple of 64.
struct FoArgs {
    const unsigned long long* inv;   // bitmap source (64-bit words over boundary handles), or null
    const uint32_t* ids;             // list source
    uint64_t n_ids;
    uint64_t words;                  // bitmap words of the table
    uint32_t n_handles;              // handles that may join: the table's, or a partition rank's owned slots
    uint32_t id_base;                // list source: an id's handle is id - id_base (a rank's first slot; else 0)
    uint32_t hnd_base;               // added to a handle on its way out (a rank's slots leave as global ids)
    uint32_t per;
    uint32_t n_tiles, n_peers;
    uint32_t* head;
    unsigned long long* has;
    SubRec* rec;
    uint64_t cap;
    uint32_t* tcnt;
    const unsigned long long* off;
    unsigned long long* out_call;
    uint32_t* out_hnd;
    uint64_t out_n;
    uint32_t* fstack;
    uint64_t free_n;
    unsigned long long* ctr;
};

// the handle of lane `lane` in group gi of tile t, and whether it is in the set and has entries
template <bool kList>
__device__ inline bool fo_lane(const FoArgs& a, uint32_t t, uint32_t gi, uint32_t lane, uint32_t* h) {
    if (kList) {
        const uint64_t i = (uint64_t)t * a.per + (uint64_t)gi * 64 + lane;
        if (i >= a.n_ids) return false;
        const uint32_t x = a.ids[i] - a.id_base;   // (an id below the base wraps past n_handles: not owned)
        *h = x;
        return x < a.n_handles && ((a.has[x >> 6] >> (x & 63)) & 1ull);
    }
    const uint64_t word = (uint64_t)t * a.per + gi;
    if (word >= a.words) return false;
    const unsigned long long w = a.inv[word] & a.has[word];
    const uint64_t x = word * 64 + lane;
    *h = (uint32_t)x;
    return ((w >> lane) & 1ull) && x < a.n_handles;
}
template <bool kList>
__device__ inline uint32_t fo_groups(const FoArgs& a) { return kList ? a.per / 64 : a.per; }

template <bool kList>
__global__ __launch_bounds__(64) void k_fo_count(FoArgs a) {
    extern __shared__ uint32_t s_cnt[];
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    for (uint32_t p = lane; p < a.n_peers; p += 64) s_cnt[p] = 0;
    __syncthreads();
    const uint32_t groups = fo_groups<kList>(a);
    for (uint32_t gi = 0; gi < groups; ++gi) {
        uint32_t h = 0;
        if (!fo_lane<kList>(a, t, gi, lane, &h)) continue;
        uint32_t r = a.head[h];
        uint64_t steps = 0;
        while (r != FGI_NONE) {
            if (r >= a.cap || ++steps > a.cap) {
                atomicAdd(a.ctr + kCErrChain, 1ull);
                break;
            }
            const SubRec e = a.rec[r];
            if (e.peer < a.n_peers) atomicAdd(&s_cnt[e.peer], 1u);
            else atomicAdd(a.ctr + kCErrPeer, 1ull);
            r = e.next;
        }
    }
    __syncthreads();
    for (uint32_t p = lane; p < a.n_peers; p += 64) a.tcnt[(uint64_t)t * a.n_peers + p] = s_cnt[p];
}

__device__ inline uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if ((int)lane >= d) v += o;
    }
    return v;
}

// block p: peer p's counts over the tiles -> their exclusive scan in place; tot[p] = the peer's entries
__global__ __launch_bounds__(64) void k_fo_scan(uint32_t* tcnt, uint32_t n_tiles, uint32_t n_peers, unsigned long long* tot) {
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    uint32_t run = 0;
    for (uint32_t base = 0; base < n_tiles; base += 64) {   // wave-uniform
        const uint32_t t = base + lane;
        const uint32_t v = t < n_tiles ? tcnt[(uint64_t)t * n_peers + p] : 0u;
        const uint32_t incl = wave_incl_scan(v, lane);
        if (t < n_tiles) tcnt[(uint64_t)t * n_peers + p] = run + incl - v;
        run += __shfl(incl, 63);
    }
    if (lane == 0) tot[p] = run;
}

// one block: off[0 .. n_peers] = exclusive scan of tot[0, n_peers); a live entry of a peer >= n_peers is an error
__global__ __launch_bounds__(kFBlock) void k_fo_offs(const unsigned long long* tot, uint32_t n_peers, unsigned long long* off,
                                                     const unsigned long long* pcnt, unsigned long long* ctr) {
    __shared__ unsigned long long s_p[kFBlock];
    const uint32_t seg = (n_peers + kFBlock - 1) / kFBlock;
    const uint32_t lo = min(n_peers, threadIdx.x * seg), hi = min(n_peers, lo + seg);
    unsigned long long sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += tot[i];
    s_p[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int k = 0; k < kFBlock; ++k) {
            const unsigned long long v = s_p[k];
            s_p[k] = run;
            run += v;
        }
        off[n_peers] = run;
    }
    __syncthreads();
    unsigned long long run = s_p[threadIdx.x];
    for (uint32_t i = lo; i < hi; ++i) {
        off[i] = run;
        run += tot[i];
    }
    bool bad = false;
    for (uint32_t p = n_peers + threadIdx.x; p < FGI_MAX_PEERS; p += kFBlock) bad |= pcnt[p] != 0;
    if (bad) atomicAdd(ctr + kCErrPeer, 1ull);
}

// the delivered entries leave the peers' live counts (queued before the write pass)
__global__ __launch_bounds__(kFBlock) void k_fo_commit(const unsigned long long* tot, uint32_t n_peers, unsigned long long* pcnt) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n_peers) pcnt[p] -= min(pcnt[p], tot[p]);
}

template <bool kList>
__global__ __launch_bounds__(64) void k_fo_write(FoArgs a) {
    extern __shared__ uint32_t s_cur[];
    __shared__ uint32_t s_rec[kFoStage];
    __shared__ uint32_t s_hnd[kFoStage];
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    for (uint32_t p = lane; p < a.n_peers; p += 64)
        s_cur[p] = (uint32_t)a.off[p] + a.tcnt[(uint64_t)t * a.n_peers + p];
    __syncthreads();
    const uint32_t groups = fo_groups<kList>(a);
    for (uint32_t gi = 0; gi < groups; ++gi) {   // wave-uniform
        uint32_t h = 0;
        const bool act = fo_lane<kList>(a, t, gi, lane, &h);
        if (!__ballot(act)) continue;
        uint32_t cur = act ? a.head[h] : FGI_NONE;
        uint64_t steps = 0;
        // Rounds: the lanes' remaining chains are staged in lane (= handle) order, as many whole chains as
        // fit; a chain that does not fit is staged as far as the room goes and no later lane stages anything
        // (its excl is past the room), so a handle's entries never follow a higher handle's.
        while (__ballot(cur != FGI_NONE)) {
            uint32_t len = 0;
            for (uint32_t r = cur; r != FGI_NONE && len <= kFoStage;) {
                if (r >= a.cap) {
                    atomicAdd(a.ctr + kCErrChain, 1ull);
                    if (len == 0) cur = FGI_NONE;
                    break;
                }
                ++len;
                r = a.rec[r].next;
            }
            const uint32_t incl = wave_incl_scan(len, lane), excl = incl - len;
            const uint32_t take = excl >= kFoStage ? 0u : min(len, kFoStage - excl);
            for (uint32_t k = 0; k < take; ++k) {
                s_rec[excl + k] = cur;
                s_hnd[excl + k] = h;
                cur = a.rec[cur].next;
            }
            steps += take;
            if (steps > a.cap) {   // a cycle: the chain is longer than the pool
                atomicAdd(a.ctr + kCErrChain, 1ull);
                cur = FGI_NONE;
            }
            const uint32_t total = min(__shfl(incl, 63), kFoStage);
            __syncthreads();
            for (uint32_t c = 0; c < total; c += 64) {   // wave-uniform
                const uint32_t i = c + lane;
                bool valid = i < total;
                uint32_t r = 0, hh = 0, peer = 0;
                unsigned long long call = 0;
                if (valid) {
                    r = s_rec[i];
                    hh = s_hnd[i];
                    const SubRec e = a.rec[r];
                    peer = e.peer;
                    call = e.call;
                    valid = peer < a.n_peers;   // (the count pass failed the call otherwise)
                }
                unsigned long long todo = __ballot(valid);
                while (todo) {   // one step per distinct peer among the 64 entries
                    const int leader = __ffsll((long long)todo) - 1;
                    const uint32_t p0 = __shfl(peer, leader);
                    const bool mine = valid && peer == p0;
                    const unsigned long long m = __ballot(mine);
                    uint32_t base = 0;
                    if ((int)lane == leader) {
                        base = s_cur[p0];
                        s_cur[p0] = base + (uint32_t)__popcll(m);
                    }
                    base = __shfl(base, leader);
                    if (mine) {
                        const uint64_t pos = (uint64_t)base + __popcll(m & ((1ull << lane) - 1));
                        if (pos < a.out_n && a.free_n + pos < a.cap) {
                            a.out_call[pos] = call;
                            a.out_hnd[pos] = hh + a.hnd_base;
                            a.fstack[a.free_n + pos] = r;
                        } else {
                            atomicAdd(a.ctr + kCErrOut, 1ull);
                        }
                    }
                    todo &= ~m;
                }
            }
            __syncthreads();
        }
        if (act) {   // delivered: unlinked
            a.head[h] = FGI_NONE;
            atomicAnd(a.has + (h >> 6), ~(1ull << (h & 63)));
        }
    }
}

// an ascending id list as a bitmap over handles id - id_base (zeroed first)
__global__ __launch_bounds__(kFBlock) void k_fo_scatter(const uint32_t* ids, uint64_t n, uint32_t id_base, uint32_t n_handles,
                                                        unsigned long long* bits) {
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthr) {
        const uint32_t h = ids[i] - id_base;
        if (h < n_handles) atomicOr(bits + (h >> 6), 1ull << (h & 63));
    }
}

// A partition rank's wave with codes, joined where the subscriptions are: inv64 is the wave's bitmap over
// engine indices, has is over handles, and owned handle h sits at engine index gc[base + h] - base. A
// wavefront per word x of has (grid-strided, wave-uniform trip count): a zero word stores 0; otherwise the
// lanes whose has bit is set probe their handle's bit of inv64, and one ballot is the word inv & has in
// handle order, stored whole by lane 0. The code table and the bitmap are read for subscribed handles only.
__global__ __launch_bounds__(kFBlock) void k_fo_probe(const unsigned long long* __restrict__ inv64,
                                                      const unsigned long long* __restrict__ has,
                                                      const uint32_t* __restrict__ gc, uint32_t base, uint32_t n_local,
                                                      unsigned long long* out, uint64_t words) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t x = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; x < words; x += nwaves) {   // wave-uniform
        const unsigned long long hw = has[x];
        if (!hw) {   // wave-uniform: every lane read the same word
            if (lane == 0) out[x] = 0ull;
            continue;
        }
        const uint64_t h = x * 64 + lane;
        bool hit = false;
        if (((hw >> lane) & 1ull) && h < n_local) {
            const uint32_t e = gc[base + (uint32_t)h] - base;
            hit = e < n_local && ((inv64[e >> 6] >> (e & 63)) & 1ull);
        }
        const unsigned long long w = __ballot(hit);
        if (lane == 0) out[x] = w;   // the wavefront owns word x: a plain store of the whole word
    }
}

struct EditArgs {
    uint32_t* head;
    unsigned long long* has;
    SubRec* rec;
    uint32_t* fstack;
    uint64_t free_n, cap;
    unsigned long long* pcnt;
    unsigned long long* ctr;
    uint32_t n_handles;
};

// pair i: the chain of from[i] goes in front of to[i]'s (handles distinct within a launch)
__global__ __launch_bounds__(kFBlock) void k_fo_move(EditArgs a, uint32_t n, const uint32_t* from, const uint32_t* to) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = from[i], d = to[i];
    if (d == FGI_NONE || f == d || f >= a.n_handles || d >= a.n_handles) return;
    const uint32_t hf = a.head[f];
    if (hf == FGI_NONE) return;
    const uint32_t hd = a.head[d];
    if (hd != FGI_NONE) {   // a detached handle handed out anew has none: released handles drop theirs
        uint32_t r = hf;
        uint64_t steps = 0;
        while (true) {
            if (r >= a.cap || ++steps > a.cap) {
                atomicAdd(a.ctr + kCErrChain, 1ull);
                return;
            }
            const uint32_t nx = a.rec[r].next;
            if (nx == FGI_NONE) break;
            r = nx;
        }
        a.rec[r].next = hd;
    }
    a.head[d] = hf;
    a.head[f] = FGI_NONE;
    atomicOr(a.has + (d >> 6), 1ull << (d & 63));
    atomicAnd(a.has + (f >> 6), ~(1ull << (f & 63)));
}

// the entries of handle h for which `all` holds or whose peer is `peer` go to the free stack
__device__ inline void fo_drop(const EditArgs& a, uint32_t h, bool all, uint32_t peer) {
    uint32_t r = a.head[h], keep = FGI_NONE;
    uint64_t steps = 0;
    while (r != FGI_NONE) {
        if (r >= a.cap || ++steps > a.cap) {
            atomicAdd(a.ctr + kCErrChain, 1ull);
            return;
        }
        const SubRec e = a.rec[r];
        if (all || e.peer == peer) {
            const unsigned long long k = atomicAdd(a.ctr + kCDropped, 1ull);
            if (a.free_n + k < a.cap) a.fstack[a.free_n + k] = r;
            else atomicAdd(a.ctr + kCErrOut, 1ull);
            if (e.peer < FGI_MAX_PEERS) atomicAdd(a.pcnt + e.peer, ~0ull);   // - 1
        } else {
            a.rec[r].next = keep;   // (the order within a handle is unspecified)
            keep = r;
        }
        r = e.next;
    }
    a.head[h] = keep;
    if (keep == FGI_NONE) atomicAnd(a.has + (h >> 6), ~(1ull << (h & 63)));
}

__global__ __launch_bounds__(kFBlock) void k_fo_drop_handles(EditArgs a, uint32_t n, const uint32_t* handles) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = handles[i];
    for (uint32_t j = 0; j < i; ++j)   // a handle listed twice is dropped once (released lists are short)
        if (handles[j] == h) return;
    if (h < a.n_handles && ((a.has[h >> 6] >> (h & 63)) & 1ull)) fo_drop(a, h, true, 0);
}

__global__ __launch_bounds__(kFBlock) void k_fo_drop_peer(EditArgs a, uint32_t peer) {
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < a.n_handles; h += nthr)
        if ((a.has[h >> 6] >> (h & 63)) & 1ull) fo_drop(a, (uint32_t)h, false, peer);
}

inline uint32_t fgrid(uint64_t n) { return (uint32_t)std::min<uint64_t>(4096, std::max<uint64_t>(1, (n + kFBlock - 1) / kFBlock)); }

// the table, allocated at the first fgi_subscribe
fgi_status fan_create(fgi_graph* g) {
    if (g->fan) return FGI_OK;
    Fanout* f = new Fanout();
    g->fan = f;
    f->words = ((uint64_t)g->ext_handles + 63) / 64;
    hipStream_t s = g->stream;
    if (hipMalloc(reinterpret_cast<void**>(&f->head), (size_t)g->ext_handles * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&f->has), f->words * 8) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&f->bits), f->words * 8) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&f->pcnt), FGI_MAX_PEERS * 8) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&f->tot), FGI_MAX_PEERS * 8) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&f->off), (FGI_MAX_PEERS + 1) * 8) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&f->ctr), kCWords * 8) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&f->ctr_h), (kCWords + 1) * 8, hipHostMallocDefault) != hipSuccess) {
        fanout_destroy(g);
        return set_err(g, FGI_ENOMEM, "the subscription table of %u handles", g->ext_handles);
    }
    for (int k = 0; k < 6; ++k)
        if (hipEventCreate(&f->ev[k]) != hipSuccess) {
            fanout_destroy(g);
            return set_err(g, FGI_EDEVICE, "the fan-out's timing events");
        }
    FGI_HIP(g, hipMemsetAsync(f->head, 0xFF, (size_t)g->ext_handles * 4, s));
    FGI_HIP(g, hipMemsetAsync(f->has, 0, f->words * 8, s));
    FGI_HIP(g, hipMemsetAsync(f->pcnt, 0, FGI_MAX_PEERS * 8, s));
    return FGI_OK;
}

// room for `need` more records: the pool grows like the edge pool (a fresh allocation, the records copied)
fgi_status fan_reserve(fgi_graph* g, uint64_t need) {
    Fanout* f = g->fan;
    if (f->free_n + (f->cap - f->bump) >= need) return FGI_OK;
    const uint64_t want = std::max<uint64_t>({f->bump + (need - f->free_n), 2 * f->cap, 1024});
    if (want >= FGI_NONE) return set_err(g, FGI_ENOMEM, "the subscription table holds at most 2^32 - 2 entries");
    DevOwn<SubRec> rec;   // until they are installed
    DevOwn<uint32_t> fs;
    if (hipMalloc(reinterpret_cast<void**>(&rec.p), want * sizeof(SubRec)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&fs.p), want * 4) != hipSuccess)
        return set_err(g, FGI_ENOMEM, "a subscription pool of %llu records", (unsigned long long)want);
    hipStream_t s = g->stream;
    if (f->bump) FGI_HIP(g, hipMemcpyAsync(rec.p, f->rec, f->bump * sizeof(SubRec), hipMemcpyDeviceToDevice, s));
    if (f->free_n) FGI_HIP(g, hipMemcpyAsync(fs.p, f->fstack, f->free_n * 4, hipMemcpyDeviceToDevice, s));
    FGI_HIP(g, hipStreamSynchronize(s));
    dfree(f->rec);
    dfree(f->fstack);
    f->rec = rec.release();
    f->fstack = fs.release();
    f->cap = want;
    return FGI_OK;
}

EditArgs edit_args(const fgi_graph* g) {
    const Fanout* f = g->fan;
    return EditArgs{f->head, f->has, f->rec, f->fstack, f->free_n, f->cap, f->pcnt, f->ctr, g->ext_handles};
}

// the call's counters back on the host (one wait)
fgi_status read_ctr(fgi_graph* g) {
    Fanout* f = g->fan;
    FGI_HIP(g, hipGetLastError());
    FGI_HIP(g, hipMemcpyAsync(f->ctr_h, f->ctr, kCWords * 8, hipMemcpyDeviceToHost, g->stream));
    FGI_HIP(g, hipStreamSynchronize(g->stream));
    return FGI_OK;
}
fgi_status check_chain(fgi_graph* g, const char* what) {
    const Fanout* f = g->fan;
    if (f->ctr_h[kCErrChain] || f->ctr_h[kCErrOut])
        return set_err(g, FGI_ESTATE, "%s: the subscription table is damaged (a chain longer than the pool of %llu records, "
                                      "or an output past its count)", what, (unsigned long long)f->cap);
    return FGI_OK;
}
// what a call that dropped entries leaves on the host
void account_dropped(Fanout* f) {
    const uint64_t d = std::min<uint64_t>(f->ctr_h[kCDropped], f->live);
    f->free_n += d;
    f->live -= d;
    f->dropped += d;
}

// how a source's ids and the table's handles relate (FoArgs): a single device joins the whole table as it is
struct FoMap {
    uint32_t n_handles, id_base, hnd_base;
};
inline FoMap whole_table(const fgi_graph* g) { return FoMap{g->ext_handles, 0u, 0u}; }
// a partition rank's owned slots: sources in the host's numbering, handles leave as global slots
inline FoMap owned_slots(const PartView& pv) { return FoMap{pv.n_local, pv.base, pv.base}; }

// The join: the invalidated set as a bitmap (inv) or as n_ids ascending ids, against the table. *total: the
// entries found. dry: count only (nothing leaves the table). The lists are left in out_call / out_hnd / off.
fgi_status fan_join(fgi_graph* g, const unsigned long long* inv, const uint32_t* ids, uint64_t n_ids, const FoMap& map,
                    uint32_t n_peers, uint64_t cap_or_all, const char* what, uint64_t* total, bool* wrote) {
    Fanout* f = g->fan;
    hipStream_t s = g->stream;
    const bool list = inv == nullptr;
    *wrote = false;
    const uint64_t max_tiles = std::max<uint64_t>(1, std::min<uint64_t>(kFoMaxTiles, kFoMaxCounts / n_peers));
    const uint64_t units = list ? (n_ids + 63) / 64 : f->words;   // groups of 64 handles
    const uint64_t gpt = std::max<uint64_t>(1, (units + max_tiles - 1) / max_tiles);   // groups per tile
    const uint32_t n_tiles = (uint32_t)std::max<uint64_t>(1, (units + gpt - 1) / gpt);
    FGI_TRY(grow(g, &f->tcnt, &f->tcnt_cap, (uint64_t)n_tiles * n_peers, "the fan-out's tile counts"));
    FoArgs a{};
    a.inv = inv;
    a.ids = ids;
    a.n_ids = n_ids;
    a.words = f->words;
    a.n_handles = map.n_handles;
    a.id_base = map.id_base;
    a.hnd_base = map.hnd_base;
    a.per = (uint32_t)(list ? gpt * 64 : gpt);
    a.n_tiles = n_tiles;
    a.n_peers = n_peers;
    a.head = f->head;
    a.has = f->has;
    a.rec = f->rec;
    a.cap = f->cap;
    a.tcnt = f->tcnt;
    a.off = f->off;
    a.fstack = f->fstack;
    a.free_n = f->free_n;
    a.ctr = f->ctr;
    const size_t lds = (size_t)n_peers * 4;
    FGI_HIP(g, hipMemsetAsync(f->ctr, 0, kCWords * 8, s));
    FGI_HIP(g, hipEventRecord(f->ev[0], s));
    if (list) hipLaunchKernelGGL(k_fo_count<true>, dim3(n_tiles), dim3(64), lds, s, a);
    else hipLaunchKernelGGL(k_fo_count<false>, dim3(n_tiles), dim3(64), lds, s, a);
    hipLaunchKernelGGL(k_fo_scan, dim3(n_peers), dim3(64), 0, s, f->tcnt, n_tiles, n_peers, f->tot);
    hipLaunchKernelGGL(k_fo_offs, dim3(1), dim3(kFBlock), 0, s, (const unsigned long long*)f->tot, n_peers, f->off,
                       (const unsigned long long*)f->pcnt, f->ctr);
    FGI_HIP(g, hipEventRecord(f->ev[1], s));
    FGI_HIP(g, hipMemcpyAsync(f->ctr_h + kCWords, f->off + n_peers, 8, hipMemcpyDeviceToHost, s));   // the total, beside the counters
    FGI_TRY(read_ctr(g));
    const uint64_t n = f->ctr_h[kCWords];
    *total = n;
    float ms = 0;
    f->last_ms = hipEventElapsedTime(&ms, f->ev[0], f->ev[1]) == hipSuccess ? ms : 0.0;
    ++f->fanouts;
    ++(list ? f->from_list : f->from_bits);
    FGI_TRY(check_chain(g, what));
    if (f->ctr_h[kCErrPeer])
        return set_err(g, FGI_EINVAL, "%s: n_peers = %u, a stored entry names a peer at or past it", what, n_peers);
    if (n > f->live) return set_err(g, FGI_ESTATE, "%s: %llu entries found, %llu stored", what, (unsigned long long)n,
                                    (unsigned long long)f->live);
    if (n == 0 || n > cap_or_all) return FGI_OK;
    uint64_t hnd_cap = f->out_cap;   // the two lists grow together
    FGI_TRY(grow(g, &f->out_hnd, &hnd_cap, std::max<uint64_t>(n, 4096), "the fan-out's lists"));
    FGI_TRY(grow(g, &f->out_call, &f->out_cap, std::max<uint64_t>(n, 4096), "the fan-out's lists"));
    a.out_call = f->out_call;
    a.out_hnd = f->out_hnd;
    a.out_n = n;
    FGI_HIP(g, hipEventRecord(f->ev[2], s));
    hipLaunchKernelGGL(k_fo_commit, dim3((n_peers + kFBlock - 1) / kFBlock), dim3(kFBlock), 0, s,
                       (const unsigned long long*)f->tot, n_peers, f->pcnt);
    if (list) hipLaunchKernelGGL(k_fo_write<true>, dim3(n_tiles), dim3(64), lds, s, a);
    else hipLaunchKernelGGL(k_fo_write<false>, dim3(n_tiles), dim3(64), lds, s, a);
    FGI_HIP(g, hipEventRecord(f->ev[3], s));
    // the entries have left the table, whatever the checks below say
    f->free_n += n;
    f->live -= n;
    f->delivered += n;
    *wrote = true;
    FGI_TRY(read_ctr(g));
    if (hipEventElapsedTime(&ms, f->ev[2], f->ev[3]) == hipSuccess) f->last_ms += ms;
    return check_chain(g, what);
}

// the last fan-out's lists into the caller's arrays
fgi_status fan_copy(fgi_graph* g, uint32_t n_peers, uint64_t n, uint64_t* peer_off, uint64_t* call_ids, uint32_t* handles) {
    Fanout* f = g->fan;
    hipStream_t s = g->stream;
    FGI_HIP(g, hipMemcpyAsync(peer_off, f->off, ((size_t)n_peers + 1) * 8, hipMemcpyDeviceToHost, s));
    if (n && call_ids) FGI_HIP(g, hipMemcpyAsync(call_ids, f->out_call, n * 8, hipMemcpyDeviceToHost, s));
    if (n && handles) FGI_HIP(g, hipMemcpyAsync(handles, f->out_hnd, n * 4, hipMemcpyDeviceToHost, s));
    FGI_HIP(g, hipStreamSynchronize(s));
    return FGI_OK;
}

// what every entry point of the section checks first
fgi_status fan_usable(fgi_graph* g, const char* what) {
    if (g->failed) return set_err(g, FGI_ESTATE, "%s: the graph is poisoned; fgi_restore or fgi_destroy", what);
    if (g->part || g->world > 1)
        return set_err(g, FGI_ENOTSUP, "%s: the replica fan-out serves a single device, not a partition", what);
    hipSetDevice(g->device);
    if (g->aw[0].busy || g->aw[1].busy) FGI_TRY(drain_async(g));
    return FGI_OK;
}
// and every fgi_part_* one: a rank's own table, no collective (a partition runs no asynchronous waves, so
// there is nothing to drain). single: the call that serves a graph on one device.
fgi_status part_fan_usable(fgi_graph* g, const char* what, const char* single, PartView* pv) {
    if (!g->part || !part_view(g, pv)) return set_err(g, FGI_ENOTSUP, "%s: not a partitioned graph (%s)", what, single);
    if (g->failed) return set_err(g, FGI_ESTATE, "%s: the graph is poisoned; fgi_restore or fgi_destroy", what);
    hipSetDevice(g->device);
    return FGI_OK;
}

// fgi_subscribe and fgi_part_subscribe behind their checks. pv: the rank's ranges, null on a single device.
fgi_status sub_insert(fgi_graph* g, const char* what, uint32_t n, const uint32_t* handle, const uint32_t* peer,
                      const uint64_t* call_id, uint32_t* out_result, const PartView* pv) {
    FGI_TRY(fan_create(g));
    FGI_TRY(fan_reserve(g, n));
    FGI_TRY(flush_vis(g));   // fgi_restore may have left the visit bitmap's clearing to the next wave
    Fanout* f = g->fan;
    hipStream_t s = g->stream;
    // the upload: handles, peers, results (4 B each), then the call ids
    const uint64_t words32 = 3ull * n + 2ull * n + 2;
    FGI_TRY(grow(g, &f->ids, &f->ids_cap, std::max<uint64_t>(words32, 4096), "the fan-out's subscription upload"));
    uint32_t* dh = f->ids;
    uint32_t* dp = dh + n;
    uint32_t* dr = dp + n;
    unsigned long long* dc = reinterpret_cast<unsigned long long*>(f->ids + ((3ull * n + 1) & ~1ull));
    FGI_HIP(g, hipMemcpyAsync(dh, handle, (size_t)n * 4, hipMemcpyHostToDevice, s));
    FGI_HIP(g, hipMemcpyAsync(dp, peer, (size_t)n * 4, hipMemcpyHostToDevice, s));
    FGI_HIP(g, hipMemcpyAsync(dc, call_id, (size_t)n * 8, hipMemcpyHostToDevice, s));
    FGI_HIP(g, hipMemsetAsync(f->ctr, 0, kCWords * 8, s));
    SubArgs a{};
    a.n = n;
    a.handle = dh;
    a.peer = dp;
    a.call = dc;
    a.result = out_result ? dr : nullptr;
    a.node = reinterpret_cast<const unsigned long long*>(g->node);
    a.vis = g->v_dirty && !g->vis_stale ? g->vis_bm : nullptr;
    a.s2l = g->lbl_hot ? g->s2l : nullptr;
    a.ext_slots = g->ext_slots;
    a.K = g->lbl_K;
    a.head = f->head;
    a.has = f->has;
    a.rec = f->rec;
    a.fstack = f->fstack;
    a.free_n = f->free_n;
    a.bump = f->bump;
    a.cap = f->cap;
    a.pcnt = f->pcnt;
    a.ctr = f->ctr;
    if (pv) {
        a.part = true;
        a.base = pv->base;
        a.n_local = pv->n_local;
        a.gc = g->lbl_perm ? g->pg_gc : nullptr;
    }
    hipLaunchKernelGGL(k_sub_insert, dim3((n + kFBlock - 1) / kFBlock), dim3(kFBlock), 0, s, a);
    if (out_result) FGI_HIP(g, hipMemcpyAsync(out_result, dr, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    FGI_TRY(read_ctr(g));
    const uint64_t stored = std::min<uint64_t>(f->ctr_h[kCStored], n);
    const uint64_t reused = std::min(stored, f->free_n);
    f->free_n -= reused;
    f->bump += stored - reused;
    f->live += stored;
    return check_chain(g, what);
}

// the repeat call of a wave's fan-out: the arrays made before, again
fgi_status fan_again(fgi_graph* g, const char* what, uint32_t n_peers, uint64_t* peer_off, uint64_t* call_ids,
                     uint32_t* handles, uint64_t cap, uint64_t* out_n) {
    const Fanout* f = g->fan;
    if (f->made_peers != n_peers)
        return set_err(g, FGI_EINVAL, "%s: this wave's lists were made for %u peers", what, f->made_peers);
    if (out_n) *out_n = f->made_n;
    if ((call_ids || handles) && f->made_n > cap)
        return set_err(g, FGI_ECAPACITY, "the fan-out holds %llu entries, the buffers %llu", (unsigned long long)f->made_n,
                       (unsigned long long)cap);
    return fan_copy(g, n_peers, f->made_n, peer_off, call_ids, handles);
}

// A host list (checked by the caller: ascending, in range) joined with the table: one upload, then the list
// form, or with FGI_OPT_FANOUT_PATH 2 the list scattered into a bitmap over the map's handles.
fgi_status fan_from_list(fgi_graph* g, const char* what, uint64_t n, const uint32_t* ids, const FoMap& map, uint32_t n_peers,
                         uint64_t* peer_off, uint64_t* call_ids, uint32_t* handles, uint64_t cap, uint64_t* out_n) {
    Fanout* f = g->fan;
    f->made_serial = 0;   // a fan-out: the last wave's lists are gone
    FGI_TRY(grow(g, &f->ids, &f->ids_cap, std::max<uint64_t>(n, 4096), "the fan-out's handle list"));
    FGI_HIP(g, hipMemcpyAsync(f->ids, ids, (size_t)n * 4, hipMemcpyHostToDevice, g->stream));   // the one upload
    const unsigned long long* inv = nullptr;
    const uint32_t* src = f->ids;
    if (g->opt_fanout_path >= 2) {
        FGI_HIP(g, hipMemsetAsync(f->bits, 0, f->words * 8, g->stream));
        hipLaunchKernelGGL(k_fo_scatter, dim3(fgrid(n)), dim3(kFBlock), 0, g->stream, (const uint32_t*)f->ids, n, map.id_base,
                           map.n_handles, f->bits);
        inv = f->bits;
        src = nullptr;
    }
    uint64_t total = 0;
    bool wrote = false;
    FGI_TRY(fan_join(g, inv, src, n, map, n_peers, (call_ids || handles) ? cap : ~0ull, what, &total, &wrote));
    if (out_n) *out_n = total;
    if (total && !wrote)
        return set_err(g, FGI_ECAPACITY, "the fan-out holds %llu entries, the buffers %llu (nothing was removed)",
                       (unsigned long long)total, (unsigned long long)cap);
    return fan_copy(g, n_peers, total, peer_off, call_ids, handles);
}

fgi_status drop_peer(fgi_graph* g, const char* what, uint32_t peer, uint64_t* out_dropped) {
    Fanout* f = g->fan;
    hipStream_t s = g->stream;
    FGI_HIP(g, hipMemsetAsync(f->ctr, 0, kCWords * 8, s));
    hipLaunchKernelGGL(k_fo_drop_peer, dim3(fgrid(g->ext_handles)), dim3(kFBlock), 0, s, edit_args(g), peer);
    FGI_TRY(read_ctr(g));
    if (out_dropped) *out_dropped = std::min<uint64_t>(f->ctr_h[kCDropped], f->live);
    account_dropped(f);
    return check_chain(g, what);
}

}  // namespace

fgi_status fanout_move(fgi_graph* g, uint32_t n, const uint32_t* from, const uint32_t* to) {
    if (!fanout_live(g) || !n) return FGI_OK;
    Fanout* f = g->fan;
    hipStream_t s = g->stream;
    FGI_TRY(grow(g, &f->ids, &f->ids_cap, std::max<uint64_t>(2ull * n, 4096), "the fan-out's handle list"));
    FGI_HIP(g, hipMemcpyAsync(f->ids, from, (size_t)n * 4, hipMemcpyHostToDevice, s));
    FGI_HIP(g, hipMemcpyAsync(f->ids + n, to, (size_t)n * 4, hipMemcpyHostToDevice, s));
    FGI_HIP(g, hipMemsetAsync(f->ctr, 0, kCWords * 8, s));
    hipLaunchKernelGGL(k_fo_move, dim3((n + kFBlock - 1) / kFBlock), dim3(kFBlock), 0, s, edit_args(g), n,
                       (const uint32_t*)f->ids, (const uint32_t*)(f->ids + n));
    FGI_TRY(read_ctr(g));   // the host arrays are the caller's: consumed when this returns
    return check_chain(g, "moving a displaced node's subscriptions");
}

fgi_status fanout_drop_handles(fgi_graph* g, uint32_t n, const uint32_t* handles) {
    if (!fanout_live(g) || !n) return FGI_OK;
    Fanout* f = g->fan;
    hipStream_t s = g->stream;
    FGI_TRY(grow(g, &f->ids, &f->ids_cap, std::max<uint64_t>(n, 4096), "the fan-out's handle list"));
    FGI_HIP(g, hipMemcpyAsync(f->ids, handles, (size_t)n * 4, hipMemcpyHostToDevice, s));
    FGI_HIP(g, hipMemsetAsync(f->ctr, 0, kCWords * 8, s));
    hipLaunchKernelGGL(k_fo_drop_handles, dim3((n + kFBlock - 1) / kFBlock), dim3(kFBlock), 0, s, edit_args(g), n,
                       (const uint32_t*)f->ids);
    FGI_TRY(read_ctr(g));
    account_dropped(f);
    return check_chain(g, "dropping a released handle's subscriptions");
}

void fanout_destroy(fgi_graph* g) {
    Fanout* f = g->fan;
    if (!f) return;
    void* dev[] = {f->head, f->has, f->rec, f->fstack, f->pcnt, f->ctr, f->tcnt, f->tot, f->off, f->out_call, f->out_hnd, f->ids, f->bits};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    if (f->ctr_h) (void)hipHostFree(f->ctr_h);
    for (hipEvent_t e : f->ev)
        if (e) (void)hipEventDestroy(e);
    delete f;
    g->fan = nullptr;
}

}  // namespace fgi

using namespace fgi;

extern "C" {

fgi_status fgi_subscribe(fgi_graph* g, uint32_t n, const uint32_t* handle, const uint32_t* peer, const uint64_t* call_id,
                         uint32_t* out_result) {
    if (!g || (n && (!handle || !peer || !call_id))) return FGI_EINVAL;
    FGI_TRY(fan_usable(g, "fgi_subscribe"));
    for (uint32_t i = 0; i < n; ++i) {
        if (handle[i] >= g->ext_handles) return set_err(g, FGI_EINVAL, "fgi_subscribe: handle %u out of range at %u", handle[i], i);
        if (peer[i] >= FGI_MAX_PEERS) return set_err(g, FGI_EINVAL, "fgi_subscribe: peer %u at %u, at most %u peers", peer[i], i, FGI_MAX_PEERS);
    }
    if (!n) return FGI_OK;
    return sub_insert(g, "fgi_subscribe", n, handle, peer, call_id, out_result, nullptr);
}

fgi_status fgi_last_wave_fanout(fgi_graph* g, uint32_t n_peers, uint64_t* peer_off, uint64_t* call_ids, uint32_t* handles,
                                uint64_t cap, uint64_t* out_n) {
    if (!g || !peer_off) return FGI_EINVAL;
    if (out_n) *out_n = 0;
    FGI_TRY(fan_usable(g, "fgi_last_wave_fanout"));
    if (n_peers == 0 || n_peers > FGI_MAX_PEERS) return set_err(g, FGI_EINVAL, "fgi_last_wave_fanout: n_peers must be 1..%u", FGI_MAX_PEERS);
    if (g->casc_kind == kCascAsync || g->casc_kind == kCascBatch)
        return set_err(g, FGI_ENOTSUP, "fgi_last_wave_fanout: the last cascades ran in %s; pass their ids to fgi_fanout_ids",
                       g->casc_kind == kCascBatch ? "fgi_run_batch" : "an asynchronous wave");
    Fanout* f = g->fan;
    const bool want = call_ids || handles;
    if (f && f->made_serial == g->casc_serial && f->made_serial)   // made already: the same arrays again
        return fan_again(g, "fgi_last_wave_fanout", n_peers, peer_off, call_ids, handles, cap, out_n);
    memset(peer_off, 0, ((size_t)n_peers + 1) * 8);
    if (!fanout_live(g) || g->casc_kind != kCascWave || g->last_wave_n == 0) return FGI_OK;
    // the source: the bitmap the wave kept (boundary order without hot labels), else its id list
    const bool kept = !g->ids_valid && g->lbl_K == 0;
    const int path = g->opt_fanout_path;
    const bool bits = path >= 2 || (path == 0 && kept);   // (3 is a partition's measurement form: 2 here)
    const unsigned long long* inv = nullptr;
    const uint32_t* ids = nullptr;
    if (bits && kept) {
        inv = reinterpret_cast<const unsigned long long*>(g->inv_bm);
    } else {
        FGI_TRY(ensure_ids(g));
        ids = g->inv_cur ? g->inv_cur : g->inv;
        if (bits) {
            FGI_HIP(g, hipMemsetAsync(f->bits, 0, f->words * 8, g->stream));
            hipLaunchKernelGGL(k_fo_scatter, dim3(fgrid(g->last_wave_n)), dim3(kFBlock), 0, g->stream, ids, g->last_wave_n,
                               0u, g->ext_handles, f->bits);
            inv = f->bits;
            ids = nullptr;
        }
    }
    uint64_t total = 0;
    bool wrote = false;
    const fgi_status st = fan_join(g, inv, ids, g->last_wave_n, whole_table(g), n_peers, ~0ull, "fgi_last_wave_fanout", &total, &wrote);
    if (wrote || (st == FGI_OK && total == 0)) {
        f->made_serial = g->casc_serial;
        f->made_peers = n_peers;
        f->made_n = total;
    }
    FGI_TRY(st);
    if (out_n) *out_n = total;
    if (want && total > cap)
        return set_err(g, FGI_ECAPACITY, "the fan-out holds %llu entries, the buffers %llu", (unsigned long long)total,
                       (unsigned long long)cap);
    return fan_copy(g, n_peers, total, peer_off, call_ids, handles);
}

fgi_status fgi_fanout_ids(fgi_graph* g, uint64_t n, const uint32_t* ids, uint32_t n_peers, uint64_t* peer_off, uint64_t* call_ids,
                          uint32_t* handles, uint64_t cap, uint64_t* out_n) {
    if (!g || !peer_off || (n && !ids)) return FGI_EINVAL;
    if (out_n) *out_n = 0;
    FGI_TRY(fan_usable(g, "fgi_fanout_ids"));
    if (n_peers == 0 || n_peers > FGI_MAX_PEERS) return set_err(g, FGI_EINVAL, "fgi_fanout_ids: n_peers must be 1..%u", FGI_MAX_PEERS);
    for (uint64_t i = 0; i < n; ++i)
        if (ids[i] >= g->ext_handles || (i && ids[i] <= ids[i - 1]))
            return set_err(g, FGI_EINVAL, "fgi_fanout_ids: the handles must be in range and strictly ascending (entry %llu)",
                           (unsigned long long)i);
    memset(peer_off, 0, ((size_t)n_peers + 1) * 8);
    if (!fanout_live(g) || n == 0) return FGI_OK;
    return fan_from_list(g, "fgi_fanout_ids", n, ids, whole_table(g), n_peers, peer_off, call_ids, handles, cap, out_n);
}

fgi_status fgi_unsubscribe_peer(fgi_graph* g, uint32_t peer, uint64_t* out_dropped) {
    if (!g) return FGI_EINVAL;
    if (out_dropped) *out_dropped = 0;
    FGI_TRY(fan_usable(g, "fgi_unsubscribe_peer"));
    if (peer >= FGI_MAX_PEERS) return set_err(g, FGI_EINVAL, "fgi_unsubscribe_peer: peer %u, at most %u peers", peer, FGI_MAX_PEERS);
    if (!fanout_live(g)) return FGI_OK;
    return drop_peer(g, "fgi_unsubscribe_peer", peer, out_dropped);
}

// ---- per rank of a partition (C-ABI 0.10): a rank's own table over its own handles, no collective ----

fgi_status fgi_part_subscribe(fgi_graph* g, uint32_t n, const uint32_t* slot, const uint32_t* peer, const uint64_t* call_id,
                              uint32_t* out_result) {
    if (!g || (n && (!slot || !peer || !call_id))) return FGI_EINVAL;
    PartView pv;
    FGI_TRY(part_fan_usable(g, "fgi_part_subscribe", "fgi_subscribe", &pv));
    for (uint32_t i = 0; i < n; ++i) {
        if (slot[i] >= pv.n_global)
            return set_err(g, FGI_EINVAL, "fgi_part_subscribe: entry %u is slot %u of %u", i, slot[i], pv.n_global);
        if (peer[i] >= FGI_MAX_PEERS)
            return set_err(g, FGI_EINVAL, "fgi_part_subscribe: peer %u at %u, at most %u peers", peer[i], i, FGI_MAX_PEERS);
    }
    if (!n) return FGI_OK;
    return sub_insert(g, "fgi_part_subscribe", n, slot, peer, call_id, out_result, &pv);
}

fgi_status fgi_part_last_wave_fanout(fgi_graph* g, uint32_t n_peers, uint64_t* peer_off, uint64_t* call_ids, uint32_t* slots,
                                     uint64_t cap, uint64_t* out_n) {
    if (!g || !peer_off) return FGI_EINVAL;
    if (out_n) *out_n = 0;
    PartView pv;
    FGI_TRY(part_fan_usable(g, "fgi_part_last_wave_fanout", "fgi_last_wave_fanout", &pv));
    if (n_peers == 0 || n_peers > FGI_MAX_PEERS)
        return set_err(g, FGI_EINVAL, "fgi_part_last_wave_fanout: n_peers must be 1..%u", FGI_MAX_PEERS);
    if (g->pout_kind == kPoutOther)
        return set_err(g, FGI_ENOTSUP, "fgi_part_last_wave_fanout: this rank's last call that ran cascades was no single wave; "
                                       "pass the ids it returned to fgi_part_fanout_ids");
    Fanout* f = g->fan;
    if (f && f->made_serial == g->pout_serial && f->made_serial)   // made already: the same arrays again
        return fan_again(g, "fgi_part_last_wave_fanout", n_peers, peer_off, call_ids, slots, cap, out_n);
    memset(peer_off, 0, ((size_t)n_peers + 1) * 8);
    if (!fanout_live(g) || g->pout_kind != kPoutWave || g->last_wave_n == 0) return FGI_OK;
    // The source. List: the rank's ascending global ids (part_out.hip). Bitmap: the host-order one if it
    // stands; else, with codes, inv & has probed from the subscribed handles; else the wave's own bitmap,
    // which is in handle order already (the map keeps what lies past the owned slots out of the join).
    const int path = g->opt_fanout_path;
    const bool list = path == 1 || (path == 0 && g->pout && g->pout->ids_valid);
    const unsigned long long* inv = nullptr;
    const uint32_t* ids = nullptr;
    f->last_ms = 0;   // (a call that fails before the join's kernels leaves no earlier call's time behind)
    FGI_HIP(g, hipEventRecord(f->ev[4], g->stream));   // what makes the source counts in last_kernel_ms
    if (list) {
        FGI_TRY(part_out_ids(g, &ids, nullptr));
    } else if (g->pout && g->pout->bits_valid) {
        inv = g->pout->bits;
    } else if (path == 3) {   // measurement only: the whole bitmap renumbered first (part_out_bits), then the AND
        uint64_t w = 0;
        FGI_TRY(part_out_bits(g, &inv, &w));
    } else if (g->lbl_perm) {
        hipLaunchKernelGGL(k_fo_probe, dim3(fgrid(f->words * 64)), dim3(kFBlock), 0, g->stream,
                           reinterpret_cast<const unsigned long long*>(g->inv_bm), (const unsigned long long*)f->has,
                           (const uint32_t*)g->pg_gc, pv.base, pv.n_local, f->bits, f->words);
        FGI_HIP(g, hipGetLastError());
        inv = f->bits;
    } else {
        inv = reinterpret_cast<const unsigned long long*>(g->inv_bm);
    }
    FGI_HIP(g, hipEventRecord(f->ev[5], g->stream));
    uint64_t total = 0;
    bool wrote = false;
    const fgi_status st = fan_join(g, inv, ids, g->last_wave_n, owned_slots(pv), n_peers, ~0ull, "fgi_part_last_wave_fanout",
                                   &total, &wrote);
    float src_ms = 0;   // (fan_join waited for the stream)
    if (hipEventElapsedTime(&src_ms, f->ev[4], f->ev[5]) == hipSuccess) f->last_ms += src_ms;
    if (wrote || (st == FGI_OK && total == 0)) {
        f->made_serial = g->pout_serial;
        f->made_peers = n_peers;
        f->made_n = total;
    }
    FGI_TRY(st);
    if (out_n) *out_n = total;
    if ((call_ids || slots) && total > cap)
        return set_err(g, FGI_ECAPACITY, "the fan-out holds %llu entries, the buffers %llu", (unsigned long long)total,
                       (unsigned long long)cap);
    return fan_copy(g, n_peers, total, peer_off, call_ids, slots);
}

fgi_status fgi_part_fanout_ids(fgi_graph* g, uint64_t n, const uint32_t* slots_in, uint32_t n_peers, uint64_t* peer_off,
                               uint64_t* call_ids, uint32_t* slots, uint64_t cap, uint64_t* out_n) {
    if (!g || !peer_off || (n && !slots_in)) return FGI_EINVAL;
    if (out_n) *out_n = 0;
    PartView pv;
    FGI_TRY(part_fan_usable(g, "fgi_part_fanout_ids", "fgi_fanout_ids", &pv));
    if (n_peers == 0 || n_peers > FGI_MAX_PEERS) return set_err(g, FGI_EINVAL, "fgi_part_fanout_ids: n_peers must be 1..%u", FGI_MAX_PEERS);
    for (uint64_t i = 0; i < n; ++i)
        if (slots_in[i] >= pv.n_global || (i && slots_in[i] <= slots_in[i - 1]))
            return set_err(g, FGI_EINVAL, "fgi_part_fanout_ids: the slots must be below %u and strictly ascending (entry %llu)",
                           pv.n_global, (unsigned long long)i);
    memset(peer_off, 0, ((size_t)n_peers + 1) * 8);
    if (!fanout_live(g) || n == 0) return FGI_OK;
    // (the slots of other ranks are skipped in the kernels: one compare each)
    return fan_from_list(g, "fgi_part_fanout_ids", n, slots_in, owned_slots(pv), n_peers, peer_off, call_ids, slots, cap, out_n);
}

fgi_status fgi_part_fanout_detached(fgi_graph* g, uint64_t n, const uint32_t* handles, uint32_t n_peers, uint64_t* peer_off,
                                    uint64_t* call_ids, uint32_t* handles_out, uint64_t cap, uint64_t* out_n) {
    if (!g || !peer_off || (n && !handles)) return FGI_EINVAL;
    if (out_n) *out_n = 0;
    PartView pv;
    FGI_TRY(part_fan_usable(g, "fgi_part_fanout_detached", "fgi_fanout_ids", &pv));
    if (n_peers == 0 || n_peers > FGI_MAX_PEERS)
        return set_err(g, FGI_EINVAL, "fgi_part_fanout_detached: n_peers must be 1..%u", FGI_MAX_PEERS);
    for (uint64_t i = 0; i < n; ++i)
        if (handles[i] < g->ext_slots || handles[i] >= g->ext_handles || (i && handles[i] <= handles[i - 1]))
            return set_err(g, FGI_EINVAL, "fgi_part_fanout_detached: the handles must be this rank's detached ones, %u..%u, "
                                          "and strictly ascending (entry %llu)", g->ext_slots, g->ext_handles - 1,
                           (unsigned long long)i);
    memset(peer_off, 0, ((size_t)n_peers + 1) * 8);
    if (!fanout_live(g) || n == 0) return FGI_OK;
    return fan_from_list(g, "fgi_part_fanout_detached", n, handles, whole_table(g), n_peers, peer_off, call_ids, handles_out, cap,
                         out_n);
}

fgi_status fgi_part_unsubscribe_peer(fgi_graph* g, uint32_t peer, uint64_t* out_dropped) {
    if (!g) return FGI_EINVAL;
    if (out_dropped) *out_dropped = 0;
    PartView pv;
    FGI_TRY(part_fan_usable(g, "fgi_part_unsubscribe_peer", "fgi_unsubscribe_peer", &pv));
    if (peer >= FGI_MAX_PEERS)
        return set_err(g, FGI_EINVAL, "fgi_part_unsubscribe_peer: peer %u, at most %u peers", peer, FGI_MAX_PEERS);
    if (!fanout_live(g)) return FGI_OK;
    return drop_peer(g, "fgi_part_unsubscribe_peer", peer, out_dropped);
}

fgi_status fgi_sub_stats_get(fgi_graph* g, fgi_sub_stats* out) {
    if (!g || !out) return FGI_EINVAL;
    memset(out, 0, sizeof(*out));
    const Fanout* f = g->fan;
    if (!f) return FGI_OK;
    out->live = f->live;
    out->pool = f->cap;
    out->delivered = f->delivered;
    out->dropped = f->dropped;
    out->fanouts = f->fanouts;
    out->from_list = f->from_list;
    out->from_bits = f->from_bits;
    out->last_kernel_ms = f->last_ms;
    return FGI_OK;
}

}  // extern "C"
