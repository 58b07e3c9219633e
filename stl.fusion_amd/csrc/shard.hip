// shard.hip — a partition loaded from per-rank shards (fgi_part_register_shard, fgi_part_load_edges_shard;
// DESIGN.md §5). Every rank hands in whatever nodes and edges it holds, whoever owns them; the engine routes
// them to their owners over the partition's own transport (PartComm's allgatherv / alltoallv, part.hip) and
// leaves every rank in the state the replicated calls (fgi_part_register_nodes / fgi_part_load_edges) would
// have left, had every rank been given the concatenation of the shards in rank order.
//
// Registration: 16-byte records {slot, state_flags, version} all-gathered, then k_shard_register over the
// whole list on every rank (the owner installs the node, every rank writes its version replica).
// Edges: each edge yields a row record for the owner of its `used` end and an in record for the owner of its
// dependant. k_shard_count validates the shard and counts the records per destination, k_shard_scatter writes
// them as one (keys, tags) pair of runs per destination, two exchanges move the rows' and the ins' records,
// and the receiver finishes as fgi_part_load_edges does, from device arrays throughout.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "fgi_internal.h"

namespace fgi {
namespace {

constexpr uint32_t kShardThreads = 256;
constexpr uint32_t kShardPer = 2048;    // fewest edges per block: the 16 counter words see few atomics
constexpr uint32_t kShardGrid = 2048;   // most blocks (a block then walks more edges)
constexpr uint32_t kBins = 16;          // bin q: row records for rank q; bin 8 + q: in records for rank q
constexpr uint32_t kNoBin = 0xFFu;

struct ShardBases {
    unsigned long long b[kBins];        // first record of each bin in the send buffers
};

inline uint32_t nblk(uint64_t n) { return (uint32_t)((n + 255) / 256); }

// blocks of a shard of m edges and the contiguous edges each walks (a multiple of the block size)
inline void shard_geometry(uint64_t m, uint32_t* grid, uint64_t* per) {
    const uint64_t g = std::min<uint64_t>(std::max<uint64_t>((m + kShardPer - 1) / kShardPer, 1), kShardGrid);
    const uint64_t p = (m + g - 1) / g;
    *grid = (uint32_t)g;
    *per = std::max<uint64_t>((p + kShardThreads - 1) / kShardThreads * kShardThreads, kShardThreads);
}

// Per block: the records of its edges per bin into blk_cnt[block][kBins] and, one atomic per non-empty bin,
// into cnt[kBins]. An edge out of range or with tag 0 belongs to no bin; the first one's index goes to *bad.
// Per wave and bin one ballot and a popcount (wave-uniform counters), then LDS, then the global words.
__global__ __launch_bounds__(kShardThreads) void k_shard_count(uint64_t m, uint64_t per, const uint32_t* __restrict__ used,
                                                               const uint32_t* __restrict__ dep,
                                                               const uint64_t* __restrict__ tag, uint32_t N, uint32_t B,
                                                               uint32_t W, uint32_t* blk_cnt, unsigned long long* cnt,
                                                               unsigned long long* bad) {
    __shared__ uint32_t s_cnt[kBins];
    if (threadIdx.x < kBins) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per < m ? lo + per : m;
    uint32_t c[kBins];
#pragma unroll
    for (uint32_t q = 0; q < kBins; ++q) c[q] = 0;
    for (uint64_t i0 = lo; i0 < hi; i0 += kShardThreads) {   // block-uniform
        const uint64_t i = i0 + threadIdx.x;
        uint32_t qr = kNoBin, qi = kNoBin;
        if (i < hi) {
            const uint32_t u = used[i], d = dep[i];
            if (u < N && d < N && tag[i] != 0) {
                qr = u / B;
                qi = d / B;
            } else {
                atomicMin(bad, (unsigned long long)i);
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) {
            if (q < W) {
                c[q] += (uint32_t)__popcll(__ballot(qr == q));
                c[8 + q] += (uint32_t)__popcll(__ballot(qi == q));
            }
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (uint32_t q = 0; q < kBins; ++q)
            if (c[q]) atomicAdd(&s_cnt[q], c[q]);
    }
    __syncthreads();
    if (threadIdx.x < kBins) {
        const uint32_t v = s_cnt[threadIdx.x];
        blk_cnt[(size_t)blockIdx.x * kBins + threadIdx.x] = v;
        if (v) atomicAdd(cnt + threadIdx.x, (unsigned long long)v);
    }
}

// The same walk (same grid, same `per`): each block reserves its run of every non-empty bin with one atomic
// (its counts are k_shard_count's), its waves take their places from LDS cursors, one ballot per bin, and
// the lanes rank themselves inside the ballot mask. Keys and tags go out as two streams; within a bin the
// order is free (the receiver sorts and deduplicates). Row key: (used - owner's base) << 32 | dependant;
// in key: (dependant - owner's base) << 32 | used; both in the host's slot numbers.
__global__ __launch_bounds__(kShardThreads) void k_shard_scatter(uint64_t m, uint64_t per, const uint32_t* __restrict__ used,
                                                                 const uint32_t* __restrict__ dep,
                                                                 const uint64_t* __restrict__ tag, uint32_t N, uint32_t B,
                                                                 uint32_t W, const uint32_t* __restrict__ blk_cnt,
                                                                 ShardBases bases, unsigned long long* cursor,
                                                                 uint64_t* keys, uint64_t* tags) {
    __shared__ unsigned long long s_cur[kBins];
    if (threadIdx.x < kBins) {
        const uint32_t v = blk_cnt[(size_t)blockIdx.x * kBins + threadIdx.x];
        s_cur[threadIdx.x] = bases.b[threadIdx.x] + (v ? atomicAdd(cursor + threadIdx.x, (unsigned long long)v) : 0ull);
    }
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per < m ? lo + per : m;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t i0 = lo; i0 < hi; i0 += kShardThreads) {   // block-uniform
        const uint64_t i = i0 + threadIdx.x;
        uint32_t qr = kNoBin, qi = kNoBin, u = 0, d = 0;
        uint64_t t = 0;
        if (i < hi) {
            u = used[i];
            d = dep[i];
            t = tag[i];
            if (u < N && d < N && t != 0) {
                qr = u / B;
                qi = d / B;
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) {
            if (q >= W) continue;
            const unsigned long long mr = __ballot(qr == q), mi = __ballot(qi == q);
            unsigned long long br = 0, bi = 0;
            if (lane == 0) {
                if (mr) br = atomicAdd(&s_cur[q], (unsigned long long)__popcll(mr));
                if (mi) bi = atomicAdd(&s_cur[8 + q], (unsigned long long)__popcll(mi));
            }
            br = __shfl(br, 0, 64);
            bi = __shfl(bi, 0, 64);
            if (qr == q) {
                const uint64_t at = br + __builtin_amdgcn_mbcnt_hi((uint32_t)(mr >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mr, 0u));
                keys[at] = ((uint64_t)(u - q * B) << 32) | d;
                tags[at] = t;
            }
            if (qi == q) {
                const uint64_t at = bi + __builtin_amdgcn_mbcnt_hi((uint32_t)(mi >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mi, 0u));
                keys[at] = ((uint64_t)(d - q * B) << 32) | u;
                tags[at] = t;
            }
        }
    }
}

// received keys (owned slot - base) << 32 | global slot, both halves to partition codes
__global__ void k_shard_codes(uint64_t n, uint64_t* keys, const uint32_t* __restrict__ gc, uint32_t base) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = keys[i];
        keys[i] = ((uint64_t)(gc[(uint32_t)(k >> 32) + base] - base) << 32) | gc[(uint32_t)k];
    }
}

// the received in records of this rank's own dependants that are live when loaded (k_part_weight's rule)
__global__ void k_shard_weight(uint64_t n, const uint64_t* __restrict__ keys, const uint64_t* __restrict__ tags,
                               const uint64_t* __restrict__ ver_all, uint32_t base, uint32_t* inc) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t d = (uint32_t)(keys[i] >> 32);
        if (tags[i] == ver_all[base + d]) atomicAdd(inc + d, 1u);
    }
}

// every rank's increments (rank q's block at q * block) added to the weights; world * block may exceed n
__global__ void k_shard_weight_add(uint32_t n, const uint32_t* __restrict__ inc_all, uint32_t* weight) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && inc_all[i]) weight[i] += inc_all[i];
}

// k_part_register's body over the gathered records {slot, state_flags, version lo, version hi}: every rank
// writes the replica, the owner installs the node. A slot with a current node counts into *err, a slot listed
// twice included: the compare-and-swap lets one record win and the other one see its node.
__global__ void k_shard_register(uint64_t n, const uint4* __restrict__ rec, const uint32_t* __restrict__ gc, uint32_t base,
                                 uint32_t n_local, uint64_t* ver_all, unsigned long long* node, uint32_t* row_len,
                                 unsigned long long* err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 r = rec[i];
    const uint32_t s = gc ? gc[r.x] : r.x;
    const uint64_t v = (uint64_t)r.z | ((uint64_t)r.w << 32);
    ver_all[s] = v;
    const uint32_t h = s - base;
    if (h >= n_local) return;
    const unsigned long long w = v ? flags_to_word(v, r.y) : 0ull;
    unsigned long long old = node[h];
    while (true) {
        if (word_is_current(old)) {
            atomicAdd(err, 1ull);
            return;
        }
        const unsigned long long seen = atomicCAS(node + h, old, w);
        if (seen == old) break;
        old = seen;
    }
    row_len[h] = 0;
}

fgi_status shard_enter(fgi_graph* g, const char* what) {
    if (!g->part) return set_err(g, FGI_ESTATE, "%s: partition not initialised", what);
    if (g->failed)
        return set_err(g, FGI_ESTATE, "%s: a batch or wave failed on the device; fgi_restore or fgi_destroy", what);
    hipSetDevice(g->device);
    return FGI_OK;
}

fgi_status map_codes(fgi_graph* g, uint64_t n, uint64_t* keys, uint32_t base) {
    if (!n) return FGI_OK;
    hipLaunchKernelGGL(k_shard_codes, dim3(std::min<uint32_t>(nblk(n), 8192)), dim3(256), 0, g->stream, n, keys,
                       (const uint32_t*)g->pg_gc, base);
    FGI_HIP(g, hipGetLastError());
    return FGI_OK;
}

}  // namespace
}  // namespace fgi

using namespace fgi;

extern "C" {

fgi_status fgi_part_register_shard(fgi_graph* g, uint32_t n, const uint32_t* slot, const uint64_t* version,
                                   const uint32_t* state_flags) {
    if (!g) return FGI_EINVAL;
    FGI_TRY(shard_enter(g, "fgi_part_register_shard"));
    PartView pv;
    part_view(g, &pv);
    const uint32_t W = pv.world;
    // This rank's verdict on its own shard travels with the counts, so a bad shard fails the call on every
    // rank at the same point: {n, first bad item + 1, what is wrong with it, the shard opens the flag gate}
    uint64_t mine[4] = {n, 0, 0, 0}, all[8 * 4];
    if (n && (!slot || !version)) {
        mine[1] = 1;
        mine[2] = 4;
    }
    for (uint32_t i = 0; i < n && !mine[1]; ++i) {
        const uint32_t what = slot[i] >= pv.n_global ? 1u : version[i] > kVMask ? 2u : (state_flags && (state_flags[i] & 3u) == 3u) ? 3u : 0u;
        if (what) {
            mine[1] = (uint64_t)i + 1;
            mine[2] = what;
        }
    }
    // a Computing node, or one with an invalidation delay, can be flagged by a visit (flagged sets): any
    // listed node counts, in any shard, so every rank decides alike
    for (uint32_t i = 0; i < n && state_flags && !mine[1] && !mine[3]; ++i)
        if (version[i] && ((state_flags[i] & FGI_STATE_MASK) == FGI_COMPUTING || (state_flags[i] & FGI_F_HAS_DELAY))) mine[3] = 1;
    FGI_TRY(part_allgather_words(g, mine, 4, all));
    uint64_t total = 0, bytes[8];
    bool gate = false;
    for (uint32_t q = 0; q < W; ++q) {
        const uint64_t* a = all + 4 * q;
        if (a[1]) {
            static const char* const kWhat[] = {"", "slot out of range", "version exceeds 2^56-1", "bad state", "null array"};
            return set_err(g, FGI_EINVAL, "fgi_part_register_shard: rank %u's shard, node %llu: %s (nothing applied)", q,
                           (unsigned long long)(a[1] - 1), kWhat[a[2] <= 4 ? a[2] : 0]);
        }
        total += a[0];
        bytes[q] = a[0] * 16;
        gate = gate || a[3];
    }
    if (gate) g->flag_gate = true;
    if (total == 0) return FGI_OK;
    hipStream_t s = g->stream;
    FGI_TRY(fold(g));
    Tmp tmine, tall, terr;
    uint4 *rec_mine, *rec_all;
    unsigned long long* err;
    FGI_TRY(tmalloc(g, tmine, &rec_mine, n));
    FGI_TRY(tmalloc(g, tall, &rec_all, total));
    FGI_TRY(tmalloc(g, terr, &err, 1));
    std::vector<uint4> rec(n);
    for (uint32_t i = 0; i < n; ++i)
        rec[i] = make_uint4(slot[i], state_flags ? state_flags[i] : (uint32_t)FGI_CONSISTENT, (uint32_t)version[i],
                       (uint32_t)(version[i] >> 32));
    if (n) FGI_HIP(g, hipMemcpyAsync(rec_mine, rec.data(), (size_t)n * 16, hipMemcpyHostToDevice, s));
    FGI_HIP(g, hipMemsetAsync(err, 0, 8, s));
    FGI_TRY(part_allgatherv(g, rec_mine, bytes, rec_all));
    hipLaunchKernelGGL(k_shard_register, dim3(nblk(total)), dim3(256), 0, s, total, (const uint4*)rec_all,
                       g->lbl_perm ? (const uint32_t*)g->pg_gc : (const uint32_t*)nullptr, pv.base, pv.n_local, pv.ver_all,
                       reinterpret_cast<unsigned long long*>(g->node), g->row_len, err);
    FGI_HIP(g, hipGetLastError());
    touch(g);          // versions changed: the pull lists are rebuilt before the next wave
    note_words(g);
    uint64_t bad = 0;
    FGI_TRY(part_allreduce_sum(g, err, &bad, 1));   // the owners' counts: every rank fails alike
    if (bad)
        return set_err(g, FGI_ESTATE, "fgi_part_register_shard: %llu listed slots already had a current node "
                                      "(or are listed twice)", (unsigned long long)bad);
    return view_rebuild(g);   // a bulk import: the state view's full build
}

fgi_status fgi_part_load_edges_shard(fgi_graph* g, uint64_t m, const uint32_t* used, const uint32_t* dependant,
                                     const uint64_t* tag) {
    if (!g) return FGI_EINVAL;
    FGI_TRY(shard_enter(g, "fgi_part_load_edges_shard"));
    PartView pv;
    part_view(g, &pv);
    const uint32_t W = pv.world, R = pv.rank, N = pv.n_global, B = pv.block, base = pv.base;
    hipStream_t s = g->stream;
    const bool null_arg = m && (!used || !dependant || !tag);
    Tmp tdu, tdd, tdt, tctr, tblk, tsk, tst, trk, trt, tik, tit;
    uint32_t *du = nullptr, *dd = nullptr, *blk_cnt = nullptr;
    uint64_t* dt = nullptr;
    unsigned long long* ctr = nullptr;   // [kBins] counts, [kBins] scatter cursors, the first bad edge
    uint32_t grid = 1;
    uint64_t per = kShardThreads;
    shard_geometry(m, &grid, &per);
    // {records per bin, first bad edge + 1, what is wrong with it}: this rank's verdict travels with the counts
    uint64_t mine[kBins + 2], all[8 * (kBins + 2)];
    std::memset(mine, 0, sizeof(mine));
    if (null_arg) {
        mine[kBins] = 1;
        mine[kBins + 1] = 3;
    } else if (m) {
        FGI_TRY(tmalloc(g, tdu, &du, m));
        FGI_TRY(tmalloc(g, tdd, &dd, m));
        FGI_TRY(tmalloc(g, tdt, &dt, m));
        FGI_TRY(tmalloc(g, tctr, &ctr, 2 * kBins + 1));
        FGI_TRY(tmalloc(g, tblk, &blk_cnt, (uint64_t)grid * kBins));
        FGI_HIP(g, hipMemcpyAsync(du, used, m * 4, hipMemcpyHostToDevice, s));
        FGI_HIP(g, hipMemcpyAsync(dd, dependant, m * 4, hipMemcpyHostToDevice, s));
        FGI_HIP(g, hipMemcpyAsync(dt, tag, m * 8, hipMemcpyHostToDevice, s));
        FGI_HIP(g, hipMemsetAsync(ctr, 0, 2 * kBins * 8, s));
        FGI_HIP(g, hipMemsetAsync(ctr + 2 * kBins, 0xFF, 8, s));
        hipLaunchKernelGGL(k_shard_count, dim3(grid), dim3(kShardThreads), 0, s, m, per, (const uint32_t*)du,
                           (const uint32_t*)dd, (const uint64_t*)dt, N, B, W, blk_cnt, ctr, ctr + 2 * kBins);
        FGI_HIP(g, hipGetLastError());
        unsigned long long h[2 * kBins + 1];
        FGI_HIP(g, hipMemcpyAsync(h, ctr, sizeof(h), hipMemcpyDeviceToHost, s));
        FGI_HIP(g, hipStreamSynchronize(s));
        for (uint32_t q = 0; q < kBins; ++q) mine[q] = h[q];
        if (h[2 * kBins] != ~0ull) {
            const uint64_t e = h[2 * kBins];
            mine[kBins] = e + 1;
            mine[kBins + 1] = tag[e] == 0 && used[e] < N && dependant[e] < N ? 2 : 1;
        }
    }
    FGI_TRY(part_allgather_words(g, mine, kBins + 2, all));
    uint64_t total_m = 0;
    for (uint32_t q = 0; q < W; ++q) {
        const uint64_t* a = all + (size_t)(kBins + 2) * q;
        if (a[kBins]) {
            static const char* const kWhat[] = {"", "out of range", "has tag 0 (LTags are positive)", "null array"};
            return set_err(g, FGI_EINVAL, "fgi_part_load_edges_shard: rank %u's shard, edge %llu %s (nothing applied)", q,
                           (unsigned long long)(a[kBins] - 1), kWhat[a[kBins + 1] <= 3 ? a[kBins + 1] : 0]);
        }
        for (uint32_t r = 0; r < 8; ++r) total_m += a[r];
    }
    // the records this rank sends (bins in order: rows for rank 0.., ins for rank 0..) and receives
    ShardBases bases;
    uint64_t soff_r[8], sb_r[8], soff_i[8], sb_i[8], roff_r[8], rb_r[8], roff_i[8], rb_i[8];
    uint64_t at = 0, n_row = 0, n_in = 0;
    for (uint32_t b = 0; b < kBins; ++b) {
        bases.b[b] = at;
        at += mine[b];
    }
    for (uint32_t q = 0; q < W; ++q) {
        const uint64_t* a = all + (size_t)(kBins + 2) * q;
        soff_r[q] = bases.b[q] * 8;
        sb_r[q] = mine[q] * 8;
        soff_i[q] = bases.b[8 + q] * 8;
        sb_i[q] = mine[8 + q] * 8;
        roff_r[q] = n_row * 8;
        rb_r[q] = a[R] * 8;
        roff_i[q] = n_in * 8;
        rb_i[q] = a[8 + R] * 8;
        n_row += a[R];
        n_in += a[8 + R];
    }
    // staging: 32 bytes per edge of the shard, 16 per record received
    uint64_t *sk, *st, *rk, *rt, *ik, *it;
    FGI_TRY(tmalloc(g, tsk, &sk, at));
    FGI_TRY(tmalloc(g, tst, &st, at));
    FGI_TRY(tmalloc(g, trk, &rk, n_row));
    FGI_TRY(tmalloc(g, trt, &rt, n_row));
    FGI_TRY(tmalloc(g, tik, &ik, n_in));
    FGI_TRY(tmalloc(g, tit, &it, n_in));
    if (m) {
        hipLaunchKernelGGL(k_shard_scatter, dim3(grid), dim3(kShardThreads), 0, s, m, per, (const uint32_t*)du,
                           (const uint32_t*)dd, (const uint64_t*)dt, N, B, W, (const uint32_t*)blk_cnt, bases, ctr + kBins, sk,
                           st);
        FGI_HIP(g, hipGetLastError());
    }
    if (total_m) {
        FGI_TRY(part_alltoallv(g, sk, soff_r, sb_r, rk, roff_r, rb_r));
        FGI_TRY(part_alltoallv(g, st, soff_r, sb_r, rt, roff_r, rb_r));
        FGI_TRY(part_alltoallv(g, sk, soff_i, sb_i, ik, roff_i, rb_i));
        FGI_TRY(part_alltoallv(g, st, soff_i, sb_i, it, roff_i, rb_i));
    }
    // the shard and what it sent are done with (every exchange returned with its data in place; a rank whose
    // scatter alone is queued reuses these on the same stream)
    for (Tmp* t : {&tdu, &tdd, &tdt, &tsk, &tst, &tblk, &tctr}) t->reset();
    // The receiver: what fgi_part_load_edges does with the whole batch, from the records of its own slots.
    // With codes already chosen the keys take them first (the replica and the weights are in code order).
    if (g->lbl_perm) {
        FGI_TRY(map_codes(g, n_row, rk, base));
        FGI_TRY(map_codes(g, n_in, ik, base));
    }
    if (total_m) {
        // list weights: every rank counts its own dependants' live entries, the blocks are all-gathered
        Tmp tinc, tinc_all;
        uint32_t *inc, *inc_all;
        FGI_TRY(tmalloc(g, tinc, &inc, B));
        FGI_TRY(tmalloc(g, tinc_all, &inc_all, (uint64_t)W * B));
        FGI_HIP(g, hipMemsetAsync(inc, 0, (size_t)B * 4, s));
        if (n_in)
            hipLaunchKernelGGL(k_shard_weight, dim3(std::min<uint32_t>(nblk(n_in), 8192)), dim3(256), 0, s, n_in,
                               (const uint64_t*)ik, (const uint64_t*)it, (const uint64_t*)pv.ver_all, base, inc);
        FGI_HIP(g, hipGetLastError());
        uint64_t wb[8];
        for (uint32_t q = 0; q < W; ++q) wb[q] = (uint64_t)B * 4;
        FGI_TRY(part_allgatherv(g, inc, wb, inc_all));
        hipLaunchKernelGGL(k_shard_weight_add, dim3(nblk(N)), dim3(256), 0, s, N, (const uint32_t*)inc_all, part_weight(g));
        FGI_HIP(g, hipGetLastError());
        FGI_HIP(g, hipStreamSynchronize(s));
        tinc.reset();
        tinc_all.reset();
        // the first bulk load of a partition that wants codes: every rank holds the same global weights
        if (part_codes_now(g)) {
            FGI_TRY(part_codes_choose(g, part_weight(g)));
            FGI_TRY(view_rebuild(g));   // the installed words moved: the state view's full build through the new map
            FGI_TRY(map_codes(g, n_row, rk, base));
            FGI_TRY(map_codes(g, n_in, ik, base));
        }
    }
    FGI_TRY(load_rows_dev(g, n_row, rk, rt, base, base));
    FGI_TRY(part_store_in_dev(g, ik, it, n_in));
    return part_rebuild_lists(g);
}

fgi_status fgi_part_local_register_shards(fgi_graph* const* gs, uint32_t p, const uint32_t* n, const uint32_t* const* slot,
                                          const uint64_t* const* version, const uint32_t* const* state_flags) {
    if (!gs || p == 0 || !n || !slot || !version) return FGI_EINVAL;
    return part_local_run(gs, p, [&](uint32_t r) {
        return fgi_part_register_shard(gs[r], n[r], slot[r], version[r], state_flags ? state_flags[r] : nullptr);
    });
}

fgi_status fgi_part_local_load_shards(fgi_graph* const* gs, uint32_t p, const uint64_t* m, const uint32_t* const* used,
                                      const uint32_t* const* dependant, const uint64_t* const* tag) {
    if (!gs || p == 0 || !m || !used || !dependant || !tag) return FGI_EINVAL;
    return part_local_run(gs, p, [&](uint32_t r) {
        return fgi_part_load_edges_shard(gs[r], m[r], used[r], dependant[r], tag[r]);
    });
}

}  // extern "C"
