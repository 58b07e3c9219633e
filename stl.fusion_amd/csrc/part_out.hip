// part_out.hip — a partition rank's last wave in the host's numbering, made on the device (C-ABI 0.8;
// DESIGN.md §5): fgi_part_last_wave_bits, fgi_part_last_wave_ids, fgi_part_wave_ids_dev, and the staging of
// fgi_part_invalidate_host's roots.
//
// A partitioned wave leaves two things on the rank's device until the rank's next wave starts (both
// drivers, run_part_wave and run_part_planned, end with a final collect that only reads the invalidated
// bitmap, and nothing but the next wave's init kernel clears it): inv_bm, the invalidated bitmap over the
// rank's engine indices, and g->inv, the same set as a list in engine order. With partition codes the
// engine's index of owned slot base + h is gc[base + h] - base, so neither is in the host's numbering.
//   k_pout_mask     no codes: the bitmap is inv_bm masked to the owned slots
//   k_pout_gather   codes, a dense wave: a wavefront per output word, lane l probes the bit of handle
//                   64 x + l's engine index, one ballot is the word, stored whole by lane 0
//   k_pout_scatter  codes, a sparse wave: one thread per entry of the wave's list, an atomic OR at the
//                   entry's handle (the bitmap zeroed first)
//   k_pout_count / k_pout_scan / k_pout_write   the ascending global ids from that bitmap: per-block
//                   popcounts, their exclusive scan, then every block writes base + bit index for its
//                   words at its offset. An id's place follows from its position in the bitmap alone.
// Everything is made on demand, at most once per wave, in buffers allocated at first use: a partition that
// never asks launches and allocates nothing here.
#include "fgi_internal.h"

#include <algorithm>
#include <cstring>

namespace fgi {
namespace {

constexpr int kOBlock = 256;   // threads per block; k_pout_count / k_pout_write: one bitmap word per thread

__global__ __launch_bounds__(kOBlock) void k_pout_mask(const unsigned long long* __restrict__ inv64, uint32_t n_local,
                                                       unsigned long long* out, uint64_t words) {
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < words; x += nthr) {
        const uint64_t h0 = x * 64;
        unsigned long long w = 0ull;
        if (h0 < n_local) {
            w = inv64[x];
            if (n_local - h0 < 64) w &= (1ull << (n_local - h0)) - 1;
        }
        out[x] = w;
    }
}

// gc: slot -> code over all global slots; a code stays in its owner's range, so gc[base + h] - base < n_local
// (checked: a table that says otherwise sets no bit and the count check of the ids reports it)
__global__ __launch_bounds__(kOBlock) void k_pout_gather(const unsigned long long* __restrict__ inv64,
                                                         const uint32_t* __restrict__ gc, uint32_t base, uint32_t n_local,
                                                         unsigned long long* out, uint64_t words) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t x = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; x < words; x += nwaves) {   // wave-uniform
        const uint64_t h = x * 64 + lane;
        bool hit = false;
        if (h < n_local) {
            const uint32_t e = gc[base + (uint32_t)h] - base;
            hit = e < n_local && ((inv64[e >> 6] >> (e & 63)) & 1ull);
        }
        const unsigned long long w = __ballot(hit);
        if (lane == 0) out[x] = w;   // the wavefront owns word x: a plain store of the whole word
    }
}

// inv: the wave's list (engine indices of the owned slots), n entries; ig: code -> slot
__global__ __launch_bounds__(kOBlock) void k_pout_scatter(const uint32_t* __restrict__ inv, uint64_t n,
                                                          const uint32_t* __restrict__ ig, uint32_t base, uint32_t n_local,
                                                          unsigned long long* out) {
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthr) {
        const uint32_t e = inv[i];
        if (e >= n_local) continue;
        const uint32_t h = ig[base + e] - base;
        if (h < n_local) atomicOr(out + (h >> 6), 1ull << (h & 63));
    }
}

// bsum[b] = set bits of words [b * kOBlock, (b + 1) * kOBlock)
__global__ __launch_bounds__(kOBlock) void k_pout_count(const unsigned long long* __restrict__ bm, uint64_t words,
                                                        unsigned long long* bsum) {
    __shared__ uint32_t s_c[kOBlock / 64];
    const uint64_t x = (uint64_t)blockIdx.x * kOBlock + threadIdx.x;
    uint32_t c = x < words ? (uint32_t)__popcll(bm[x]) : 0u;
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int k = 0; k < kOBlock / 64; ++k) t += s_c[k];
        bsum[blockIdx.x] = t;
    }
}

// one block: bsum[0, nb) to its exclusive scan in place, bsum[nb] = the total
__global__ __launch_bounds__(kOBlock) void k_pout_scan(unsigned long long* bsum, uint32_t nb) {
    __shared__ unsigned long long s_p[kOBlock];
    const uint32_t seg = (nb + kOBlock - 1) / kOBlock;
    const uint32_t lo = min(nb, threadIdx.x * seg), hi = min(nb, lo + seg);
    unsigned long long sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += bsum[i];
    s_p[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int k = 0; k < kOBlock; ++k) {
            const unsigned long long v = s_p[k];
            s_p[k] = run;
            run += v;
        }
        bsum[nb] = run;
    }
    __syncthreads();
    unsigned long long run = s_p[threadIdx.x];
    for (uint32_t i = lo; i < hi; ++i) {   // the thread's own segment: read, then written
        const unsigned long long v = bsum[i];
        bsum[i] = run;
        run += v;
    }
}

// off: the scanned block counts. A wavefront emits its 64 words one after the other, lane l the id of bit l
// at the word's offset + the set bits below l: ascending, and a dense word leaves in one 256-byte store.
// Nothing is written at or past cap (a bitmap that disagrees with the wave's count: part_out_ids).
__global__ __launch_bounds__(kOBlock) void k_pout_write(const unsigned long long* __restrict__ bm, uint64_t words,
                                                        const unsigned long long* __restrict__ off, uint32_t base,
                                                        uint32_t* out, uint64_t cap) {
    __shared__ uint32_t s_w[kOBlock / 64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t x = (uint64_t)blockIdx.x * kOBlock + threadIdx.x;
    const unsigned long long w = x < words ? bm[x] : 0ull;
    const uint32_t c = (uint32_t)__popcll(w);
    uint32_t inc = c;   // the wavefront's inclusive scan
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(inc, d);
        if (lane >= (uint32_t)d) inc += v;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    unsigned long long o = off[blockIdx.x] + (inc - c);
    for (uint32_t k = 0; k < wv; ++k) o += s_w[k];
    const uint64_t x0 = (uint64_t)blockIdx.x * kOBlock + (uint64_t)wv * 64;
    for (int k = 0; k < 64; ++k) {
        const unsigned long long wk = __shfl(w, k);
        const unsigned long long ok = __shfl(o, k);
        if (!wk) continue;   // wave-uniform
        if ((wk >> lane) & 1ull) {
            const unsigned long long idx = ok + (unsigned long long)__popcll(wk & ((1ull << lane) - 1));
            if (idx < cap) out[idx] = base + (uint32_t)((x0 + k) * 64 + lane);
        }
    }
}

inline uint32_t ogrid(uint64_t n) { return (uint32_t)std::min<uint64_t>(2048, std::max<uint64_t>(1, (n + kOBlock - 1) / kOBlock)); }

PartOut* pout_of(fgi_graph* g) {
    if (!g->pout) g->pout = new PartOut();
    return g->pout;
}

}  // namespace

fgi_status part_out_stage_roots(fgi_graph* g, uint32_t n, const uint32_t* roots, const uint8_t* imm, uint32_t** roots_dev,
                                uint8_t** imm_dev) {
    *roots_dev = nullptr;
    *imm_dev = nullptr;
    if (!n) return FGI_OK;
    // (the previous call's copies are complete: its wave waited for the stream)
    return pout_of(g)->roots.stage(g, n, roots, imm, roots_dev, imm_dev);
}

fgi_status part_out_bits(fgi_graph* g, const unsigned long long** bits_dev, uint64_t* words_out) {
    PartView pv;
    if (!part_view(g, &pv)) return set_err(g, FGI_ESTATE, "partition not initialised");
    PartOut* o = pout_of(g);
    const uint64_t words = ((uint64_t)g->ext_handles + 63) / 64;
    *words_out = words;
    if (!o->bits_valid) {
        FGI_TRY(grow(g, &o->bits, &o->bits_cap, words, "a partitioned wave's bitmap"));
        hipStream_t s = g->stream;
        const auto* inv64 = reinterpret_cast<const unsigned long long*>(g->inv_bm);
        const uint64_t n = g->last_wave_n;
        if (!g->lbl_perm) {   // engine indices are the handles
            hipLaunchKernelGGL(k_pout_mask, dim3(ogrid(words)), dim3(kOBlock), 0, s, inv64, pv.n_local, o->bits, words);
        } else {
            // the wave has been waited for, so the host knows its count when it chooses
            const int path = g->opt_part_ids_path;
            const bool gather = path == 2 || (path == 0 && n * kPartIdsGatherDen >= pv.n_local);
            if (gather) {
                hipLaunchKernelGGL(k_pout_gather, dim3(ogrid(words * 64)), dim3(kOBlock), 0, s, inv64,
                                   (const uint32_t*)g->pg_gc, pv.base, pv.n_local, o->bits, words);
            } else {
                FGI_HIP(g, hipMemsetAsync(o->bits, 0, words * 8, s));
                if (n)
                    hipLaunchKernelGGL(k_pout_scatter, dim3(ogrid(n)), dim3(kOBlock), 0, s, (const uint32_t*)g->inv, n,
                                       (const uint32_t*)g->pg_ig, pv.base, pv.n_local, o->bits);
            }
        }
        FGI_HIP(g, hipGetLastError());
        o->bits_valid = true;
    }
    *bits_dev = o->bits;
    return FGI_OK;
}

fgi_status part_out_ids(fgi_graph* g, const uint32_t** ids_dev, uint32_t* host_copy) {
    PartView pv;
    if (!part_view(g, &pv)) return set_err(g, FGI_ESTATE, "partition not initialised");
    PartOut* o = pout_of(g);
    if (!o->ids_valid) {
        const unsigned long long* bits = nullptr;
        uint64_t words = 0;
        FGI_TRY(part_out_bits(g, &bits, &words));
        const uint64_t n = g->last_wave_n;
        const uint32_t nb = (uint32_t)((words + kOBlock - 1) / kOBlock);
        FGI_TRY(grow(g, &o->bsum, &o->bsum_cap, (uint64_t)nb + 1, "a partitioned wave's block counts"));
        FGI_TRY(grow(g, &o->ids, &o->ids_cap, std::max<uint64_t>(n, 1), "a partitioned wave's id list"));
        hipStream_t s = g->stream;
        hipLaunchKernelGGL(k_pout_count, dim3(nb), dim3(kOBlock), 0, s, bits, words, o->bsum);
        hipLaunchKernelGGL(k_pout_scan, dim3(1), dim3(kOBlock), 0, s, o->bsum, nb);
        hipLaunchKernelGGL(k_pout_write, dim3(nb), dim3(kOBlock), 0, s, bits, words, (const unsigned long long*)o->bsum,
                           pv.base, o->ids, n);
        FGI_HIP(g, hipGetLastError());
        unsigned long long total = 0;
        FGI_HIP(g, hipMemcpyAsync(&total, o->bsum + nb, 8, hipMemcpyDeviceToHost, s));
        // the caller's copy rides on the count check's wait (at most n ids were written, whatever the total)
        if (host_copy && n) FGI_HIP(g, hipMemcpyAsync(host_copy, o->ids, n * 4, hipMemcpyDeviceToHost, s));
        FGI_HIP(g, hipStreamSynchronize(s));
        if (total != n)   // the code tables and the bitmap disagree: no list is better than a wrong one
            return set_err(g, FGI_ESTATE, "rank %u: the wave invalidated %llu of its slots, its bitmap in the host's "
                                          "numbering holds %llu", pv.rank, (unsigned long long)n, total);
        o->ids_valid = true;
    } else if (host_copy && g->last_wave_n) {
        FGI_HIP(g, hipMemcpyAsync(host_copy, o->ids, g->last_wave_n * 4, hipMemcpyDeviceToHost, g->stream));
        FGI_HIP(g, hipStreamSynchronize(g->stream));
    }
    *ids_dev = o->ids;
    return FGI_OK;
}

void part_out_destroy(fgi_graph* g) {
    PartOut* o = g->pout;
    if (!o) return;
    dfree(o->bits);
    dfree(o->ids);
    dfree(o->bsum);
    o->roots.release();
    delete o;
    g->pout = nullptr;
}

}  // namespace fgi

using namespace fgi;

extern "C" {

// what the three accessors share: FGI_OK with *live = whether a wave's result is there to be made (else
// the result is empty), or the status to return
static fgi_status pout_check(fgi_graph* g, const char* what, bool* live) {
    *live = false;
    if (!g->part) return set_err(g, FGI_ENOTSUP, "%s: not a partitioned graph (fgi_last_wave_ids, fgi_wave_ids_dev, "
                                                 "fgi_invalidate_bits serve a single device)", what);
    if (g->failed) return set_err(g, FGI_ESTATE, "%s: the graph is poisoned; fgi_restore or fgi_destroy", what);
    if (g->pout_kind == kPoutOther)
        return set_err(g, FGI_ENOTSUP, "%s: this rank's last call that ran cascades was no single wave "
                                       "(fgi_part_begin_compute, fgi_part_set_output and fgi_part_run_batch return "
                                       "their ids through out_ids)", what);
    *live = g->pout_kind == kPoutWave && g->last_wave_n != 0;
    return FGI_OK;
}

fgi_status fgi_part_last_wave_ids(fgi_graph* g, uint32_t* out_ids, uint64_t cap, uint64_t* out_n) {
    if (!g) return FGI_EINVAL;
    bool live = false;
    FGI_TRY(pout_check(g, "fgi_part_last_wave_ids", &live));
    const uint64_t n = live ? g->last_wave_n : 0;
    if (out_n) *out_n = n;
    if (!out_ids || !n) return FGI_OK;
    if (n > cap) return set_err(g, FGI_ECAPACITY, "the wave invalidated %llu of this rank's slots, the buffer holds %llu",
                                (unsigned long long)n, (unsigned long long)cap);
    hipSetDevice(g->device);
    const uint32_t* ids = nullptr;
    return part_out_ids(g, &ids, out_ids);   // on FGI_ESTATE (the count check) out_ids holds no list
}

fgi_status fgi_part_last_wave_bits(fgi_graph* g, uint64_t* out_bits, uint64_t words, uint64_t* out_n) {
    if (!g) return FGI_EINVAL;
    bool live = false;
    FGI_TRY(pout_check(g, "fgi_part_last_wave_bits", &live));
    if (out_n) *out_n = live ? g->last_wave_n : 0;
    if (!out_bits) return FGI_OK;
    const uint64_t need = ((uint64_t)g->ext_handles + 63) / 64;
    if (words < need)
        return set_err(g, FGI_ECAPACITY, "bitmap of %llu words needs %llu", (unsigned long long)words, (unsigned long long)need);
    if (!live) {
        memset(out_bits, 0, need * 8);
        return FGI_OK;
    }
    hipSetDevice(g->device);
    const unsigned long long* bits = nullptr;
    uint64_t w = 0;
    FGI_TRY(part_out_bits(g, &bits, &w));
    FGI_HIP(g, hipMemcpyAsync(out_bits, bits, need * 8, hipMemcpyDeviceToHost, g->stream));
    FGI_HIP(g, hipStreamSynchronize(g->stream));
    return FGI_OK;
}

fgi_status fgi_part_wave_ids_dev(fgi_graph* g, const uint32_t** ids_dev, uint64_t* n) {
    if (!g || !ids_dev) return FGI_EINVAL;
    *ids_dev = nullptr;
    bool live = false;
    FGI_TRY(pout_check(g, "fgi_part_wave_ids_dev", &live));
    if (n) *n = live ? g->last_wave_n : 0;
    if (!live) return FGI_OK;
    hipSetDevice(g->device);
    return part_out_ids(g, ids_dev, nullptr);
}

}  // extern "C"
