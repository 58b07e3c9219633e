// view.hip — the host-memory state view (fgi_state_view_open; C-ABI 0.6).
//
// Six bit planes over the boundary's handles (registered, consistent, computing, ioso, delay_started,
// has_delay) live twice: on the device, where the kernels below keep them current, and in fine-grained
// host memory, where any host thread reads a node's state with a load. A dirty bitmap (one bit per
// device plane word) names the words that differ; one flush kernel copies them and clears the bits.
//   k_view_build    every plane from the node words and the unfolded visit bits: one coalesced pass,
//                   64 handles per wavefront, a ballot per plane (open, bulk loads, fgi_restore)
//   k_view_wave     a wave's invalidated bitmap out of `consistent` and `delay_started`: streaming bit
//                   operations over 16-byte loads, no node word read
//   k_view_part_wave  the same for a partition rank whose engine runs on codes (fgi_part_state_view_open;
//                   C-ABI 0.7): a sparse wave scatters its set bits through code -> slot, a dense one
//                   gathers each plane word through slot -> code with one ballot
//   k_view_refresh  listed handles (a call's own lists, a wave's flagged records) from their node words
//   k_view_flush    dirty device words -> host planes, fenced at system scope
// A node's state is its word plus its visit bit, so nothing here calls fold: a visited
// node's canonical word is visited_word(word).
#define FGI_VIEW_OUT_OF_LINE 1   // this file emits the exported copies of fgi.h's inline read helpers
#include "fgi_internal.h"

#include <algorithm>
#include <cstring>

namespace fgi {
namespace {

constexpr int kVBlock = 256;

// where the engine keeps boundary handles: handle h lives at label s2l[h] if it is a hot slot, else K + h.
// A partition rank (K = 0) with codes keeps owned slot base + h (h < n_local) at engine index
// gc[base + h] - base, and engine index e < n_local is handle ig[base + e] - base; every other handle
// (the unowned slot bits, the detached handles) is its own index.
struct ViewMap {
    const uint32_t* s2l;   // null: no hot labels
    const uint32_t* l2s;
    uint32_t ext_slots, ext_handles, K, n_labels;
    const uint32_t* gc;    // null: no partition codes
    const uint32_t* ig;
    uint32_t base, n_local;   // a partition rank's first slot and its owned slots (0, 0 on a single device)
};
__device__ __forceinline__ uint32_t view_label(const ViewMap& m, uint32_t h) {
    if (m.gc) return h < m.n_local ? m.gc[m.base + h] - m.base : h;
    if (m.s2l && h < m.ext_slots) {
        const uint32_t l = m.s2l[h];
        if (l != FGI_NONE) return l;
    }
    return h + m.K;
}
__device__ __forceinline__ uint32_t view_handle(const ViewMap& m, uint32_t l) {
    if (l >= m.n_labels) return FGI_NONE;
    if (m.ig) return l < m.n_local ? m.ig[m.base + l] - m.base : l;
    if (l < m.K) return m.l2s ? m.l2s[l] : FGI_NONE;
    return l - m.K;
}

// the plane bits of the node at label l: bit p = plane p
__device__ __forceinline__ uint32_t plane_bits(const unsigned long long* __restrict__ node, const uint32_t* __restrict__ vis,
                                               uint32_t l) {
    unsigned long long w = node[l];
    if ((w & kVMask) == 0) return 0;
    if (vis && ((vis[l >> 5] >> (l & 31)) & 1u)) w = visited_word(w);
    const uint32_t f = word_to_flags(w);
    const uint32_t st = f & FGI_STATE_MASK;
    return (1u << kVpRegistered) | (st == FGI_CONSISTENT ? 1u << kVpConsistent : 0u) |
           (st == FGI_COMPUTING ? 1u << kVpComputing : 0u) | (f & FGI_F_INVALIDATE_ON_SET_OUTPUT ? 1u << kVpIoso : 0u) |
           (f & FGI_F_INVALIDATION_DELAY_STARTED ? 1u << kVpDelayStarted : 0u) | (f & FGI_F_HAS_DELAY ? 1u << kVpHasDelay : 0u);
}

__device__ __forceinline__ void mark_dirty(unsigned long long* dirty, uint64_t idx) {
    const unsigned long long m = 1ull << (idx & 63);
    if (!(dirty[idx >> 6] & m)) atomicOr(dirty + (idx >> 6), m);
}

__global__ __launch_bounds__(kVBlock) void k_view_build(ViewMap m, const unsigned long long* __restrict__ node,
                                                        const uint32_t* __restrict__ vis, unsigned long long* dev,
                                                        uint64_t words) {
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t lim = words * 64;
    for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < lim; h += nthr) {   // wave-uniform trip count
        const uint32_t b = h < m.ext_handles ? plane_bits(node, vis, view_label(m, (uint32_t)h)) : 0u;
        unsigned long long pw[kViewPlanes];
#pragma unroll
        for (uint32_t p = 0; p < kViewPlanes; ++p) pw[p] = __ballot((b >> p) & 1u);
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (uint32_t p = 0; p < kViewPlanes; ++p) dev[p * words + (h >> 6)] = pw[p];
        }
    }
}

// bits m of boundary word x leave `consistent` and `delay_started` (an Invalidated node reports neither)
__device__ __forceinline__ void wave_clear(unsigned long long* dev, unsigned long long* dirty, uint64_t words, uint64_t x,
                                           unsigned long long m) {
    unsigned long long* c = dev + kVpConsistent * words + x;
    if (*c & m) {
        atomicAnd(c, ~m);
        mark_dirty(dirty, kVpConsistent * words + x);
    }
    unsigned long long* d = dev + kVpDelayStarted * words + x;
    if (*d & m) {
        atomicAnd(d, ~m);
        mark_dirty(dirty, kVpDelayStarted * words + x);
    }
}

__device__ __forceinline__ void wave_word(const ViewMap& m, unsigned long long w, uint64_t x, uint64_t k64,
                                          unsigned long long* dev, unsigned long long* dirty, uint64_t words) {
    if (!w) return;
    if (x >= k64) {   // cold labels: K is a multiple of 64, so label word x is boundary word x - K / 64
        if (x - k64 < words) wave_clear(dev, dirty, words, x - k64, w);
        return;
    }
    if (!m.l2s) return;
    for (; w; w &= w - 1) {   // hot labels: each to its slot
        const uint32_t h = m.l2s[x * 64 + (uint32_t)(__ffsll((long long)w) - 1)];
        if (h < m.ext_handles) wave_clear(dev, dirty, words, h >> 6, 1ull << (h & 63));
    }
}

// inv64: the wave's invalidated bitmap over labels, lwords 64-bit words (16-byte aligned)
__global__ __launch_bounds__(kVBlock) void k_view_wave(ViewMap m, const unsigned long long* __restrict__ inv64, uint64_t lwords,
                                                       unsigned long long* dev, unsigned long long* dirty, uint64_t words) {
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t k64 = m.K / 64;
    const uint64_t pairs = lwords / 2;
    const ulonglong2* inv2 = reinterpret_cast<const ulonglong2*>(inv64);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += nthr) {
        const ulonglong2 w = inv2[i];
        if (!(w.x | w.y)) continue;
        wave_word(m, w.x, 2 * i, k64, dev, dirty, words);
        wave_word(m, w.y, 2 * i + 1, k64, dev, dirty, words);
    }
    if ((lwords & 1) && blockIdx.x == 0 && threadIdx.x == 0)
        wave_word(m, inv64[lwords - 1], lwords - 1, k64, dev, dirty, words);
}

// A partition rank's wave with codes. Codes are dealt round-robin over the pull blocks' runs, so the 64
// bits of one word of inv64 (over engine indices) belong to 64 unrelated plane words. inv_n: the rank's
// invalidated count, left by the final collect queued before this kernel; every thread reads the same
// value, so the choice below is grid-uniform and the host waits for nothing to make it.
// path: 0 by the count (gather from n_local / den invalidated handles on), 1 scatter, 2 gather.
//   scatter: as k_view_wave's hot labels: stream the bitmap, each set bit to its handle's plane words
//   gather:  a wavefront per plane word x: lane l probes the bit of handle 64 x + l's engine index; the
//            ballot is the word of newly invalidated handles, applied by lane 0 with plain loads and
//            stores (the wavefront owns plane word x; nothing else runs on the stream)
__global__ __launch_bounds__(kVBlock) void k_view_part_wave(ViewMap m, const unsigned long long* __restrict__ inv64,
                                                            uint64_t lwords, const unsigned long long* __restrict__ inv_n,
                                                            int path, uint32_t den, unsigned long long* dev,
                                                            unsigned long long* dirty, uint64_t words) {
    // (the count covers the rank's owned slots only and just steers the choice: no early return on 0, so a
    // bit at a detached handle's index would still be applied, as k_view_wave would apply it)
    const unsigned long long n_inv = *inv_n;
    const bool gather = path == 2 || (path == 0 && n_inv * den >= m.n_local);
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!gather) {
        const uint64_t pairs = lwords / 2;
        const ulonglong2* inv2 = reinterpret_cast<const ulonglong2*>(inv64);
        for (uint64_t i = tid; i <= pairs; i += nthr) {
            unsigned long long w[2] = {0ull, 0ull};
            if (i < pairs) {
                const ulonglong2 v = inv2[i];
                w[0] = v.x;
                w[1] = v.y;
            } else if (lwords & 1) {
                w[0] = inv64[lwords - 1];
            }
#pragma unroll
            for (int k = 0; k < 2; ++k)
                for (unsigned long long b = w[k]; b; b &= b - 1) {
                    const uint32_t h = view_handle(m, (uint32_t)((2 * i + k) * 64) + (uint32_t)(__ffsll((long long)b) - 1));
                    if (h < m.ext_handles) wave_clear(dev, dirty, words, h >> 6, 1ull << (h & 63));
                }
        }
        return;
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = nthr >> 6;
    for (uint64_t x = tid >> 6; x < words; x += nwaves) {   // wave-uniform trip count
        const uint32_t h = (uint32_t)(x * 64 + lane);
        bool hit = false;
        if (h < m.ext_handles) {
            const uint32_t e = view_label(m, h);
            hit = ((uint64_t)e >> 6) < lwords && ((inv64[e >> 6] >> (e & 63)) & 1ull);
        }
        const unsigned long long w = __ballot(hit);
        if (lane == 0 && w) {
            unsigned long long* c = dev + kVpConsistent * words + x;
            const unsigned long long cv = *c;
            if (cv & w) {
                *c = cv & ~w;
                mark_dirty(dirty, kVpConsistent * words + x);
            }
            unsigned long long* d = dev + kVpDelayStarted * words + x;
            const unsigned long long dv = *d;
            if (dv & w) {
                *d = dv & ~w;
                mark_dirty(dirty, kVpDelayStarted * words + x);
            }
        }
    }
}

__global__ __launch_bounds__(kVBlock) void k_view_refresh(ViewMap m, int kind, const void* __restrict__ list, uint64_t n,
                                                          const unsigned long long* __restrict__ n_dev,
                                                          const unsigned long long* __restrict__ node,
                                                          const uint32_t* __restrict__ vis, unsigned long long* dev,
                                                          unsigned long long* dirty, uint64_t words) {
    if (n_dev && *n_dev < n) n = *n_dev;
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthr) {
        uint32_t h;
        if (kind == kViewRecords) h = (uint32_t)(static_cast<const unsigned long long*>(list)[i] >> 32) - m.base;
        else if (kind == kViewCodes) {   // a partition's global engine ids: the owned ones
            const uint32_t l = static_cast<const uint32_t*>(list)[i] - m.base;
            h = l < m.n_local ? view_handle(m, l) : FGI_NONE;
        } else if (kind == kViewLabels) h = view_handle(m, static_cast<const uint32_t*>(list)[i]);
        else h = static_cast<const uint32_t*>(list)[i];
        if (h >= m.ext_handles) continue;
        const uint32_t b = plane_bits(node, vis, view_label(m, h));
        const unsigned long long bit = 1ull << (h & 63);
#pragma unroll
        for (uint32_t p = 0; p < kViewPlanes; ++p) {
            unsigned long long* w = dev + p * words + (h >> 6);
            const bool want = (b >> p) & 1u;
            if (((*w & bit) != 0) == want) continue;
            if (want) atomicOr(w, bit);
            else atomicAnd(w, ~bit);
            mark_dirty(dirty, p * words + (h >> 6));
        }
    }
}

// The host planes are written with plain vector stores (8 bytes each: a host reader sees a plane word's
// old or new value); the fence orders them before whatever the stream publishes next.
__global__ __launch_bounds__(kVBlock) void k_view_flush(unsigned long long* dirty, uint64_t dirty_words,
                                                        const unsigned long long* __restrict__ dev, unsigned long long* host,
                                                        uint64_t total, unsigned long long* pub) {
    // a wavefront per dirty word: lane l copies plane word 64 * i + l if its bit is set, so a dense wave's
    // words leave in 512-byte runs
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    unsigned long long mine = 0;
    for (uint64_t i = wave; i < dirty_words; i += nwaves) {   // wave-uniform
        const unsigned long long d = dirty[i];
        if (!d) continue;
        const uint64_t idx = i * 64 + lane;
        if (((d >> lane) & 1ull) && idx < total) host[idx] = dev[idx];
        if (lane == 0) {
            dirty[i] = 0ull;
            mine += (unsigned long long)__popcll(d);
        }
    }
    if (mine) atomicAdd(pub, mine);
    __threadfence_system();
}

inline uint32_t vgrid(uint64_t n) { return (uint32_t)std::min<uint64_t>(2048, std::max<uint64_t>(1, (n + kVBlock - 1) / kVBlock)); }

ViewMap view_map(const fgi_graph* g) {
    const View* v = g->view;
    return ViewMap{g->lbl_hot ? g->s2l : nullptr, g->lbl_hot ? g->l2s : nullptr, g->ext_slots, g->ext_handles, g->lbl_K,
                   g->n_handles, g->lbl_perm ? g->pg_gc : nullptr, g->lbl_perm ? g->pg_ig : nullptr, v->part_base,
                   v->part_n_local};
}
// the visit bitmap while it holds this graph's unfolded visits (fgi_restore may have left it stale)
const uint32_t* view_vis(const fgi_graph* g) { return g->v_dirty && !g->vis_stale ? g->vis_bm : nullptr; }

void seq_store(View* v, bool odd) {
    unsigned long long* s = v->host + kViewPlanes * v->words;
    const unsigned long long cur = __atomic_load_n(s, __ATOMIC_RELAXED);
    if (((cur & 1) != 0) != odd) __atomic_store_n(s, cur + 1, __ATOMIC_SEQ_CST);
}

}  // namespace

void view_begin(fgi_graph* g) {
    if (!view_on(g)) return;
    View* v = g->view;
    if (!(__atomic_load_n(v->host + kViewPlanes * v->words, __ATOMIC_RELAXED) & 1)) ++v->updates;
    seq_store(v, true);
}

void view_end(fgi_graph* g) {
    if (!view_on(g) || g->aw[0].busy || g->aw[1].busy) return;
    seq_store(g->view, false);
}

fgi_status view_rebuild(fgi_graph* g) {
    if (!view_on(g)) return FGI_OK;
    View* v = g->view;
    view_begin(g);
    hipStream_t s = g->stream;
    hipLaunchKernelGGL(k_view_build, dim3(vgrid(v->words * 64)), dim3(kVBlock), 0, s, view_map(g),
                       reinterpret_cast<const unsigned long long*>(g->node), view_vis(g), v->dev, v->words);
    FGI_HIP(g, hipGetLastError());
    FGI_HIP(g, hipMemsetAsync(v->dirty, 0, v->dirty_words * 8, s));
    FGI_HIP(g, hipMemcpyAsync(v->host, v->dev, kViewPlanes * v->words * 8, hipMemcpyDeviceToHost, s));
    FGI_HIP(g, hipStreamSynchronize(s));
    ++v->full_builds;
    v->pub_base += kViewPlanes * v->words;
    view_end(g);
    return FGI_OK;
}

fgi_status view_wave(fgi_graph* g) {
    if (!view_on(g)) return FGI_OK;
    View* v = g->view;
    const uint64_t lwords = ((uint64_t)g->n_handles + 63) / 64;
    hipLaunchKernelGGL(k_view_wave, dim3(vgrid(lwords / 2 + 1)), dim3(kVBlock), 0, g->stream, view_map(g),
                       reinterpret_cast<const unsigned long long*>(g->inv_bm), lwords, v->dev, v->dirty, v->words);
    FGI_HIP(g, hipGetLastError());
    return FGI_OK;
}

fgi_status view_part_wave(fgi_graph* g) {
    if (!view_on(g)) return FGI_OK;
    if (!g->lbl_perm) return view_wave(g);   // engine indices are the handles: k_view_wave with K = 0
    View* v = g->view;
    const uint64_t lwords = ((uint64_t)g->n_handles + 63) / 64;
    // a grid for the gather (a wavefront per plane word); the scatter strides over it
    hipLaunchKernelGGL(k_view_part_wave, dim3(vgrid(v->words * 64)), dim3(kVBlock), 0, g->stream, view_map(g),
                       reinterpret_cast<const unsigned long long*>(g->inv_bm), lwords, &g->ctr->inv, g->opt_part_view_path,
                       kPartViewGatherDen, v->dev, v->dirty, v->words);
    FGI_HIP(g, hipGetLastError());
    return FGI_OK;
}

fgi_status view_refresh(fgi_graph* g, int kind, const void* list_dev, uint64_t n, const unsigned long long* n_dev) {
    if (!view_on(g) || !n || !list_dev) return FGI_OK;
    View* v = g->view;
    hipLaunchKernelGGL(k_view_refresh, dim3(vgrid(n)), dim3(kVBlock), 0, g->stream, view_map(g), kind, list_dev, n, n_dev,
                       reinterpret_cast<const unsigned long long*>(g->node), view_vis(g), v->dev, v->dirty, v->words);
    FGI_HIP(g, hipGetLastError());
    return FGI_OK;
}

fgi_status view_refresh_host(fgi_graph* g, const uint32_t* handles, uint64_t n) {
    if (!view_on(g) || !n) return FGI_OK;
    Tmp td;
    uint32_t* d;
    FGI_TRY(tmalloc(g, td, &d, n));
    FGI_HIP(g, hipMemcpyAsync(d, handles, n * 4, hipMemcpyHostToDevice, g->stream));
    FGI_TRY(view_refresh(g, kViewHandles, d, n));
    FGI_HIP(g, hipStreamSynchronize(g->stream));   // the caller's array is pageable
    return FGI_OK;
}

fgi_status view_flush(fgi_graph* g) {
    if (!view_on(g)) return FGI_OK;
    View* v = g->view;
    hipLaunchKernelGGL(k_view_flush, dim3(vgrid(v->dirty_words * 64)), dim3(kVBlock), 0, g->stream, v->dirty, v->dirty_words,
                       v->dev, v->host, kViewPlanes * v->words, v->pub_dev);
    FGI_HIP(g, hipGetLastError());
    return FGI_OK;
}

fgi_status view_commit(fgi_graph* g) {
    if (!view_on(g)) return FGI_OK;
    FGI_TRY(view_flush(g));
    FGI_HIP(g, hipStreamSynchronize(g->stream));
    ++g->view->extra_waits;
    view_end(g);
    return FGI_OK;
}

void view_destroy(fgi_graph* g) {
    View* v = g->view;
    if (!v) return;
    if (v->host) (void)hipHostFree(v->host);
    if (v->dev) (void)hipFree(v->dev);
    if (v->dirty) (void)hipFree(v->dirty);
    if (v->pub_dev) (void)hipFree(v->pub_dev);
    delete v;
    g->view = nullptr;
}

}  // namespace fgi

using namespace fgi;

extern "C" {

// what both opens share: the planes on first use, a full build on every open, the caller's struct
static fgi_status view_open(fgi_graph* g, fgi_state_view* out, uint32_t part_base, uint32_t part_n_local) {
    hipSetDevice(g->device);
    if (g->aw[0].busy || g->aw[1].busy) FGI_TRY(drain_async(g));
    if (!g->view) {
        View* v = new View();
        g->view = v;
        v->words = ((uint64_t)g->ext_handles + 63) / 64;
        const uint64_t total = kViewPlanes * v->words;
        v->dirty_words = (total + 63) / 64;
        if (hipHostMalloc(reinterpret_cast<void**>(&v->host), (total + 8) * 8, hipHostMallocCoherent) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&v->dev), total * 8) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&v->dirty), v->dirty_words * 8) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&v->pub_dev), 8) != hipSuccess) {
            view_destroy(g);
            return set_err(g, FGI_ENOMEM, "fgi_state_view_open: the planes");
        }
        memset(v->host, 0, (total + 8) * 8);
        FGI_HIP(g, hipMemsetAsync(v->pub_dev, 0, 8, g->stream));
    }
    View* v = g->view;
    v->part_base = part_base;
    v->part_n_local = part_n_local;
    if (!v->open) {
        v->open = true;
        g->wave_clean = g->wave_kept = false;   // a wave with a view open keeps its invalidated bitmap: the next one clears it
        FGI_TRY(view_rebuild(g));
    }
    out->n_handles = g->ext_handles;
    out->words = v->words;
    const uint64_t* h = reinterpret_cast<const uint64_t*>(v->host);
    out->registered = h + kVpRegistered * v->words;
    out->consistent = h + kVpConsistent * v->words;
    out->computing = h + kVpComputing * v->words;
    out->ioso = h + kVpIoso * v->words;
    out->delay_started = h + kVpDelayStarted * v->words;
    out->has_delay = h + kVpHasDelay * v->words;
    out->seq = h + kViewPlanes * v->words;
    return FGI_OK;
}

fgi_status fgi_state_view_open(fgi_graph* g, fgi_state_view* out) {
    if (!g || !out || out->struct_size < sizeof(fgi_state_view)) return FGI_EINVAL;
    // (a partition's ranks each hold their slots' share: fgi_part_state_view_open)
    if (g->part) return set_err(g, FGI_ENOTSUP, "fgi_state_view_open: a partitioned graph has a view per rank (fgi_part_state_view_open)");
    if (g->failed) return set_err(g, FGI_ESTATE, "fgi_state_view_open: the graph is poisoned; fgi_restore or fgi_destroy");
    return view_open(g, out, 0, 0);
}

fgi_status fgi_part_state_view_open(fgi_graph* g, fgi_state_view* out, uint32_t* out_base) {
    if (!g || !out || out->struct_size < sizeof(fgi_state_view)) return FGI_EINVAL;
    PartView pv;
    if (!g->part || !part_view(g, &pv))
        return set_err(g, FGI_ENOTSUP, "fgi_part_state_view_open: not a partitioned graph (fgi_state_view_open)");
    if (g->failed) return set_err(g, FGI_ESTATE, "fgi_part_state_view_open: the graph is poisoned; fgi_restore or fgi_destroy");
    FGI_TRY(view_open(g, out, pv.base, pv.n_local));   // no collective: the rank's own handles
    if (out_base) *out_base = pv.base;
    return FGI_OK;
}

fgi_status fgi_state_view_close(fgi_graph* g) {
    if (!g) return FGI_EINVAL;
    if (!view_on(g)) return FGI_OK;
    hipSetDevice(g->device);
    if (!g->failed && (g->aw[0].busy || g->aw[1].busy)) FGI_TRY(drain_async(g));
    FGI_HIP(g, hipStreamSynchronize(g->stream));
    seq_store(g->view, false);
    g->view->open = false;   // the planes stay allocated: a second open returns the same ones
    return FGI_OK;
}

fgi_status fgi_state_view_stats(fgi_graph* g, fgi_view_stats* out) {
    if (!g || !out) return FGI_EINVAL;
    out->updates = out->words_published = out->full_builds = out->extra_waits = 0;
    const View* v = g->view;
    if (!v) return FGI_OK;
    hipSetDevice(g->device);
    unsigned long long pub = 0;
    FGI_HIP(g, hipMemcpyAsync(&pub, v->pub_dev, 8, hipMemcpyDeviceToHost, g->stream));
    FGI_HIP(g, hipStreamSynchronize(g->stream));
    out->updates = v->updates;
    out->words_published = v->pub_base + pub;
    out->full_builds = v->full_builds;
    out->extra_waits = v->extra_waits;
    return FGI_OK;
}

}  // extern "C"
