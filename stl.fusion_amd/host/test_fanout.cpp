// test_fanout.cpp — the mirror's replica fan-out with ComputedRegistry::DeviceFanout on against the same
// registry with it off (the host gather over sub_head_). Needs a GPU; run by tests/test_gpu_host_fanout.py.
//
// Shape: 100 hubs x 100 leaves (one leaf in ten delayed), 7 peers, PeerBatch 64, every leaf held by one or two
// peers and every hub by one, plus a small second component a reentrant sink invalidates. Both registries must
// deliver the same call ids per peer, in the same order, cut into the same batches, each exactly once:
//   normal      one scope over all hubs, with the wave's ids returned as a list and as a bitmap
//   reentrant   peer 0's sink runs a wave of its own from inside its first batch
//   async       the scope flushed as an asynchronous wave, fanned out at its completion (fgi_fanout_ids)
// `--bench` runs BASELINE configs[4]'s 10M-leaf workload (test_fusion.cpp's fanout_10m, without delayed leaves)
// with DeviceFanout on and prints one JSON line.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "fusion.hpp"

using namespace fusion;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                            \
        }                                                                        \
    } while (0)

static void must(fgi_status s, const char* what) {
    if (s != FGI_OK) throw FgiError(s, what);
}

static uint64_t version_of(uint32_t s) {
    uint64_t x = (uint64_t)s * 0x9E3779B97F4A7C15ull + 0x5EED00E0;
    x ^= x >> 31;
    return ((x * 0xBF58476D1CE4E5B9ull) & ((1ull << 54) - 1)) | 1ull;
}

// hubs [0, H), their leaves [H, H + H * Lh), then `extra` more hubs with 5 leaves each
static void load_hubs(ComputedRegistry& r, uint32_t H, uint32_t Lh, uint32_t extra, uint32_t delayed_every) {
    const uint32_t N = H + H * Lh + extra * 6;
    std::vector<uint32_t> slot(N), flags(N);
    std::vector<uint64_t> ver(N);
    for (uint32_t s = 0; s < N; ++s) {
        slot[s] = s;
        ver[s] = version_of(s);
        const bool delayed = delayed_every && s >= H && s < H + H * Lh && s % delayed_every == 0;
        flags[s] = FGI_CONSISTENT | (delayed ? FGI_F_HAS_DELAY : 0u);
    }
    must(fgi_register_nodes(r.Graph(), N, slot.data(), ver.data(), flags.data()), "register");
    std::vector<uint32_t> hub, leaf;
    std::vector<uint64_t> tag;
    for (uint32_t k = 0; k < H * Lh; ++k) {
        hub.push_back(k / Lh);
        leaf.push_back(H + k);
    }
    const uint32_t x0 = H + H * Lh;
    for (uint32_t e = 0; e < extra; ++e)
        for (uint32_t k = 0; k < 5; ++k) {
            hub.push_back(x0 + e * 6);
            leaf.push_back(x0 + e * 6 + 1 + k);
        }
    for (const uint32_t l : leaf) tag.push_back(version_of(l));
    must(fgi_load_edges(r.Graph(), hub.size(), hub.data(), leaf.data(), tag.data()), "load");
}

// what the peers saw: per peer its call ids in arrival order and the size of every batch
struct Seen {
    std::vector<std::vector<uint64_t>> calls, batches;
    uint64_t fan_calls = 0, fan_batches = 0;
    uint32_t device = 0;
    bool operator==(const Seen& o) const { return calls == o.calls && batches == o.batches; }
};

enum { kNormalIds, kNormalBits, kReentrant, kAsync };

static Seen run_case(bool device, int what) {
    const uint32_t H = 100, Lh = 100, P = 7, N0 = H + H * Lh;
    ComputedRegistry r(N0 + 12, 16);
    r.DeviceFanout = device;
    r.PeerBatch = 64;
    r.WaveOutput = what == kNormalBits ? 2 : 1;
    load_hubs(r, H, Lh, 2, 10);
    Seen seen;
    seen.calls.resize(P);
    seen.batches.resize(P);
    bool nested = false;
    for (uint32_t q = 0; q < P; ++q)
        r.AddPeer([&, q](uint32_t peer, const uint64_t* ids, size_t n) {
            CHECK(peer == q && n >= 1 && n <= 64);
            seen.calls[peer].insert(seen.calls[peer].end(), ids, ids + n);
            seen.batches[peer].push_back(n);
            if (what == kReentrant && peer == 0 && !nested) {   // a sink that runs a wave of its own
                nested = true;
                r.InvalidateSlots({N0});
            }
        });
    std::vector<uint32_t> sh, sp;
    std::vector<uint64_t> sc;
    auto sub = [&](uint32_t h, uint32_t p, uint64_t c) {
        sh.push_back(h);
        sp.push_back(p);
        sc.push_back(c);
    };
    for (uint32_t h = 0; h < H; ++h) sub(h, h % P, 8ull * h);
    for (uint32_t l = H; l < N0; ++l) {
        sub(l, l % P, 8ull * l);
        if ((l * 3 + 1) % P != l % P && l % 4 == 0) sub(l, (l * 3 + 1) % P, 8ull * l + 1);   // two peers on one handle
    }
    for (uint32_t x = N0; x < N0 + 12; ++x) sub(x, x % P, 8ull * x);
    r.Subscribe(sh.size(), sh.data(), sp.data(), sc.data());
    std::vector<uint32_t> roots(H);
    for (uint32_t h = 0; h < H; ++h) roots[h] = h;
    if (what == kAsync) {
        const uint64_t t = r.InvalidateSlotsAsync(roots);
        CHECK(r.PendingWaves() == 1);
        for (auto& c : seen.calls) CHECK(c.empty());   // nothing fans out before the completion
        r.Complete(t);
    } else {
        r.InvalidateSlots(roots);
    }
    // exactly once, and exactly the entries of the invalidated nodes
    uint64_t want = 0;
    for (size_t i = 0; i < sh.size(); ++i) {
        const uint32_t h = sh[i];
        const bool delayed = h >= H && h < N0 && h % 10 == 0;
        const bool in_first = h < N0 && !delayed;
        const bool in_nested = what == kReentrant && h >= N0 && h < N0 + 6;
        want += (in_first || in_nested) ? 1 : 0;
    }
    std::unordered_set<uint64_t> once;
    uint64_t got = 0;
    for (auto& c : seen.calls)
        for (const uint64_t id : c) {
            ++got;
            CHECK(once.insert(id).second);
        }
    CHECK(got == want);
    const FanoutStats& f = r.LastFanout();
    seen.fan_calls = f.calls;
    seen.fan_batches = f.batches;
    seen.device = f.device;
    CHECK(f.device == (device ? 1u : 0u));
    if (what == kReentrant) CHECK(nested);
    // a second wave over the same hubs delivers nothing more
    r.InvalidateSlots(roots);
    uint64_t after = 0;
    for (auto& c : seen.calls) after += c.size();
    CHECK(after == got);
    if (device) {
        // a subscription to a node that is Invalidated already is delivered at once, and only then
        const size_t before = seen.calls[3].size();
        r.Subscribe(H + 1, 3, 777777);   // leaf 101: invalidated above
        CHECK(seen.calls[3].size() == before + 1 && seen.calls[3].back() == 777777);
        seen.calls[3].pop_back();
        seen.batches[3].pop_back();
        fgi_sub_stats st{};
        must(fgi_sub_stats_get(r.Graph(), &st), "stats");
        CHECK(st.delivered == got && st.live == sh.size() - got);
    }
    return seen;
}

static void compare(int what, const char* name) {
    const Seen off = run_case(false, what), on = run_case(true, what);
    CHECK(off == on);
    CHECK(off.fan_calls == on.fan_calls && off.fan_batches == on.fan_batches);
    uint64_t n = 0;
    for (auto& c : on.calls) n += c.size();
    std::printf("%s: %llu call ids, same per peer, same order, same batches: %s\n", name, (unsigned long long)n,
                off == on ? "yes" : "NO");
}

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : v[v.size() / 2];
}
static double spread(const std::vector<double>& v) {
    return v.empty() ? 0.0 : *std::max_element(v.begin(), v.end()) - *std::min_element(v.begin(), v.end());
}
static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// 10,000 hubs x 1,000 leaves, 100 peers, every leaf held by peer leaf % 100. all: one scope over all hubs,
// `reps` times (restore, subscribe, wave). one: one hub's scope with the 10M subscriptions live, on each path.
static void bench(int reps) {
    const uint32_t H = 10000, Lh = 1000, P = 100, N = H + H * Lh;
    ComputedRegistry r(N, 64);
    r.DeviceFanout = true;
    r.WaveOutput = 2;
    load_hubs(r, H, Lh, 0, 0);
    must(fgi_snapshot(r.Graph()), "snapshot");
    std::vector<uint64_t> got(P, 0), last(P, 0);
    uint64_t order_bad = 0;
    for (uint32_t q = 0; q < P; ++q)
        r.AddPeer([&](uint32_t peer, const uint64_t* ids, size_t n) {
            for (size_t i = 0; i < n; ++i) {
                order_bad += (got[peer] + i && ids[i] <= last[peer]) ? 1 : 0;
                last[peer] = ids[i];
            }
            got[peer] += n;
        });
    std::vector<uint32_t> roots(H), sh(N - H), sp(N - H);
    std::vector<uint64_t> sc(N - H);
    for (uint32_t h = 0; h < H; ++h) roots[h] = h;
    for (uint32_t k = 0; k < N - H; ++k) {
        sh[k] = H + k;
        sp[k] = (H + k) % P;
        sc[k] = H + k;
    }
    std::vector<double> sub_ms, disp_ms, kern_ms, wave_ms, one_disp[2], one_kern[2];
    for (int rep = 0; rep < reps + 1; ++rep) {   // the first repeat warms up (allocations, the wave's plan)
        must(fgi_restore(r.Graph()), "restore");
        std::fill(got.begin(), got.end(), 0);
        const auto t0 = std::chrono::steady_clock::now();
        r.Subscribe(sh.size(), sh.data(), sp.data(), sc.data());
        const double s_ms = ms_since(t0);
        // one hub's scope first, once per path, on hubs no other repeat uses
        double od[2] = {0, 0}, ok[2] = {0, 0};
        for (int path = 1; path <= 2; ++path) {
            must(fgi_set_option(r.Graph(), FGI_OPT_FANOUT_PATH, path), "option");
            r.InvalidateSlots({(uint32_t)(2 * rep + path - 1)});
            CHECK(r.LastFanout().calls == Lh && r.LastFanout().device == 1);
            od[path - 1] = r.LastFanout().dispatch_ms;
            ok[path - 1] = r.LastFanout().device_kernel_ms;
        }
        must(fgi_set_option(r.Graph(), FGI_OPT_FANOUT_PATH, 0), "option");
        std::fill(got.begin(), got.end(), 0);
        order_bad = 0;
        r.InvalidateSlots(roots);
        const FanoutStats& f = r.LastFanout();
        uint64_t tot = 0;
        for (const uint64_t x : got) tot += x;
        CHECK(f.device == 1 && order_bad == 0 && tot == (uint64_t)(H - 2) * Lh && f.calls == tot);
        if (rep == 0) continue;
        sub_ms.push_back(s_ms);
        disp_ms.push_back(f.dispatch_ms);
        kern_ms.push_back(f.device_kernel_ms);
        wave_ms.push_back(r.LastWave().total_ms);
        for (int k = 0; k < 2; ++k) {
            one_disp[k].push_back(od[k]);
            one_kern[k].push_back(ok[k]);
        }
    }
    std::printf("DEVICE_FANOUT {\"workload\": \"10000 hubs x 1000 leaves, 100 peers\", \"reps\": %d, "
                "\"subscribe_ms\": {\"median\": %.3f, \"spread\": %.3f}, "
                "\"wave_return_to_last_sink_ms\": {\"median\": %.3f, \"spread\": %.3f}, "
                "\"fanout_kernel_ms\": {\"median\": %.3f, \"spread\": %.3f}, \"wave_call_ms\": {\"median\": %.3f}, "
                "\"one_hub\": {\"list\": {\"dispatch_ms\": %.3f, \"kernel_ms\": %.3f}, "
                "\"bitmap\": {\"dispatch_ms\": %.3f, \"kernel_ms\": %.3f}}}\n",
                reps, median(sub_ms), spread(sub_ms), median(disp_ms), spread(disp_ms), median(kern_ms), spread(kern_ms),
                median(wave_ms), median(one_disp[0]), median(one_kern[0]), median(one_disp[1]), median(one_kern[1]));
}

int main(int argc, char** argv) {
    try {
        if (argc > 1 && std::strcmp(argv[1], "--bench") == 0) {
            bench(argc > 2 ? std::max(1, std::atoi(argv[2])) : 5);
        } else {
            compare(kNormalIds, "normal (id list)");
            compare(kNormalBits, "normal (bitmap)");
            compare(kReentrant, "reentrant sink");
            compare(kAsync, "asynchronous completion");
        }
    } catch (const FgiError& e) {
        std::fprintf(stderr, "FgiError %d: %s\n", (int)e.status, e.what());
        return 2;
    }
    std::printf("%d/%d checks passed\n", g_checks - g_fail, g_checks);
    return g_fail ? 1 : 0;
}
