// test_timers.cpp — the delay timers in the engine (ComputedRegistry::DeviceTimers, fgi_timers_*) against the
// registry's host timers: test_delay.cpp's scenarios and a 10,000-leaf hub graph with every 10th leaf delayed,
// each run on two registries, one with DeviceTimers on and one with it off, driven by the same fake clock. The
// two must agree on the handler invocations per node, on State() and Flags() of every node after every step, on
// what RunDueTimers returns, and on PendingTimers() wherever the host path's count is the engine's (the engine
// keeps the entry of a node invalidated before its due time until that time comes).
// Needs a GPU; run by tests/test_gpu_host_timers.py.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "fusion.hpp"

using namespace fusion;
using namespace std::chrono_literals;
using ns = std::chrono::nanoseconds;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        ++g_checks;                                                                       \
        if (!(cond)) {                                                                    \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                                     \
        }                                                                                 \
    } while (0)

// one registry, its clock, the nodes it made (by a label of the test's) and everything observable, in order
struct Run {
    ComputedRegistry r;
    ComputedRegistry::TimePoint now{};
    std::vector<std::pair<std::string, std::shared_ptr<Computed>>> nodes;
    std::vector<std::string> trace;
    Run(bool device, uint32_t n_slots, ns default_delay) : r(n_slots) {
        r.DeviceTimers = device;
        r.DefaultInvalidationDelay = default_delay;
        r.Clock = [this] { return now; };
    }
    std::shared_ptr<Computed> Track(const std::string& label, std::shared_ptr<Computed> c) {
        c->OnInvalidated([this, label](Computed&) { trace.push_back("handler " + label); });
        nodes.emplace_back(label, c);
        return c;
    }
    // ComputeMethodFunctionBase.Compute: begin (with the node's InvalidationDelay), AddUsed each dep, TrySetOutput
    std::shared_ptr<Computed> Compute(const std::string& in, std::initializer_list<std::shared_ptr<Computed>> deps = {},
                                      ns delay = 0ns) {
        auto c = r.BeginCompute(in, delay);
        for (auto& d : deps) CHECK(r.AddUsed(*c, *d) == FGI_USED_ADDED);
        CHECK(r.SetOutput(*c));
        return Track(in, c);
    }
    // after a step: every node's state, and the pending count where both paths hold the same entries
    void Step(const std::string& what, bool pending_exact = true) {
        std::string s = "step " + what + ":";
        for (auto& n : nodes) s += " " + n.first + "=" + std::to_string((int)n.second->State()) + "/" + std::to_string(n.second->Flags());
        if (pending_exact) s += " pending=" + std::to_string(r.PendingTimers());
        trace.push_back(s);
    }
    void Tick(ns d, const std::string& what, bool pending_exact = true) {
        now += d;
        trace.push_back("fired " + std::to_string(r.RunDueTimers()));
        Step(what, pending_exact);
    }
};

using Scenario = std::function<void(Run&)>;

// the scenario on a registry with host timers and on one with the engine's: the same trace, line by line
static void both(const char* name, uint32_t n_slots, ns default_delay, const Scenario& sc, size_t min_lines) {
    Run host(false, n_slots, default_delay), dev(true, n_slots, default_delay);
    sc(host);
    sc(dev);
    CHECK(host.trace.size() >= min_lines);
    CHECK(host.trace.size() == dev.trace.size());
    size_t same = 0;
    for (size_t i = 0; i < host.trace.size() && i < dev.trace.size(); ++i) {
        if (host.trace[i] == dev.trace[i]) {
            ++same;
            continue;
        }
        std::fprintf(stderr, "%s, line %zu:\n  host:   %s\n  device: %s\n", name, i, host.trace[i].c_str(), dev.trace[i].c_str());
    }
    CHECK(same == host.trace.size());
    fgi_timer_stats st{};
    CHECK(fgi_timers_stats_get(dev.r.Graph(), &st) == FGI_OK && st.armed == st.fired + st.dropped + st.stored);
    CHECK(fgi_timers_stats_get(host.r.Graph(), &st) == FGI_OK && st.armed == 0);   // never opened there
    std::printf("%s: %zu trace lines agree\n", name, same);
}

// the chain a -> b -> c -> d (delay 5 s) -> e
static void chain(Run& x) {
    auto a = x.Compute("a");
    auto b = x.Compute("b", {a});
    auto c = x.Compute("c", {b});
    auto d = x.Compute("d", {c}, 5s);
    x.Compute("e", {d});
}

static void invalidation_delay_then_timer(Run& x) {
    chain(x);
    x.Step("built");
    x.nodes[0].second->Invalidate();
    x.Step("a invalidated");
    x.Tick(4s, "4 s");
    x.Tick(1s, "5 s");
    x.Tick(0s, "again");
    // a second visit of a node whose delay has started starts nothing
    auto s1 = x.Compute("s1");
    auto s1b = x.Compute("s1b");
    x.Compute("w", {s1, s1b}, 5s);
    s1->Invalidate();
    x.Step("s1");
    x.now += 1s;
    s1b->Invalidate();
    x.Step("s1b");
    // never: flagged, no timer; a bare has_delay node: a timer only under a registry default
    auto src = x.Compute("src");
    x.Compute("never", {src}, ns::max());
    auto h = x.r.BeginCompute("hd", true);
    CHECK(x.r.AddUsed(*h, *src) == FGI_USED_ADDED && x.r.SetOutput(*h));
    x.Track("hd", h);
    src->Invalidate();
    x.Step("src");
    x.Tick(2s, "2 s later");
    x.Tick(10s, "w's timer");
}

static void displacement_with_delay(Run& x) {
    auto d1 = x.Compute("d", {}, 3s);
    x.nodes.back().first = "d/1";
    x.Compute("top", {d1});
    auto d2 = x.Track("d/2", x.r.BeginCompute("d", 3s));
    CHECK(d1->Handle() != d2->Handle() && d1->Handle() >= 64);
    x.Step("d displaced");
    x.Tick(3s, "3 s");
    CHECK(x.r.Get("d") == d2);
    // a node whose timer is already running keeps it when it is displaced
    CHECK(x.r.SetOutput(*d2));
    auto s = x.Compute("s");
    auto w = x.Compute("w", {s}, 4s);
    s->Invalidate();
    x.Step("s");
    x.now += 1s;
    x.Track("w/2", x.r.BeginCompute("w"));
    CHECK(w->Handle() >= 64);
    x.Step("w displaced");
    x.Tick(2s, "3 s after the visit");
    x.Tick(1s, "4 s after the visit");
}

// the node's Invalidated handler disposes the host timer; the engine drops the entry when it comes due
static void direct_invalidation_before_timer(Run& x) {
    chain(x);
    x.nodes[0].second->Invalidate();
    x.Step("a");
    x.now += 2s;
    x.nodes[3].second->Invalidate(true);
    x.Step("d at once", false);
    x.Tick(10s, "past d's due time");
}

static void two_due_together(Run& x) {
    auto s = x.Compute("s");
    auto a = x.Compute("x", {s}, 5s);
    auto b = x.Compute("y", {s}, 3s);
    x.Compute("tx", {a});
    x.Compute("ty", {b});
    s->Invalidate();
    x.Step("s");
    x.Tick(5s, "both due");
    x.trace.push_back("roots " + std::to_string(x.r.LastWave().roots) + " v_inv " + std::to_string(x.r.LastWave().v_inv));
    // timers also run at the start of a registry call
    auto s2 = x.Compute("s2");
    x.Compute("z", {s2}, 1s);
    s2->Invalidate();
    x.Step("s2");
    x.now += 1s;
    CHECK(x.r.Get("z") == nullptr);
    x.Step("Get(z)");
}

// a timer's wave starts the next timer: p (1 s) -> q (2 s) -> leaf
static void cascading(Run& x) {
    auto s = x.Compute("s");
    auto p = x.Compute("p", {s}, 1s);
    auto q = x.Compute("q", {p}, 2s);
    x.Compute("leaf", {q});
    s->Invalidate();
    x.Step("s");
    x.Tick(1s, "p fires, q starts");
    x.Tick(1s, "1 s of q's 2");
    x.Tick(1s, "q fires");
}

static void async_scope(Run& x) {
    chain(x);
    {
        auto sc = x.r.InvalidateAsync();
        x.nodes[0].second->Invalidate();
    }
    x.trace.push_back("pending waves " + std::to_string(x.r.PendingWaves()));
    x.r.Complete(x.r.LastTicket());
    x.Step("completed");
    x.Tick(5s, "5 s");
}

// bulk-registered nodes under a registry default: delayed leaves 1, 11, 21, ... of `leaves` under hub 0
static void hub_graph(uint32_t leaves) {
    const uint32_t n = leaves + 1;
    std::vector<uint32_t> slot(n), flags(n, FGI_CONSISTENT), used(leaves, 0u), dep(leaves);
    std::vector<uint64_t> ver(n), tag(leaves);
    for (uint32_t i = 0; i < n; ++i) {
        slot[i] = i;
        ver[i] = 2ull * i + 1;
        if (i && i % 10 == 1) flags[i] |= FGI_F_HAS_DELAY;
    }
    for (uint32_t i = 0; i < leaves; ++i) {
        dep[i] = i + 1;
        tag[i] = ver[i + 1];
    }
    struct Side {
        Run run;
        uint64_t ids = 0, sum = 0;
        std::vector<uint64_t> v;
        std::vector<uint32_t> f;
        Side(bool device, uint32_t n) : run(device, n, 3s), v(n + 1024), f(n + 1024) {
            run.r.OnInvalidatedBatch = [this](const uint32_t* ids_, size_t k) {
                ids += k;
                for (size_t i = 0; i < k; ++i) sum += ids_[i];
            };
        }
        void Dump() { CHECK(fgi_dump_states(run.r.Graph(), v.data(), f.data()) == FGI_OK); }
    };
    Side host(false, n), dev(true, n);
    for (Side* s : {&host, &dev}) {
        CHECK(fgi_register_nodes(s->run.r.Graph(), n, slot.data(), ver.data(), flags.data()) == FGI_OK);
        CHECK(fgi_load_edges(s->run.r.Graph(), leaves, used.data(), dep.data(), tag.data()) == FGI_OK);
    }
    auto agree = [&](const char* what, uint64_t want_ids) {
        host.Dump();
        dev.Dump();
        CHECK(host.v == dev.v && host.f == dev.f);
        CHECK(host.ids == want_ids && dev.ids == want_ids && host.sum == dev.sum);
        CHECK(host.run.r.PendingTimers() == dev.run.r.PendingTimers());
        std::printf("hub graph, %s: %llu handler ids, %zu pending\n", what, (unsigned long long)dev.ids, dev.run.r.PendingTimers());
    };
    const uint32_t delayed = (leaves + 9) / 10;
    for (Side* s : {&host, &dev}) s->run.r.InvalidateSlots({0});
    agree("hub wave", 1 + leaves - delayed);
    CHECK(dev.run.r.PendingTimers() == delayed);
    for (Side* s : {&host, &dev}) {
        s->run.now += 2s;
        CHECK(s->run.r.RunDueTimers() == 0);
    }
    agree("2 s", 1 + leaves - delayed);
    for (Side* s : {&host, &dev}) {
        s->run.now += 1s;
        CHECK(s->run.r.RunDueTimers() == delayed);
    }
    agree("3 s", 1 + leaves);
    CHECK(dev.run.r.PendingTimers() == 0);
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

// --bench: 10,000 hubs x 1,000 leaves, every 10th leaf delayed (8 s, the registry's default), bulk-registered.
// Per repeat and path (host timers, engine timers, alternating, a fresh registry each): a scope over hubs
// [0, 1000) at 0 s, a scope over the other 9,000 hubs at 5 s (900,000 leaves flagged), then at 8 s RunDueTimers
// with 1,000,000 timers pending and the first 100,000 due.
//   ready_ms: the 9,000-hub scope from the wave's return to the registry being ready for its next call: the
//             call less the wave's own span, plus the RunDueTimers the next call starts with (nothing due)
//   due_ms:   RunDueTimers at 8 s, its wave and the fan-out of its 100,000 ids included
static void bench(int reps) {
    const uint32_t H = 10000, L = 1000, N = H + H * L;
    std::vector<uint32_t> slot(N), flags(N, FGI_CONSISTENT), used(N - H), dep(N - H);
    std::vector<uint64_t> ver(N), tag(N - H);
    for (uint32_t i = 0; i < N; ++i) {
        slot[i] = i;
        ver[i] = 2ull * i + 1;
        if (i >= H && (i - H) % 10 == 0) flags[i] |= FGI_F_HAS_DELAY;
    }
    for (uint32_t k = 0; k < N - H; ++k) {
        used[k] = k / L;
        dep[k] = H + k;
        tag[k] = ver[H + k];
    }
    std::vector<uint32_t> first(1000), rest(H - 1000);
    for (uint32_t h = 0; h < H; ++h) (h < 1000 ? first[h] : rest[h - 1000]) = h;
    std::vector<double> ready[2], due[2], scope[2], wave[2], kern;
    for (int rep = 0; rep < reps + 1; ++rep) {   // the first repeat warms up
        for (int path = 0; path < 2; ++path) {
            Run x(path == 1, N, 8s);
            x.r.WaveOutput = 2;
            CHECK(fgi_register_nodes(x.r.Graph(), N, slot.data(), ver.data(), flags.data()) == FGI_OK);
            CHECK(fgi_load_edges(x.r.Graph(), N - H, used.data(), dep.data(), tag.data()) == FGI_OK);
            x.r.InvalidateSlots(first);
            CHECK(x.r.RunDueTimers() == 0);
            x.now += 5s;
            auto t0 = std::chrono::steady_clock::now();
            x.r.InvalidateSlots(rest);
            const double call_ms = ms_since(t0), wave_ms = x.r.LastWave().total_ms;
            t0 = std::chrono::steady_clock::now();
            CHECK(x.r.RunDueTimers() == 0);
            const double next_ms = ms_since(t0);
            CHECK(x.r.PendingTimers() == (size_t)H * L / 10);
            x.now += 3s;
            t0 = std::chrono::steady_clock::now();
            const size_t fired = x.r.RunDueTimers();
            const double d_ms = ms_since(t0);
            CHECK(fired == 1000u * L / 10 && x.r.PendingTimers() == 9000u * L / 10);
            if (rep == 0) continue;
            ready[path].push_back(call_ms - wave_ms + next_ms);
            scope[path].push_back(call_ms);
            wave[path].push_back(wave_ms);
            due[path].push_back(d_ms);
            if (path == 1) {
                fgi_timer_stats st{};
                CHECK(fgi_timers_stats_get(x.r.Graph(), &st) == FGI_OK);
                kern.push_back(st.last_kernel_ms);
            }
        }
    }
    auto runs = [](const std::vector<double>& v) {
        std::string s = "[";
        for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
        return s + "]";
    };
    std::printf("DEVICE_TIMERS {\"workload\": \"10000 hubs x 1000 leaves, every 10th leaf delayed (8 s default), bulk-registered\", \"reps\": %d", reps);
    for (int path = 0; path < 2; ++path)
        std::printf(", \"%s\": {\"ready_ms\": {\"median\": %.3f, \"spread\": %.3f, \"runs\": %s}, "
                    "\"run_due_ms\": {\"median\": %.3f, \"spread\": %.3f, \"runs\": %s}, "
                    "\"scope_call_ms\": {\"median\": %.3f}, \"wave_span_ms\": {\"median\": %.3f}}",
                    path ? "device_timers_on" : "device_timers_off", median(ready[path]), spread(ready[path]), runs(ready[path]).c_str(),
                    median(due[path]), spread(due[path]), runs(due[path]).c_str(), median(scope[path]), median(wave[path]));
    std::printf(", \"due_pass_kernel_ms\": {\"median\": %.3f, \"spread\": %.3f}}\n", median(kern), spread(kern));
}

int main(int argc, char** argv) {
    try {
        if (argc > 1 && std::strcmp(argv[1], "--bench") == 0) {
            bench(argc > 2 ? std::max(1, std::atoi(argv[2])) : 5);
            std::printf("%d/%d checks passed\n", g_checks - g_fail, g_checks);
            return g_fail ? 1 : 0;
        }
        both("invalidation_delay_then_timer", 64, 0ns, invalidation_delay_then_timer, 20);
        both("the same under a default delay", 64, 2s, invalidation_delay_then_timer, 20);
        both("displacement_with_delay", 64, 0ns, displacement_with_delay, 10);
        both("direct_invalidation_before_timer", 64, 0ns, direct_invalidation_before_timer, 6);
        both("two_due_together", 64, 0ns, two_due_together, 8);
        both("cascading", 64, 0ns, cascading, 8);
        both("async_scope", 64, 0ns, async_scope, 6);
        hub_graph(10000);
    } catch (const FgiError& e) {
        std::fprintf(stderr, "FgiError %d: %s\n", (int)e.status, e.what());
        return 2;
    }
    std::printf("%d/%d checks passed\n", g_checks - g_fail, g_checks);
    return g_fail ? 1 : 0;
}
