// test_auto.cpp — auto-invalidation (ComputedOptions.AutoInvalidationDelay / TransientErrorInvalidationDelay,
// StartAutoInvalidation at TrySetOutput) in the engine (ComputedRegistry::DeviceTimers: fgi_timers_auto_open,
// fgi_timers_set_auto_delay, fgi_set_output_ex) against the registry's host timers: every scenario runs on two
// registries, one with DeviceTimers on and one with it off, driven by the same fake clock. The two must agree on
// the handler invocations per node, on State() and Flags() of every node after every step, on what RunDueTimers
// returns, and on PendingTimers() wherever the host path's count is the engine's (the engine keeps the entry of a
// node invalidated before its due time until that time comes).
// Needs a GPU; run by tests/test_gpu_host_auto.py.
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

static ComputedOptions opts(ns delay, ns auto_delay, ns transient = ns::max()) {
    ComputedOptions o;
    o.InvalidationDelay = delay;
    o.AutoInvalidationDelay = auto_delay;
    o.TransientErrorInvalidationDelay = transient;
    return o;
}

// one registry, its clock, the nodes it made (by a label of the test's) and everything observable, in order
struct Run {
    ComputedRegistry r;
    ComputedRegistry::TimePoint now{};
    std::vector<std::pair<std::string, std::shared_ptr<Computed>>> nodes;
    std::vector<std::string> trace;
    Run(bool device, uint32_t n_slots, ns default_auto = ns::max(), ns default_transient = ns::max()) : r(n_slots) {
        r.DeviceTimers = device;
        r.DefaultAutoInvalidationDelay = default_auto;
        r.DefaultTransientErrorInvalidationDelay = default_transient;
        r.Clock = [this] { return now; };
    }
    std::shared_ptr<Computed> Track(const std::string& label, std::shared_ptr<Computed> c) {
        c->OnInvalidated([this, label](Computed&) { trace.push_back("handler " + label); });
        nodes.emplace_back(label, c);
        return c;
    }
    // ComputeMethodFunctionBase.Compute: begin with the node's options, AddUsed each dep, TrySetOutput
    std::shared_ptr<Computed> Compute(const std::string& label, const std::string& in, const ComputedOptions& o,
                                      std::initializer_list<std::shared_ptr<Computed>> deps = {}, bool transient_error = false) {
        auto c = r.BeginCompute(in, o);
        for (auto& d : deps) CHECK(r.AddUsed(*c, *d) == FGI_USED_ADDED);
        CHECK(r.SetOutput(*c, transient_error));
        return Track(label, c);
    }
    std::shared_ptr<Computed> Plain(const std::string& in, std::initializer_list<std::shared_ptr<Computed>> deps = {},
                                    bool transient_error = false) {
        auto c = r.BeginCompute(in);
        for (auto& d : deps) CHECK(r.AddUsed(*c, *d) == FGI_USED_ADDED);
        CHECK(r.SetOutput(*c, transient_error));
        return Track(in, c);
    }
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
    size_t Count(const std::string& line) const { return (size_t)std::count(trace.begin(), trace.end(), line); }
};

using Scenario = std::function<void(Run&)>;

static void both(const char* name, const Scenario& sc, size_t min_lines, ns default_auto = ns::max(),
                 ns default_transient = ns::max()) {
    Run host(false, 64, default_auto, default_transient), dev(true, 64, default_auto, default_transient);
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
    fgi_timer_auto_stats as{};
    CHECK(fgi_timers_auto_stats_get(dev.r.Graph(), &as) == FGI_OK && as.armed_auto >= 1);
    CHECK(fgi_timers_stats_get(host.r.Graph(), &st) == FGI_OK && st.armed == 0);   // never opened there
    std::printf("%s: %zu trace lines agree\n", name, same);
}

// a (auto 5 s) <- b: nothing at 4 s; at 5 s a's timer fires (a never had DelayStarted) and the wave takes b
static void chain(Run& x) {
    auto a = x.Compute("a", "a", opts(0ns, 5s));
    x.Compute("b", "b", opts(0ns, ns::max()), {a});
    x.Step("built");
    x.Tick(4s, "4 s");
    CHECK(x.Count("handler a") == 0);
    x.Tick(1s, "5 s");
    CHECK(x.Count("handler a") == 1 && x.Count("handler b") == 1 && x.Count("fired 1") == 1);
    x.Tick(10s, "later");
}

// "errors retry by themselves": err's output is a transient error, it goes after its TransientErrorInvalidationDelay
// (2 s) and is computed again; its sibling ok (AutoInvalidationDelay = max()) and an error node without a
// transient delay stay
static void transient_retry(Run& x) {
    auto err = x.Compute("err/1", "err", opts(0ns, 60s, 2s), {}, true);
    auto ok = x.Compute("ok", "ok", opts(0ns, ns::max(), 2s));
    x.Compute("err2", "err2", opts(0ns, 7s), {}, true);
    x.Compute("reader", "reader", opts(0ns, ns::max()), {err, ok});
    x.Step("built");
    x.Tick(1s, "1 s");
    x.Tick(1s, "2 s");
    CHECK(x.Count("handler err/1") == 1 && x.Count("handler reader") == 1 && x.Count("handler ok") == 0);
    CHECK(x.r.Get("err") == nullptr && x.r.Get("ok") == ok);
    auto again = x.Compute("err/2", "err", opts(0ns, 60s, 2s));   // the retry succeeds: the auto delay (60 s) holds now
    x.Tick(2s, "4 s");
    CHECK(x.r.Get("err") == again && x.Count("handler err/2") == 0);
    x.Tick(58s, "62 s");
    CHECK(x.Count("handler err/2") == 1 && x.Count("handler ok") == 0 && x.Count("handler err2") == 0);
}

// the registry's defaults serve the nodes begun without ComputedOptions
static void registry_defaults(Run& x) {
    auto p = x.Plain("p");
    auto q = x.Plain("q", {}, true);
    x.Compute("own", "own", opts(0ns, 1s));
    x.Compute("off", "off", opts(0ns, ns::max()));
    x.Step("built");
    x.Tick(1s, "1 s: own");
    x.Tick(1s, "2 s: q (transient default)");
    x.Tick(1s, "3 s: p (auto default)");
    x.Tick(10s, "13 s");
    CHECK(x.Count("handler p") == 1 && x.Count("handler q") == 1 && x.Count("handler own") == 1 && x.Count("handler off") == 0);
    (void)p;
    (void)q;
}

// a Computing node with InvalidationDelay 50 s and AutoInvalidationDelay 2 s that a cascade reached: TrySetOutput
// invalidates it, it survives as Consistent + DelayStarted and gets its delay timer only
static void ioso_with_delay(Run& x) {
    auto s = x.Compute("s", "s", opts(0ns, ns::max()));
    auto n = x.r.BeginCompute("n", opts(50s, 2s));
    CHECK(x.r.AddUsed(*n, *s) == FGI_USED_ADDED);
    x.Track("n", n);
    s->Invalidate();
    x.Step("s invalidated");
    CHECK((n->Flags() & FGI_F_INVALIDATE_ON_SET_OUTPUT) != 0);
    CHECK(x.r.SetOutput(*n));
    x.Step("n set");
    CHECK(n->State() == ConsistencyState::Consistent && (n->Flags() & FGI_F_INVALIDATION_DELAY_STARTED) != 0);
    x.Tick(2s, "2 s");
    CHECK(x.Count("handler n") == 0);
    x.Tick(48s, "50 s");
    CHECK(x.Count("handler n") == 1);
    // (the dev registry's auto-invalidation is open because of n's delay, though nothing was armed by it)
    x.Compute("z", "z", opts(0ns, 1s));
    x.Tick(1s, "z");
}

// AddOrUpdateToEarlier in both directions
static void merge(Run& x) {
    auto s1 = x.Compute("s1", "s1", opts(0ns, ns::max()));
    auto s2 = x.Compute("s2", "s2", opts(0ns, ns::max()));
    x.Compute("X", "X", opts(3s, 100s), {s1});    // auto due 100 s; a visit at 10 s brings it to 13 s
    x.Compute("Y", "Y", opts(50s, 12s), {s2});    // auto due 12 s; a visit at 10 s (60 s) leaves it
    x.now += 10s;
    s1->Invalidate();
    s2->Invalidate();
    x.Step("visited");
    x.Tick(1s, "11 s");
    x.Tick(1s, "12 s: Y, with its delay started");
    CHECK(x.Count("handler Y") == 1 && x.Count("handler X") == 0);
    x.Tick(1s, "13 s: X");
    CHECK(x.Count("handler X") == 1);
    x.Tick(100s, "later");
}

// X (delay 4 s, auto 20 s) displaced at 3 s survives on a detached handle: its auto entry follows it and its delay
// timer joins it (7 s). Z (no delay, auto 20 s) does not survive.
static void displacement(Run& x) {
    auto X = x.Compute("X/1", "X", opts(4s, 20s));
    auto Z = x.Compute("Z/1", "Z", opts(0ns, 20s));
    x.Compute("top", "top", opts(0ns, ns::max()), {X});
    x.now += 3s;
    auto X2 = x.Track("X/2", x.r.BeginCompute("X", opts(4s, 20s)));
    auto Z2 = x.Track("Z/2", x.r.BeginCompute("Z", opts(0ns, 20s)));
    CHECK(X->Handle() >= 64 && Z->IsInvalidated());
    x.Step("displaced", false);
    x.Tick(3s, "6 s", false);
    CHECK(x.Count("handler X/1") == 0);
    x.Tick(1s, "7 s", false);
    CHECK(x.Count("handler X/1") == 1 && x.Count("handler top") == 1);
    CHECK(x.r.SetOutput(*X2) && x.r.SetOutput(*Z2));
    x.Tick(13s, "20 s: the first nodes' due time", false);
    x.Tick(7s, "27 s: the second nodes'");
    CHECK(x.Count("handler X/2") == 1 && x.Count("handler Z/2") == 1);
}

// a fired auto node's wave starts a delayed dependant's timer at that time
static void cascading(Run& x) {
    auto a = x.Compute("a", "a", opts(0ns, 5s));
    auto b = x.Compute("b", "b", opts(4s, ns::max()), {a});
    x.Compute("leaf", "leaf", opts(0ns, ns::max()), {b});
    x.Tick(5s, "a fires, b starts");
    x.Tick(3s, "8 s");
    x.Tick(1s, "9 s: b");
    CHECK(x.Count("handler a") == 1 && x.Count("handler b") == 1 && x.Count("handler leaf") == 1);
}

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : v[v.size() / 2];
}
static double spread(const std::vector<double>& v) {
    return v.empty() ? 0.0 : *std::max_element(v.begin(), v.end()) - *std::min_element(v.begin(), v.end());
}

// --bench N reps: N nodes begun with AutoInvalidationDelay 8 s, then SetOutput of each; ready_ms is the time
// from the first SetOutput until the registry has taken its next call (a RunDueTimers with nothing due).
static void bench(uint32_t n, int reps) {
    std::vector<double> ready[2];
    for (int rep = 0; rep < reps + 1; ++rep) {   // the first repeat warms up
        for (int path = 0; path < 2; ++path) {
            Run x(path == 1, n);
            std::vector<std::shared_ptr<Computed>> c(n);
            for (uint32_t i = 0; i < n; ++i) c[i] = x.r.BeginCompute("n" + std::to_string(i), opts(0ns, 8s));
            const auto t0 = std::chrono::steady_clock::now();
            for (uint32_t i = 0; i < n; ++i) x.r.SetOutput(*c[i]);
            CHECK(x.r.RunDueTimers() == 0);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            CHECK(x.r.PendingTimers() == n);
            if (rep) ready[path].push_back(ms);
        }
    }
    std::printf("AUTO_TIMERS_MIRROR {\"nodes\": %u, \"reps\": %d", n, reps);
    for (int path = 0; path < 2; ++path)
        std::printf(", \"%s\": {\"ready_ms\": {\"median\": %.3f, \"spread\": %.3f}}", path ? "device_timers_on" : "device_timers_off",
                    median(ready[path]), spread(ready[path]));
    std::printf("}\n");
}

int main(int argc, char** argv) {
    try {
        if (argc > 1 && std::strcmp(argv[1], "--bench") == 0) {
            bench(argc > 2 ? (uint32_t)std::max(1, std::atoi(argv[2])) : 100000u, argc > 3 ? std::max(1, std::atoi(argv[3])) : 3);
            std::printf("%d/%d checks passed\n", g_checks - g_fail, g_checks);
            return g_fail ? 1 : 0;
        }
        both("chain", chain, 8);
        both("transient_retry", transient_retry, 12);
        both("registry_defaults", registry_defaults, 10, 3s, 2s);
        both("ioso_with_delay", ioso_with_delay, 10);
        both("merge", merge, 10);
        both("displacement", displacement, 10);
        both("cascading", cascading, 8);
    } catch (const FgiError& e) {
        std::fprintf(stderr, "FgiError %d: %s\n", (int)e.status, e.what());
        return 2;
    }
    std::printf("%d/%d checks passed\n", g_checks - g_fail, g_checks);
    return g_fail ? 1 : 0;
}
