// test_view.cpp — the host mirror's state reads over the engine's host-memory state view (C-ABI 0.6):
// IComputed.ConsistencyState is a plain field in the reference (Computed.cs:46), read on every cache hit
// (ComputedExt.TryUseExisting, Internal/ComputedExt.cs:13-22). The mirror reads it from the view: a load, no
// engine call. Checked here: after every wave of a small registry each Computed's Flags() equals what
// fgi_get_state reports for its handle; with no wave pending, state reads and TryUseExisting hits make no
// engine call (EngineCalls); and the hit throughput on one thread is printed (no threshold).
// Needs a GPU; run by tests/test_gpu_host_view.py.
#include <chrono>
#include <cstdio>
#include <string>
#include <vector>

#include "fusion.hpp"

using namespace fusion;
using namespace std::chrono_literals;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        ++g_checks;                                                                       \
        if (!(cond)) {                                                                    \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                                     \
        }                                                                                 \
    } while (0)

static std::shared_ptr<Computed> Compute(ComputedRegistry& r, const std::string& in,
                                         std::initializer_list<std::shared_ptr<Computed>> deps = {},
                                         std::chrono::nanoseconds delay = 0ns) {
    auto c = r.BeginCompute(in, delay);
    for (auto& d : deps) CHECK(r.AddUsed(*c, *d) == FGI_USED_ADDED);
    CHECK(r.SetOutput(*c));
    return c;
}

// every node's Flags() against the engine's own report for its handle
static void check_all(ComputedRegistry& r, const std::vector<std::shared_ptr<Computed>>& nodes, const char* what) {
    for (const auto& c : nodes) {
        const uint32_t h = c->Handle();
        uint64_t v = 0;
        uint32_t f = 0;
        CHECK(fgi_get_state(r.Graph(), 1, &h, &v, &f) == FGI_OK);
        const uint32_t want = v == c->Version() ? f : FGI_INVALIDATED;   // a node that is gone reads as Invalidated
        const uint32_t got = c->Flags();
        if (got != want) std::fprintf(stderr, "%s: %s handle %u: Flags() %u, fgi_get_state %u\n", what, c->Input().c_str(), h, got, want);
        CHECK(got == want);
        CHECK(c->IsConsistent() == ((want & FGI_STATE_MASK) == FGI_CONSISTENT));
        CHECK((uint32_t)c->State() == (want & FGI_STATE_MASK));
    }
}

// a -> b -> c -> d (delay 5 s) -> e, a Computing node p that used c, and an unrelated pair x -> y
static void scenario_waves() {
    ComputedRegistry r(64);
    ComputedRegistry::TimePoint now{};
    r.Clock = [&now] { return now; };
    auto a = Compute(r, "a");
    auto b = Compute(r, "b", {a});
    auto c = Compute(r, "c", {b});
    auto d = Compute(r, "d", {c}, 5s);
    auto e = Compute(r, "e", {d});
    auto x = Compute(r, "x");
    auto y = Compute(r, "y", {x});
    auto p = r.BeginCompute("p");   // stays Computing
    CHECK(r.AddUsed(*p, *c) == FGI_USED_ADDED);
    std::vector<std::shared_ptr<Computed>> all{a, b, c, d, e, x, y, p};
    check_all(r, all, "built");
    CHECK(a->IsConsistent() && p->State() == ConsistencyState::Computing);
    a->Invalidate();   // depth 3: a, b, c invalidated; d only flagged (its timer), p gains InvalidateOnSetOutput
    check_all(r, all, "wave 1");
    CHECK(a->IsInvalidated() && c->IsInvalidated() && d->IsConsistent() && e->IsConsistent());
    CHECK((d->Flags() & FGI_F_INVALIDATION_DELAY_STARTED) && (p->Flags() & FGI_F_INVALIDATE_ON_SET_OUTPUT));
    CHECK(x->IsConsistent() && y->IsConsistent());
    now += 5s;
    CHECK(r.RunDueTimers() == 1);   // d's timer: Invalidate(true), e follows
    check_all(r, all, "timer wave");
    CHECK(d->IsInvalidated() && e->IsInvalidated());
    {   // a scope's batched wave
        auto scope = r.Invalidate();
        x->Invalidate();
    }
    check_all(r, all, "scope wave");
    CHECK(x->IsInvalidated() && y->IsInvalidated());
    CHECK(r.SetOutput(*p));   // InvalidateOnSetOutput: invalidated at once
    check_all(r, all, "set_output");
    CHECK(p->IsInvalidated());
    // a displaced node: the slot's new object owns the handle, the old one is gone (decided on the host)
    auto a2 = Compute(r, "a");
    all.push_back(a2);
    check_all(r, all, "recomputed");
    CHECK(a->IsInvalidated() && a2->IsConsistent() && a->Handle() == a2->Handle());
    // a delayed node displaced while Consistent lives on under a detached handle
    auto q = Compute(r, "q", {}, 5s);
    auto q2 = r.BeginCompute("q");
    all.push_back(q);
    all.push_back(q2);
    check_all(r, all, "displaced delayed");
    CHECK(q->Handle() != q2->Handle() && q->IsConsistent() && (q->Flags() & FGI_F_INVALIDATION_DELAY_STARTED));
    // an asynchronous wave: the read completes it first
    auto z = Compute(r, "z");
    auto z2 = Compute(r, "z2", {z});
    all.push_back(z);
    all.push_back(z2);
    {
        auto scope = r.InvalidateAsync();
        z->Invalidate();
    }
    CHECK(r.PendingWaves() == 1);
    CHECK(z2->IsInvalidated() && r.PendingWaves() == 0);
    check_all(r, all, "async wave");
    CHECK((*r.View().seq & 1) == 0);
}

// with no wave pending a state read and a cache hit make no engine call
static void reads_make_no_engine_call() {
    ComputedRegistry r(64);
    auto a = Compute(r, "a");
    auto b = Compute(r, "b", {a});
    int accessed = 0;
    r.OnAccess = [&accessed](Computed&, bool) { ++accessed; };
    const uint64_t before = r.EngineCalls();
    CHECK(before > 0);
    int ok = 0;
    for (int i = 0; i < 1000; ++i) ok += b->IsConsistent() ? 1 : 0;
    for (int i = 0; i < 1000; ++i) ok += r.TryUseExisting("b") ? 1 : 0;
    ok += (a->Flags() == FGI_CONSISTENT) + (a->State() == ConsistencyState::Consistent) + (r.GetExisting("a") == a);
    CHECK(ok == 2003 && accessed == 1001);
    CHECK(r.EngineCalls() == before);
    a->Invalidate();
    CHECK(r.EngineCalls() > before && !r.TryUseExisting("b") && !r.TryUseExisting("a"));
}

// hit throughput on one thread (reported, no threshold)
static void hit_throughput() {
    ComputedRegistry r(1024);
    std::vector<std::shared_ptr<Computed>> nodes;
    std::vector<std::string> names;
    for (int i = 0; i < 256; ++i) {
        names.push_back("svc.Get(" + std::to_string(i) + ")");
        nodes.push_back(Compute(r, names.back()));
    }
    const int iters = 1 << 21;   // 2.1 M
    const uint64_t before = r.EngineCalls();
    uint64_t hits = 0;
    auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < iters; ++i) hits += nodes[i & 255]->IsConsistent() ? 1 : 0;
    const double s1 = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < iters; ++i) hits += r.TryUseExisting(names[i & 255]) ? 1 : 0;
    const double s2 = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    CHECK(hits == 2ull * iters && r.EngineCalls() == before);
    std::printf("hit throughput, one thread, %d iterations each: IsConsistent %.1f M/s, TryUseExisting %.1f M/s\n", iters,
                iters / s1 / 1e6, iters / s2 / 1e6);
}

int main() {
    try {
        scenario_waves();
        reads_make_no_engine_call();
        hit_throughput();
    } catch (const FgiError& e) {
        std::fprintf(stderr, "FgiError %d: %s\n", e.status, e.what());
        return 2;
    }
    if (g_fail) {
        std::fprintf(stderr, "%d of %d checks FAILED\n", g_fail, g_checks);
        return 1;
    }
    std::printf("%d checks passed\n", g_checks);
    return 0;
}
