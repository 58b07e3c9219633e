// test_delay.cpp — delayed invalidation through the C++ host mirror (fusion.hpp) over the fgi engine:
// Computed.Invalidate() on a Consistent node with an InvalidationDelay only sets InvalidationDelayStarted
// and starts the node's own timer, which later calls Invalidate(true) (Computed.cs:186-197,
// ComputedExt.cs:10-45). The mirror starts its timers from the flagged set the engine reports for every wave
// (fgi_last_wave_flagged / fgi_wave_wait_flagged) and a fake clock drives them: no threads, no sleeping.
// Needs a GPU; run by tests/test_gpu_host_delay.py.
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

// a clock the test advances
struct FakeClock {
    ComputedRegistry::TimePoint now{};
    void Install(ComputedRegistry& r) {
        r.Clock = [this] { return now; };
    }
};

// ComputeMethodFunctionBase.Compute: begin (with the node's InvalidationDelay), AddUsed each dep, TrySetOutput
static std::shared_ptr<Computed> Compute(ComputedRegistry& r, const std::string& in,
                                         std::initializer_list<std::shared_ptr<Computed>> deps = {},
                                         std::chrono::nanoseconds delay = 0ns) {
    auto c = r.BeginCompute(in, delay);
    for (auto& d : deps) CHECK(r.AddUsed(*c, *d) == FGI_USED_ADDED);
    CHECK(r.SetOutput(*c));
    return c;
}

// the chain a -> b -> c -> d (delay 5 s) -> e with a counter per node
struct Chain {
    std::shared_ptr<Computed> a, b, c, d, e;
    int fa = 0, fb = 0, fc = 0, fd = 0, fe = 0;
    explicit Chain(ComputedRegistry& r) {
        a = Compute(r, "a");
        b = Compute(r, "b", {a});
        c = Compute(r, "c", {b});
        d = Compute(r, "d", {c}, 5s);
        e = Compute(r, "e", {d});
        a->OnInvalidated([this](Computed&) { ++fa; });
        b->OnInvalidated([this](Computed&) { ++fb; });
        c->OnInvalidated([this](Computed&) { ++fc; });
        d->OnInvalidated([this](Computed&) { ++fd; });
        e->OnInvalidated([this](Computed&) { ++fe; });
    }
};

// TimeoutsTest-style InvalidationDelay (Computed.cs:186-197 -> ComputedExt.Invalidate(TimeSpan)): the delayed
// node sits at cascade depth 3, where only the engine sees the visit
static void invalidation_delay_then_timer() {
    ComputedRegistry r(64);
    FakeClock clk;
    clk.Install(r);
    Chain ch(r);
    CHECK(r.PendingTimers() == 0);
    ch.a->Invalidate();
    CHECK(ch.fa == 1 && ch.fb == 1 && ch.fc == 1 && ch.fd == 0 && ch.fe == 0);
    CHECK(r.PendingTimers() == 1);
    CHECK(ch.d->IsConsistent() && (ch.d->Flags() & FGI_F_INVALIDATION_DELAY_STARTED) && ch.e->IsConsistent());
    clk.now += 4s;
    CHECK(r.RunDueTimers() == 0 && ch.fd == 0 && ch.fe == 0 && r.PendingTimers() == 1);
    clk.now += 1s;
    CHECK(r.RunDueTimers() == 1);
    CHECK(ch.fd == 1 && ch.fe == 1 && r.PendingTimers() == 0);
    CHECK(ch.d->IsInvalidated() && ch.e->IsInvalidated());
    CHECK(r.RunDueTimers() == 0 && ch.fd == 1 && ch.fe == 1);
    // a second visit of a node whose delay has started starts nothing
    auto s1 = Compute(r, "s1");
    auto s1b = Compute(r, "s1b");
    auto w = Compute(r, "w", {s1, s1b}, 5s);
    s1->Invalidate();
    CHECK(r.PendingTimers() == 1);
    clk.now += 1s;
    s1b->Invalidate();
    CHECK(r.PendingTimers() == 1 && w->IsConsistent());
    // never (TimeSpan.MaxValue, ComputedExt.cs:12): flagged, no timer; a bare has_delay node: no timer
    // without a registry default
    auto src = Compute(r, "src");
    auto n = Compute(r, "never", {src}, std::chrono::nanoseconds::max());
    auto h = r.BeginCompute("hd", true);
    CHECK(r.AddUsed(*h, *src) == FGI_USED_ADDED && r.SetOutput(*h));
    src->Invalidate();
    CHECK((n->Flags() & FGI_F_INVALIDATION_DELAY_STARTED) && (h->Flags() & FGI_F_INVALIDATION_DELAY_STARTED));
    CHECK(r.PendingTimers() == 1);
    // the same bare node under a registry default gets one
    r.DefaultInvalidationDelay = 2s;
    auto s2 = Compute(r, "s2");
    auto h2 = r.BeginCompute("hd2", true);
    CHECK(r.AddUsed(*h2, *s2) == FGI_USED_ADDED && r.SetOutput(*h2));
    s2->Invalidate();
    CHECK(r.PendingTimers() == 2);
    clk.now += 2s;
    CHECK(r.RunDueTimers() == 1 && h2->IsInvalidated() && r.PendingTimers() == 1);
}

// ComputedRegistry.Register (ComputedRegistry.cs:83-97): BeginCompute on a delayed Consistent node detaches
// it and starts its timer; the timer invalidates the detached node and its dependants, not the new computation
static void displacement_with_delay() {
    ComputedRegistry r(64);
    FakeClock clk;
    clk.Install(r);
    auto d1 = Compute(r, "d", {}, 3s);
    auto top = Compute(r, "top", {d1});
    int f1 = 0, ft = 0, f2 = 0;
    d1->OnInvalidated([&](Computed&) { ++f1; });
    top->OnInvalidated([&](Computed&) { ++ft; });
    auto d2 = r.BeginCompute("d", 3s);
    d2->OnInvalidated([&](Computed&) { ++f2; });
    CHECK(d1->Handle() != d2->Handle() && d1->Handle() >= 64);
    CHECK(d1->IsConsistent() && (d1->Flags() & FGI_F_INVALIDATION_DELAY_STARTED) && top->IsConsistent());
    CHECK(r.PendingTimers() == 1 && f1 == 0 && ft == 0);
    clk.now += 3s;
    CHECK(r.RunDueTimers() == 1);
    CHECK(f1 == 1 && ft == 1 && f2 == 0 && r.PendingTimers() == 0);
    CHECK(d1->IsInvalidated() && top->IsInvalidated() && d2->State() == ConsistencyState::Computing);
    CHECK(r.Get("d") == d2);
    // a node whose timer is already running keeps it when it is displaced
    CHECK(r.SetOutput(*d2));
    auto s = Compute(r, "s");
    auto w = Compute(r, "w", {s}, 4s);
    int fw = 0;
    w->OnInvalidated([&](Computed&) { ++fw; });
    s->Invalidate();
    CHECK(r.PendingTimers() == 1);
    clk.now += 1s;
    auto w2 = r.BeginCompute("w");
    CHECK(r.PendingTimers() == 1 && w->IsConsistent() && w->Handle() >= 64);
    clk.now += 2s;
    CHECK(r.RunDueTimers() == 0);
    clk.now += 1s;   // 4 s after the first visit, not after the displacement
    CHECK(r.RunDueTimers() == 1 && fw == 1 && w->IsInvalidated() && w2->State() == ConsistencyState::Computing);
}

// ComputedExt.cs:38-45: the node's Invalidated handler disposes the timer
static void direct_invalidation_before_timer() {
    ComputedRegistry r(64);
    FakeClock clk;
    clk.Install(r);
    Chain ch(r);
    ch.a->Invalidate();
    CHECK(r.PendingTimers() == 1);
    clk.now += 2s;
    ch.d->Invalidate(true);
    CHECK(ch.fd == 1 && ch.fe == 1 && r.PendingTimers() == 0);
    clk.now += 10s;
    CHECK(r.RunDueTimers() == 0 && ch.fd == 1 && ch.fe == 1);
}

// due together: one wave, immediately = true for the batch
static void two_due_together() {
    ComputedRegistry r(64);
    FakeClock clk;
    clk.Install(r);
    auto s = Compute(r, "s");
    auto x = Compute(r, "x", {s}, 5s);
    auto y = Compute(r, "y", {s}, 3s);
    auto tx = Compute(r, "tx", {x});
    auto ty = Compute(r, "ty", {y});
    int fired = 0;
    for (auto* c : {x.get(), y.get(), tx.get(), ty.get()}) c->OnInvalidated([&](Computed&) { ++fired; });
    s->Invalidate();
    CHECK(r.PendingTimers() == 2 && fired == 0);
    clk.now += 5s;
    CHECK(r.RunDueTimers() == 2);
    CHECK(r.LastWave().roots == 2 && r.LastWave().v_inv == 4 && fired == 4 && r.PendingTimers() == 0);
    // timers also run at the start of a registry call
    auto s2 = Compute(r, "s2");
    auto z = Compute(r, "z", {s2}, 1s);
    s2->Invalidate();
    CHECK(r.PendingTimers() == 1);
    clk.now += 1s;
    CHECK(r.Get("z") == nullptr && z->IsInvalidated() && r.PendingTimers() == 0);
}

// the same chain through an asynchronous scope: the wave's flagged set is read when the wave is completed
static void async_scope() {
    ComputedRegistry r(64);
    FakeClock clk;
    clk.Install(r);
    Chain ch(r);
    {
        auto sc = r.InvalidateAsync();
        ch.a->Invalidate();
    }
    CHECK(r.PendingWaves() == 1 && r.PendingTimers() == 0 && ch.fa == 0);
    r.Complete(r.LastTicket());
    CHECK(ch.fa == 1 && ch.fb == 1 && ch.fc == 1 && ch.fd == 0 && ch.fe == 0 && r.PendingTimers() == 1);
    clk.now += 5s;
    CHECK(r.RunDueTimers() == 1 && ch.fd == 1 && ch.fe == 1 && r.PendingTimers() == 0);
}

// an inner InvalidateAsync() inside an outer Invalidate() does not make the outer scope's flush asynchronous
static void nested_scopes() {
    ComputedRegistry r(64);
    auto a = Compute(r, "a");
    auto b = Compute(r, "b");
    int fired = 0;
    a->OnInvalidated([&](Computed&) { ++fired; });
    b->OnInvalidated([&](Computed&) { ++fired; });
    {
        auto outer = r.Invalidate();
        a->Invalidate();
        {
            auto inner = r.InvalidateAsync();
            b->Invalidate();
        }
        CHECK(fired == 0 && r.PendingWaves() == 0);
    }
    CHECK(fired == 2 && r.PendingWaves() == 0 && r.LastWave().roots == 2);
    // and an outermost InvalidateAsync() still flushes asynchronously, nested scopes included
    auto c = Compute(r, "c");
    auto d = Compute(r, "d");
    {
        auto outer = r.InvalidateAsync();
        c->Invalidate();
        {
            auto inner = r.Invalidate();
            d->Invalidate();
        }
    }
    CHECK(r.PendingWaves() == 1);
    r.CompletePending();
    CHECK(c->IsInvalidated() && d->IsInvalidated());
}

int main() {
    try {
        invalidation_delay_then_timer();
        displacement_with_delay();
        direct_invalidation_before_timer();
        two_due_together();
        async_scope();
        nested_scopes();
    } catch (const FgiError& e) {
        std::fprintf(stderr, "FgiError %d: %s\n", (int)e.status, e.what());
        return 2;
    }
    std::printf("%d/%d checks passed\n", g_checks - g_fail, g_checks);
    return g_fail ? 1 : 0;
}
