// fusion.cpp — implementation of the host-layer mirror (see fusion.hpp).
#include "fusion.hpp"

#include <algorithm>
#include <chrono>
#include <thread>

namespace fusion {

namespace {
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kParallelMin = 1u << 16;   // ids below this fan out on the dispatcher thread

// every call into the engine is counted (ComputedRegistry::EngineCalls): in the registry's own methods,
// and in Computed's through its registry
#define FGI_CALL(fn, ...) (++calls_, fn(__VA_ARGS__))
#define FGI_RCALL(fn, ...) (++reg_->calls_, fn(__VA_ARGS__))

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

// ---- InvalidatedHandlerSet ------------------------------------------------------------------------
void InvalidatedHandlerSet::Add(const InvalidatedHandler& h) {
    if (!h) return;
    if (set_) {
        set_->insert(h);
        return;
    }
    for (const auto& x : list_)
        if (x == h) return;
    if (list_.size() < ListSize) {
        list_.push_back(h);
        return;
    }
    set_ = std::make_unique<std::unordered_set<InvalidatedHandler>>(list_.begin(), list_.end());
    set_->insert(h);
    list_.clear();
}

void InvalidatedHandlerSet::Remove(const InvalidatedHandler& h) {
    if (!h) return;
    if (set_) {
        set_->erase(h);
        return;
    }
    auto it = std::find(list_.begin(), list_.end(), h);
    if (it != list_.end()) list_.erase(it);
}

void InvalidatedHandlerSet::Invoke(Computed& c) const {
    if (set_) {
        for (const auto& h : *set_) (*h)(c);
        return;
    }
    for (const auto& h : list_) (*h)(c);
}

// ---- registry -------------------------------------------------------------------------------------
ComputedRegistry::ComputedRegistry(uint32_t n_slots, uint32_t n_detached, int device) : n_slots_(n_slots) {
    fgi_config cfg{};
    cfg.struct_size = sizeof(cfg);
    cfg.device = device;
    cfg.n_slots = n_slots;
    cfg.n_detached = n_detached;
    cfg.world = 1;
    fgi_status s = FGI_CALL(fgi_create, &cfg, &g_);
    if (s != FGI_OK) throw FgiError(s, "fgi_create failed (no GPU?)");
    // the nodes' states are read from host memory the engine keeps current (Computed::Flags)
    view_.struct_size = sizeof(view_);
    s = FGI_CALL(fgi_state_view_open, g_, &view_);
    if (s != FGI_OK) {
        const std::string why = fgi_last_error(g_);
        fgi_destroy(g_);
        throw FgiError(s, "fgi_state_view_open: " + why);
    }
    n_handles_ = n_slots + n_detached;
    current_.resize(n_slots);
    has_obj_.assign(n_handles_, 0);
}

ComputedRegistry::~ComputedRegistry() {
    if (dev_buf_) fgi_free_pinned(dev_buf_);
    FGI_CALL(fgi_destroy, g_);
}

void ComputedRegistry::Check(fgi_status s, const char* what) const {
    if (s != FGI_OK) throw FgiError(s, std::string(what) + ": " + FGI_CALL(fgi_last_error, g_));
}

uint32_t ComputedRegistry::SlotOf(const std::string& input, bool create) {
    auto it = slots_.find(input);
    if (it != slots_.end()) return it->second;
    if (!create) return FGI_NONE;
    if (slots_.size() >= n_slots_) throw FgiError(FGI_ECAPACITY, "registry is full");
    const uint32_t s = (uint32_t)slots_.size();
    slots_.emplace(input, s);
    return s;
}

// LTagVersionGenerator.NextVersion (LTagVersionGenerator.cs:13-20): a fresh positive tag != current
LTag ComputedRegistry::NextVersion(LTag current) {
    do {
        ltag_ = ((ltag_ + 1) & ((1ull << 55) - 1));
    } while (ltag_ == 0 || ltag_ == current);
    return ltag_;
}

uint32_t* ComputedRegistry::IdsBuffer(uint64_t need) {
    if (need > ids_cap_) {
        const uint64_t cap = std::max<uint64_t>(need, ids_cap_ + ids_cap_ / 2);
        ids_.reset(new uint32_t[cap]);   // default-initialised: no zero-fill
        ids_cap_ = cap;
    }
    return ids_.get();
}

std::shared_ptr<Computed> ComputedRegistry::Get(const std::string& input) {
    Sync();
    const uint32_t s = SlotOf(input, false);
    if (s == FGI_NONE || !current_[s]) return nullptr;
    const ConsistencyState st = current_[s]->State();
    if (st == ConsistencyState::Invalidated) return nullptr;   // unregistered on invalidation
    return current_[s];
}

void ComputedRegistry::MoveSubs(uint32_t from, uint32_t to) {
    if (from >= sub_head_.size() || sub_head_[from] == kNone) return;
    if (to >= sub_head_.size()) sub_head_.resize(n_handles_, kNone);
    sub_head_[to] = sub_head_[from];
    sub_head_[from] = kNone;
}

// the options of a node begun without ComputedOptions: the registry's auto-invalidation defaults
ComputedOptions ComputedRegistry::DefaultOptions(std::chrono::nanoseconds delay) const {
    ComputedOptions o;
    o.InvalidationDelay = delay;
    o.AutoInvalidationDelay = DefaultAutoInvalidationDelay;
    o.TransientErrorInvalidationDelay = DefaultTransientErrorInvalidationDelay;
    return o;
}

std::shared_ptr<Computed> ComputedRegistry::BeginCompute(const std::string& input, bool has_delay) {
    return BeginComputeImpl(input, has_delay, DefaultOptions(std::chrono::nanoseconds::zero()));
}

std::shared_ptr<Computed> ComputedRegistry::BeginCompute(const std::string& input, const ComputedOptions& options) {
    return BeginComputeImpl(input, options.InvalidationDelay != std::chrono::nanoseconds::zero(), options);
}

// an auto-invalidation delay in the engine's ticks; 0: off (max(), or <= 0: "at once" is not built)
static uint64_t AutoTicks(std::chrono::nanoseconds d) {
    using ns = std::chrono::nanoseconds;
    return d == ns::max() || d <= ns::zero() ? 0ull : (uint64_t)d.count();
}

std::shared_ptr<Computed> ComputedRegistry::BeginComputeImpl(const std::string& input, bool has_delay,
                                                             const ComputedOptions& options) {
    const std::chrono::nanoseconds delay = options.InvalidationDelay;
    Sync();
    const uint32_t s = SlotOf(input, true);
    auto c = std::make_shared<Computed>();
    c->reg_ = this;
    c->input_ = input;
    c->slot_ = s;
    c->handle_ = s;
    c->version_ = NextVersion(current_[s] ? current_[s]->version_ : 0);
    c->delay_ = delay;
    c->auto_delay_ = options.AutoInvalidationDelay;
    c->transient_delay_ = options.TransientErrorInvalidationDelay;
    const uint8_t hd = has_delay ? 1 : 0;
    uint32_t detached = FGI_NONE;
    fgi_wave_stats ws{};
    Check(FGI_CALL(fgi_begin_compute, g_, 1, &s, &c->version_, &hd, &detached, &ws), "fgi_begin_compute");
    StartTimers(0);   // the delayed nodes the displacement cascade reached
    if (dev_timers_) {
        // the engine moved or armed the displaced node's timer and gave its detached handle the slot's delay;
        // the slot's delay is the new node's from here on (one call, and only when it changes)
        using ns = std::chrono::nanoseconds;
        const uint64_t d = delay == ns::max() ? FGI_TIMER_NEVER : delay <= ns::zero() ? 0ull : (uint64_t)delay.count();
        if (slot_delay_[s] != d) {
            Check(FGI_CALL(fgi_timers_set_delay, g_, 1, &s, &d), "fgi_timers_set_delay");
            slot_delay_[s] = d;
        }
        // ... and so are its auto-invalidation delays, once any node has had one
        const uint64_t a = AutoTicks(c->auto_delay_), t = AutoTicks(c->transient_delay_);
        if (a || t) EnsureAuto();
        if (dev_auto_ && (slot_auto_[s] != a || slot_transient_[s] != t)) {
            Check(FGI_CALL(fgi_timers_set_auto_delay, g_, 1, &s, &a, &t), "fgi_timers_set_auto_delay");
            slot_auto_[s] = a;
            slot_transient_[s] = t;
        }
        if (detached != FGI_NONE) maybe_armed_ = true;
    }
    auto old = current_[s];
    if (detached != FGI_NONE) {   // displaced but alive (Computing / delayed): its handle moves
        if (old) {
            old->handle_ = detached;
            detached_[detached] = old;
            has_obj_[detached] = 1;
            // a delayed node displaced while Consistent is flagged under its new handle (the call's flagged
            // set does not list its slot, which names the new node now): its timer starts here, or follows
            // it if it was already running
            auto it = timers_.find(s);
            if (dev_timers_) {
                // (the engine's move kernel did the same on its table)
            } else if (it != timers_.end() && it->second.version == old->version_) {
                const bool was_auto = it->second.is_auto;
                timers_[detached] = it->second;
                timers_.erase(s);
                // an auto entry of a node whose delay the displacement has just started: the delay timer joins
                // it and the earlier due time stays (ComputedRegistry.cs:91-96 -> Computed.cs:186-197)
                const uint32_t f = was_auto ? fgi_view_flags(&view_, detached) : 0u;
                if ((f & FGI_STATE_MASK) == FGI_CONSISTENT && (f & FGI_F_INVALIDATION_DELAY_STARTED))
                    StartTimer(detached, old->version_, old->delay_);
            } else {
                const uint32_t f = fgi_view_flags(&view_, detached);   // the handle names the old node alone
                if ((f & FGI_STATE_MASK) == FGI_CONSISTENT && (f & FGI_F_INVALIDATION_DELAY_STARTED))
                    StartTimer(detached, old->version_, old->delay_);
            }
        }
        if (!DeviceFanout) MoveSubs(s, detached);   // the replicas follow the old node (the engine moves its own)
    } else if (old) {
        old->gone_ = true;   // the slot names the new node from here on (its handlers may still read its state)
    }
    // the displacement cascade's invalidated nodes (the old node among them) get their handlers
    if (ws.v_inv) {
        uint64_t n = 0;
        uint32_t* ids = IdsBuffer(ws.v_inv);
        Check(FGI_CALL(fgi_last_wave_ids, g_, ids, ws.v_inv, &n), "fgi_last_wave_ids");
        last_ = ws;
        Dispatch(ids, n);
    }
    current_[s] = c;
    has_obj_[s] = 1;
    if (OnRegister) OnRegister(*c);
    return c;
}

std::shared_ptr<Computed> ComputedRegistry::BeginCompute(const std::string& input, std::chrono::nanoseconds delay) {
    return BeginComputeImpl(input, delay != std::chrono::nanoseconds::zero(), DefaultOptions(delay));
}

uint32_t ComputedRegistry::AddUsed(Computed& dependant, Computed& used) {
    Sync();
    uint32_t out = 0;
    const uint32_t d = dependant.handle_, u = used.handle_;
    Check(FGI_CALL(fgi_add_used, g_, 1, &d, &u, &out), "fgi_add_used");
    return out;
}

bool ComputedRegistry::SetOutput(Computed& c, bool transient_error) {
    Sync();
    uint8_t set = 0;
    const uint32_t h = c.handle_;
    uint64_t n = 0;
    uint32_t* ids = IdsBuffer(1024);
    const std::chrono::nanoseconds auto_delay = transient_error ? c.transient_delay_ : c.auto_delay_;
    // the host path decides what the engine's kernel decides: a node that carries InvalidateOnSetOutput is
    // invalidated by the call and never starts its auto-invalidation (Computed.cs:153-156)
    const bool host_auto = !dev_timers_ && AutoTicks(auto_delay) != 0 && Owns(c);
    const bool ioso = host_auto && (fgi_view_flags(&view_, h) & FGI_F_INVALIDATE_ON_SET_OUTPUT) != 0;
    const uint8_t tr = transient_error ? 1 : 0;
    fgi_status s = dev_auto_ ? FGI_CALL(fgi_set_output_ex, g_, 1, &h, &tr, &set, ids, ids_cap_, &n, &last_)
                             : FGI_CALL(fgi_set_output, g_, 1, &h, &set, ids, ids_cap_, &n, &last_);
    if (s == FGI_ECAPACITY) {   // the cascade completed; fetch its ids with the right size
        ids = IdsBuffer(n);
        s = FGI_CALL(fgi_last_wave_ids, g_, ids, n, &n);
    }
    Check(s, "fgi_set_output");
    StartTimers(0);
    if (dev_auto_) maybe_armed_ = true;   // the engine armed the node behind the call
    if (host_auto && set && !ioso && (fgi_view_flags(&view_, h) & FGI_STATE_MASK) == FGI_CONSISTENT)
        StartAutoTimer(h, c.version_, auto_delay);   // StartAutoInvalidation (Computed.cs:235-246)
    Dispatch(ids, n);
    return set != 0;
}

void ComputedRegistry::RunWave(const uint32_t* roots, size_t n_roots, const uint8_t* imm) {
    Sync();
    uint64_t n = 0;
    last_ = fgi_wave_stats{};
    // the bitmap (n_handles / 8 bytes) costs less to bring back than the id list (4 B per node) once a
    // wave invalidates more than 1/32 of the handles; the previous wave's size predicts this one's
    const uint64_t words = ((uint64_t)n_handles_ + 63) / 64;
    const bool use_bits = WaveOutput == 2 || (WaveOutput == 0 && pred_v_ * 32 > (uint64_t)n_handles_);
    if (use_bits) {
        if (!bits_) bits_.reset(new uint64_t[words]);
        uint64_t* bits = bits_.get();
        Check(FGI_CALL(fgi_invalidate_bits, g_, (uint32_t)n_roots, roots, imm, bits, words, &n, &last_), "fgi_invalidate_bits");
        pred_v_ = n;
        StartTimers(0);
        DispatchBits(bits, words, n);
        return;
    }
    uint32_t* ids = IdsBuffer(1024);
    fgi_status s = FGI_CALL(fgi_invalidate, g_, (uint32_t)n_roots, roots, imm, ids, ids_cap_, &n, &last_);
    if (s == FGI_ECAPACITY) {   // the wave itself completed; fetch the ids with the right size
        ids = IdsBuffer(n);
        s = FGI_CALL(fgi_last_wave_ids, g_, ids, n, &n);
    }
    Check(s, "fgi_invalidate");
    pred_v_ = n;
    StartTimers(0);
    Dispatch(ids, n);
}

// The post-wave fan-out (fusion.hpp, "Threading"). Reference: InvalidatedHandlerSet.Invoke
// (Internal/InvalidatedHandlerSet.cs:100-127) per node; one `$sys-c.Invalidate` per replica call
// (Client/Internal/RpcInboundComputeCall.cs:53-62, 102-106), batched per peer here.
// Reentrant: peer sinks, batch handlers and Invalidated handlers are user code and may run waves
// themselves (a handler invalidating another node is the reference's normal pattern). While this
// fan-out runs it owns the ids buffer (a nested wave gets a fresh one) and its host objects are
// resolved before the first callback, so a nested BeginCompute that replaces a slot's node cannot
// redirect this wave's handlers to the new node.
void ComputedRegistry::Dispatch(const uint32_t* ids, uint64_t n) { DispatchImpl(ids, nullptr, 0, n); }

// The same fan-out over the wave's invalidated bitmap (fgi_invalidate_bits): each gather thread
// decodes its own range of words, so the ids are never materialised as a list (unless a batch
// handler wants them: chunks of BatchChunk are decoded for it).
void ComputedRegistry::DispatchBits(const uint64_t* bits, uint64_t words, uint64_t n) {
    DispatchImpl(nullptr, bits, words, n);
}

void ComputedRegistry::DispatchImpl(const uint32_t* ids, const uint64_t* bits, uint64_t words, uint64_t n) {
    const auto t0 = std::chrono::steady_clock::now();
    const bool from_ticket = from_ticket_;
    from_ticket_ = false;   // read once: the callbacks below may run waves of their own
    DropTimers(ids, bits, words, n);
    std::unique_ptr<uint32_t[]> own;
    uint64_t own_cap = 0;
    if (ids_ && ids && ids == ids_.get()) {
        own = std::move(ids_);
        own_cap = ids_cap_;
        ids_cap_ = 0;
    }
    std::unique_ptr<uint64_t[]> own_bits;
    if (bits_ && bits && bits == bits_.get()) own_bits = std::move(bits_);
    const uint32_t P = (uint32_t)peers_.size();
    FanoutStats fan;
    fan.ids = n;
    fan.peer_calls.assign(P, 0);
    fan.peer_batches.assign(P, 0);
    // 1. parallel gather: per thread, per peer call ids (ids ascending -> handle order), freed
    //    subscription entries, and the host objects of the ids (read-only lookups)
    uint32_t T = 1;
    if (n >= kParallelMin) {
        T = FanoutThreads ? FanoutThreads : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
        T = (uint32_t)std::min<uint64_t>(T, (n + kParallelMin - 1) / kParallelMin * 4);
    }
    fan.threads = T;
    fan.bitmap = bits ? 1u : 0u;
    struct Part {
        std::vector<std::vector<uint64_t>> calls;
        std::vector<uint32_t> freed;
        std::vector<std::pair<uint32_t, std::shared_ptr<Computed>>> objs;
    };
    std::vector<Part> parts(T);
    // DeviceFanout: the per-peer lists come from the engine's join (fgi_last_wave_fanout; a ticket's ids through
    // fgi_fanout_ids), fetched before the gather releases detached handles (a release drops their entries);
    // the gather then only resolves host objects and never touches sub_head_
    // The call ids land in a page-locked buffer kept across waves (no zero-fill, a copy at the link's rate).
    // This fan-out owns it while its callbacks run (a nested wave gets a fresh one), like the ids buffer.
    std::vector<uint64_t> dev_off;
    struct Lease {   // hands the (larger) buffer back when this fan-out ends, also by an exception
        ComputedRegistry* r;
        uint64_t* p;
        uint64_t cap;
        ~Lease() {
            if (!p) return;
            if (cap > r->dev_buf_cap_) {
                if (r->dev_buf_) fgi_free_pinned(r->dev_buf_);
                r->dev_buf_ = p;
                r->dev_buf_cap_ = cap;
            } else {
                fgi_free_pinned(p);
            }
        }
    } lease{this, dev_buf_, dev_buf_cap_};
    uint64_t*& dev_calls = lease.p;
    uint64_t& dev_cap = lease.cap;
    dev_buf_ = nullptr;
    dev_buf_cap_ = 0;
    auto dev_room = [&](uint64_t entries) {   // 8 B of call id and 4 B of handle per entry
        if (dev_cap >= entries && dev_calls) return;
        if (dev_calls) fgi_free_pinned(dev_calls);
        dev_calls = nullptr;
        dev_cap = 0;
        void* p = nullptr;
        Check(fgi_alloc_pinned(std::max<uint64_t>(entries, 4096) * 12, &p), "fgi_alloc_pinned");
        dev_calls = static_cast<uint64_t*>(p);
        dev_cap = std::max<uint64_t>(entries, 4096);
    };
    if (DeviceFanout && dev_subs_ && P && n) {
        dev_off.assign((size_t)P + 1, 0);
        uint64_t tot = 0;
        if (from_ticket && ids) {
            fgi_sub_stats st{};
            Check(FGI_CALL(fgi_sub_stats_get, g_, &st), "fgi_sub_stats_get");
            dev_room(std::max<uint64_t>(st.live, 1));
            Check(FGI_CALL(fgi_fanout_ids, g_, n, ids, P, dev_off.data(), dev_calls, reinterpret_cast<uint32_t*>(dev_calls + dev_cap),
                           dev_cap, &tot),
                  "fgi_fanout_ids");
        } else {
            Check(FGI_CALL(fgi_last_wave_fanout, g_, P, dev_off.data(), nullptr, nullptr, 0, &tot), "fgi_last_wave_fanout");
            if (tot) {
                dev_room(tot);
                Check(FGI_CALL(fgi_last_wave_fanout, g_, P, dev_off.data(), dev_calls, nullptr, dev_cap, &tot),
                      "fgi_last_wave_fanout");
            }
        }
        fgi_sub_stats st{};
        Check(FGI_CALL(fgi_sub_stats_get, g_, &st), "fgi_sub_stats_get");
        fan.device = 1;
        fan.device_kernel_ms = st.last_kernel_ms;
    }
    const bool any_subs = !DeviceFanout && !subs_.empty() && !sub_head_.empty();
    auto gather = [&](uint32_t t) {
        Part& pt = parts[t];
        pt.calls.resize(P);
        auto visit = [&](const uint32_t h) {
            if (h >= n_handles_) return;
            if (has_obj_[h]) {
                std::shared_ptr<Computed> c;
                if (h < n_slots_) {
                    c = current_[h];
                } else {
                    auto it = detached_.find(h);
                    if (it != detached_.end()) c = it->second;
                }
                pt.objs.emplace_back(h, std::move(c));
            }
            if (!any_subs || h >= sub_head_.size()) return;
            uint32_t e = sub_head_[h];
            if (e == kNone) return;
            sub_head_[h] = kNone;   // a call completes once (each handle is in one range only)
            while (e != kNone) {
                const Sub& sb = subs_[e];
                pt.calls[sb.peer].push_back(sb.call_id);
                pt.freed.push_back(e);
                e = sb.next;
            }
        };
        if (bits) {   // ascending handles of this thread's words
            const uint64_t lo = words * t / T, hi = words * (t + 1) / T;
            for (uint64_t w = lo; w < hi; ++w)
                for (uint64_t m = bits[w]; m; m &= m - 1) visit((uint32_t)(w * 64 + (uint64_t)__builtin_ctzll(m)));
        } else {
            const uint64_t lo = n * t / T, hi = n * (t + 1) / T;
            for (uint64_t i = lo; i < hi; ++i) visit(ids[i]);
        }
    };
    if (T == 1) {
        gather(0);
    } else {
        std::vector<std::thread> th;
        th.reserve(T - 1);
        for (uint32_t t = 1; t < T; ++t) th.emplace_back(gather, t);
        gather(0);
        for (auto& x : th) x.join();
    }
    for (auto& pt : parts) sub_free_.insert(sub_free_.end(), pt.freed.begin(), pt.freed.end());
    // detached nodes leave the engine now (before any callback can hand their handles out again)
    for (auto& pt : parts)
        for (auto& o : pt.objs) {
            const uint32_t h = o.first;
            if (h < n_slots_ || !o.second) continue;
            auto it = detached_.find(h);
            if (it != detached_.end() && it->second == o.second) {
                detached_.erase(it);
                has_obj_[h] = 0;
                FGI_CALL(fgi_release, g_, 1, &h);
            }
        }
    fan.gather_ms = ms_since(t0);
    // 2. per peer: its call ids in handle order, PeerBatch per sink call
    std::vector<uint64_t> buf;
    for (uint32_t q = 0; q < P; ++q) {
        uint64_t tot = 0;
        for (auto& pt : parts) tot += pt.calls[q].size();
        if (!dev_off.empty()) tot = dev_off[q + 1] - dev_off[q];
        if (!tot) continue;
        const uint64_t* data;
        if (!dev_off.empty()) {
            data = dev_calls + dev_off[q];
        } else if (T == 1) {
            data = parts[0].calls[q].data();
        } else {
            buf.clear();
            buf.reserve(tot);
            for (auto& pt : parts) buf.insert(buf.end(), pt.calls[q].begin(), pt.calls[q].end());
            data = buf.data();
        }
        const size_t B = std::max<size_t>(1, PeerBatch);
        for (uint64_t o = 0; o < tot; o += B) {
            const size_t k = (size_t)std::min<uint64_t>(B, tot - o);
            if (q < peers_.size() && peers_[q]) peers_[q](q, data + o, k);
            ++fan.peer_batches[q];
        }
        fan.peer_calls[q] = tot;
        fan.calls += tot;
        fan.batches += fan.peer_batches[q];
        ++fan.peers_hit;
    }
    // 3. the registry-level handler class, over the whole list
    if (OnInvalidatedBatch) {
        const size_t C = std::max<size_t>(1, BatchChunk);
        if (bits) {
            std::vector<uint32_t> chunk;
            chunk.reserve((size_t)std::min<uint64_t>(C, n));
            for (uint64_t w = 0; w < words; ++w)
                for (uint64_t m = bits[w]; m; m &= m - 1) {
                    chunk.push_back((uint32_t)(w * 64 + (uint64_t)__builtin_ctzll(m)));
                    if (chunk.size() == C) {
                        OnInvalidatedBatch(chunk.data(), chunk.size());
                        chunk.clear();
                    }
                }
            if (!chunk.empty()) OnInvalidatedBatch(chunk.data(), chunk.size());
        } else {
            for (uint64_t o = 0; o < n; o += C) OnInvalidatedBatch(ids + o, (size_t)std::min<uint64_t>(C, n - o));
        }
    }
    // 4. host objects: OnUnregister, then each node's handler set, exactly once
    for (auto& pt : parts) {
        for (auto& o : pt.objs) {
            Computed* c = o.second.get();
            if (!c || c->fired_) continue;
            ++fan.objects;
            c->fired_ = true;
            if (o.first < n_slots_ && OnUnregister) OnUnregister(*c);
            InvalidatedHandlerSet hs = std::move(c->handlers_);
            c->handlers_.Clear();
            hs.Invoke(*c);
        }
    }
    fan.dispatch_ms = ms_since(t0);
    fan_ = std::move(fan);
    if (own && own_cap > ids_cap_) {   // hand the (larger) buffer back for the next wave
        ids_ = std::move(own);
        ids_cap_ = own_cap;
    }
    if (own_bits && !bits_) bits_ = std::move(own_bits);
}

uint32_t ComputedRegistry::AddPeer(PeerSink sink) {
    peers_.push_back(std::move(sink));
    return (uint32_t)peers_.size() - 1;
}

void ComputedRegistry::Subscribe(uint32_t handle, uint32_t peer, uint64_t call_id) {
    Subscribe(1, &handle, &peer, &call_id);
}

void ComputedRegistry::Subscribe(size_t n, const uint32_t* handles, const uint32_t* peers, const uint64_t* call_ids) {
    if (DeviceFanout) {
        // the engine stores the entries (fgi_subscribe); a node that is Invalidated already completes its
        // WhenInvalidated at once (ComputedExt.cs:99-125): its call id goes to the peer's sink now
        for (size_t i = 0; i < n; ++i)
            if (peers[i] >= peers_.size()) throw FgiError(FGI_EINVAL, "Subscribe: bad handle or peer");
        std::vector<uint32_t> res(n);
        Check(FGI_CALL(fgi_subscribe, g_, (uint32_t)n, handles, peers, call_ids, res.data()), "fgi_subscribe");
        dev_subs_ = true;
        std::vector<std::vector<uint64_t>> now;
        for (size_t i = 0; i < n; ++i) {
            if (res[i] != FGI_SUB_INVALIDATED) continue;
            if (now.empty()) now.resize(peers_.size());
            now[peers[i]].push_back(call_ids[i]);
        }
        const size_t B = std::max<size_t>(1, PeerBatch);
        for (uint32_t q = 0; q < now.size(); ++q)
            for (size_t o = 0; o < now[q].size(); o += B)
                if (peers_[q]) peers_[q](q, now[q].data() + o, std::min(B, now[q].size() - o));
        return;
    }
    if (sub_head_.empty()) sub_head_.assign(n_handles_, kNone);   // once, on the first subscription
    for (size_t i = 0; i < n; ++i) {
        const uint32_t h = handles[i];
        if (h >= n_handles_ || peers[i] >= peers_.size()) throw FgiError(FGI_EINVAL, "Subscribe: bad handle or peer");
        uint32_t e;
        if (!sub_free_.empty()) {
            e = sub_free_.back();
            sub_free_.pop_back();
        } else {
            e = (uint32_t)subs_.size();
            subs_.push_back({});
        }
        subs_[e] = Sub{call_ids[i], peers[i], sub_head_[h]};
        sub_head_[h] = e;
    }
}

void ComputedRegistry::InvalidateInput(const std::string& input) {
    const uint32_t s = SlotOf(input, false);
    if (s == FGI_NONE) return;   // TryUseExisting: no existing computed -> nothing to invalidate
    if (IsInvalidating()) {
        scope_roots_.push_back(s);
        scope_imm_.push_back(0);
    } else {
        RunWave(&s, 1, nullptr);
    }
}

void ComputedRegistry::InvalidateSlots(const std::vector<uint32_t>& slots) {
    if (IsInvalidating()) {
        scope_roots_.insert(scope_roots_.end(), slots.begin(), slots.end());
        scope_imm_.insert(scope_imm_.end(), slots.size(), 0);
    } else {
        RunWave(slots.data(), slots.size(), nullptr);
    }
}

void ComputedRegistry::FlushScope() {
    const bool async = async_scope_;
    async_scope_ = false;
    if (scope_roots_.empty()) return;
    std::vector<uint32_t> roots;
    std::vector<uint8_t> imm;
    roots.swap(scope_roots_);
    imm.swap(scope_imm_);
    if (async) {
        InvalidateSlotsAsync(roots, &imm);
        return;
    }
    RunWave(roots.data(), roots.size(), imm.data());
}

// ---- asynchronous waves (ComputedExt.WhenInvalidated over fgi_invalidate_async_host) ------------------
// The engine keeps at most two waves in flight (a third call waits for the oldest inside the library);
// the mirror completes a wave — its ids brought back and fanned out exactly as a synchronous wave's —
// when asked, or before any other registry call (whose view of the registry must include the wave).
uint64_t ComputedRegistry::InvalidateSlotsAsync(const std::vector<uint32_t>& roots, const std::vector<uint8_t>* imm) {
    // a third wave makes the library wait for the oldest: complete it here so its fan-out runs in order
    while (pending_.size() >= 2) Complete(pending_.front());
    uint64_t t = 0;
    Check(FGI_CALL(fgi_invalidate_async_host, g_, (uint32_t)roots.size(), roots.data(),
                                    imm && imm->size() == roots.size() ? imm->data() : nullptr, &t),
          "fgi_invalidate_async_host");
    pending_.push_back(t);
    last_ticket_ = t;
    return t;
}

void ComputedRegistry::Complete(uint64_t ticket) {
    while (!pending_.empty() && pending_.front() <= ticket) {
        const uint64_t t = pending_.front();
        pending_.pop_front();   // before the fan-out: its handlers may call back into the registry
        fgi_wave_stats ws{};
        uint64_t n = 0;
        uint32_t* ids = IdsBuffer(1024);
        fgi_status s = FGI_CALL(fgi_wave_wait_ids, g_, t, ids, ids_cap_, &n, &ws);
        if (s == FGI_ECAPACITY) {   // the wave completed; fetch its ids with the right size
            ids = IdsBuffer(n);
            s = FGI_CALL(fgi_wave_wait_ids, g_, t, ids, n, &n, nullptr);
        }
        Check(s, "fgi_wave_wait_ids");
        last_ = ws;
        pred_v_ = n;
        StartTimers(t);
        from_ticket_ = true;   // the device fan-out of a ticket's ids goes through fgi_fanout_ids
        Dispatch(ids, n);
    }
}

void ComputedRegistry::CompletePending() {
    if (!pending_.empty()) Complete(pending_.back());
}

// ---- delayed invalidation (Computed.cs:186-197, ComputedExt.cs:10-45) -----------------------------------
// The reference's delayed node starts a timer of its own when Invalidate() only sets InvalidationDelayStarted;
// the timer calls Invalidate(true), and the node's Invalidated handler disposes it. Here the engine reports
// the nodes a wave flagged, the registry keeps one entry per such node, and the host drives the clock.
void ComputedRegistry::Sync() {
    CompletePending();
    RunDueTimers();
}

// DeviceTimers: the engine's timer set opens with the first registry call that needs the registry current
void ComputedRegistry::EnsureTimers() {
    if (dev_timers_ || !DeviceTimers) return;
    using ns = std::chrono::nanoseconds;
    fgi_timers_config cfg{};
    cfg.struct_size = sizeof(cfg);
    cfg.default_delay = DefaultInvalidationDelay > ns::zero() && DefaultInvalidationDelay != ns::max()
                            ? (uint64_t)DefaultInvalidationDelay.count() : 0ull;
    cfg.now = 0;
    Check(FGI_CALL(fgi_timers_open, g_, &cfg), "fgi_timers_open");
    epoch_ = Clock();
    slot_delay_.assign(n_slots_, 0);
    dev_timers_ = true;
}

void ComputedRegistry::EnsureAuto() {
    if (dev_auto_ || !dev_timers_) return;
    fgi_timers_auto_config cfg{};   // no graph defaults: every slot carries its node's own delays
    cfg.struct_size = sizeof(cfg);
    Check(FGI_CALL(fgi_timers_auto_open, g_, &cfg), "fgi_timers_auto_open");
    slot_auto_.assign(n_slots_, 0);
    slot_transient_.assign(n_slots_, 0);
    dev_auto_ = true;
}

// Clock in the engine's ticks: nanoseconds since the timers opened, never running backwards
uint64_t ComputedRegistry::NowTicks() {
    const auto d = std::chrono::duration_cast<std::chrono::nanoseconds>(Clock() - epoch_).count();
    return std::max<uint64_t>(ticks_, d > 0 ? (uint64_t)d : 0ull);
}

size_t ComputedRegistry::PendingTimers() const {
    if (!dev_timers_) return timers_.size();
    fgi_timer_stats st{};
    Check(FGI_CALL(fgi_timers_stats_get, g_, &st), "fgi_timers_stats_get");
    return (size_t)st.stored;
}

// One engine call per clock tick that can fire something. While no wave or displacement has run since the
// last look (maybe_armed_) and the clock is short of the engine's next due time, the tick costs the engine
// nothing but its clock (fgi_timers_set_now: no device work), which the next wave arms by.
size_t ComputedRegistry::RunDueTimersDevice() {
    if (in_timers_) return 0;
    CompletePending();
    const uint64_t now = NowTicks();
    if (!maybe_armed_ && now < next_due_) {
        if (now > ticks_) {
            Check(FGI_CALL(fgi_timers_set_now, g_, now), "fgi_timers_set_now");
            ticks_ = now;
        }
        return 0;
    }
    maybe_armed_ = false;   // before the fan-out: its callbacks may run waves of their own
    fgi_wave_stats ws{};
    uint64_t n = 0, fired = 0;
    uint32_t* ids = IdsBuffer(1024);
    fgi_status s = FGI_CALL(fgi_timers_run_due, g_, now, ids, ids_cap_, &n, &fired, &ws);
    if (s == FGI_ECAPACITY) {   // the wave itself completed; fetch the ids with the right size
        ids = IdsBuffer(n);
        s = FGI_CALL(fgi_last_wave_ids, g_, ids, n, &n);
    }
    Check(s, "fgi_timers_run_due");
    ticks_ = now;
    Check(FGI_CALL(fgi_timers_next_due, g_, &next_due_, nullptr), "fgi_timers_next_due");   // the fired wave's own flagged set included
    if (!fired) return 0;
    last_ = ws;
    pred_v_ = n;
    struct Guard {
        bool& b;
        ~Guard() { b = false; }
    } guard{in_timers_};
    in_timers_ = true;
    Dispatch(ids, n);   // exactly as RunWave fans out
    return (size_t)fired;
}

void ComputedRegistry::StartTimer(uint32_t handle, LTag version, std::chrono::nanoseconds delay) {
    using ns = std::chrono::nanoseconds;
    if (delay == ns::zero()) delay = DefaultInvalidationDelay;
    if (delay <= ns::zero() || delay == ns::max()) return;   // none, or never (TimeSpan.MaxValue, ComputedExt.cs:12)
    auto it = timers_.find(handle);
    const TimePoint now = Clock();
    const TimePoint due = delay > TimePoint::max() - now ? TimePoint::max() : now + delay;
    if (it != timers_.end() && it->second.version == version) {
        // already running; an auto-invalidation's entry keeps the earlier due time (AddOrUpdateToEarlier)
        if (it->second.is_auto && due < it->second.due) it->second.due = due;
        return;
    }
    timers_[handle] = Timer{due, version, false};
}

void ComputedRegistry::StartAutoTimer(uint32_t handle, LTag version, std::chrono::nanoseconds delay) {
    using ns = std::chrono::nanoseconds;
    if (delay <= ns::zero() || delay == ns::max()) return;   // off (Computed.cs:244); "at once" is not built
    const TimePoint now = Clock();
    const TimePoint due = delay > TimePoint::max() - now ? TimePoint::max() : now + delay;
    auto it = timers_.find(handle);
    if (it != timers_.end() && it->second.version == version) {
        if (due < it->second.due) it->second.due = due;
        it->second.is_auto = true;
        return;
    }
    timers_[handle] = Timer{due, version, true};
}

void ComputedRegistry::StartTimers(uint64_t ticket) {
    if (dev_timers_) {   // the engine armed them behind the wave; the next tick asks it what is due
        maybe_armed_ = true;
        return;
    }
    auto read = [&](uint32_t* ids, uint32_t* flags, uint64_t cap, uint64_t* n) {
        return ticket ? FGI_CALL(fgi_wave_wait_flagged, g_, ticket, ids, flags, cap, n) : FGI_CALL(fgi_last_wave_flagged, g_, ids, flags, cap, n);
    };
    uint64_t n = 0;
    Check(read(nullptr, nullptr, 0, &n), "fgi_last_wave_flagged");
    if (!n) return;
    std::vector<uint32_t> ids(n), flags(n);
    Check(read(ids.data(), flags.data(), n, &n), "fgi_last_wave_flagged");
    std::vector<uint32_t> bare;   // flagged nodes without a host object (bulk-registered)
    for (uint64_t i = 0; i < n; ++i) {
        // Computing nodes in the set need no host action: TrySetOutput invalidates them (Computed.cs:153-156)
        if ((flags[i] & FGI_STATE_MASK) != FGI_CONSISTENT || !(flags[i] & FGI_F_INVALIDATION_DELAY_STARTED)) continue;
        const uint32_t h = ids[i];
        std::shared_ptr<Computed> c;
        if (h < n_slots_) {
            c = current_[h];
        } else {
            auto it = detached_.find(h);
            if (it != detached_.end()) c = it->second;
        }
        if (c) StartTimer(h, c->version_, c->delay_);
        else bare.push_back(h);
    }
    if (bare.empty() || DefaultInvalidationDelay <= std::chrono::nanoseconds::zero()) return;
    std::vector<uint64_t> ver(bare.size());
    std::vector<uint32_t> fl(bare.size());
    Check(FGI_CALL(fgi_get_state, g_, (uint32_t)bare.size(), bare.data(), ver.data(), fl.data()), "fgi_get_state");
    for (size_t i = 0; i < bare.size(); ++i) StartTimer(bare[i], ver[i], std::chrono::nanoseconds::zero());
}

void ComputedRegistry::DropTimers(const uint32_t* ids, const uint64_t* bits, uint64_t words, uint64_t n) {
    if (dev_timers_ || timers_.empty() || n == 0) return;   // (the engine removes a stale entry when it comes due)
    for (auto it = timers_.begin(); it != timers_.end();) {
        const uint32_t h = it->first;
        const bool hit = bits ? ((uint64_t)(h >> 6) < words && ((bits[h >> 6] >> (h & 63)) & 1ull))
                              : (ids && std::binary_search(ids, ids + n, h));   // ids come in ascending order
        it = hit ? timers_.erase(it) : std::next(it);
    }
}

size_t ComputedRegistry::RunDueTimers() {
    EnsureTimers();
    if (dev_timers_) return RunDueTimersDevice();
    if (in_timers_ || timers_.empty()) return 0;
    CompletePending();   // a wave in flight may have invalidated a due node: its fan-out removes the entry
    const TimePoint now = Clock();
    std::vector<std::pair<uint32_t, LTag>> entries;   // (handle, version << 1 | auto)
    for (auto it = timers_.begin(); it != timers_.end();) {
        if (it->second.due <= now) {
            entries.emplace_back(it->first, it->second.version << 1 | (it->second.is_auto ? 1u : 0u));
            it = timers_.erase(it);
        } else {
            ++it;
        }
    }
    if (entries.empty()) return 0;
    std::sort(entries.begin(), entries.end());
    std::vector<uint32_t> due;
    for (const auto& e : entries) due.push_back(e.first);
    // the entry fires only for the node it was started for, still Consistent, and waiting (DelayStarted) unless
    // the entry is an auto-invalidation's, whose timer invalidates any live node (ComputedExt.cs:35)
    std::vector<uint64_t> ver(due.size());
    std::vector<uint32_t> fl(due.size());
    Check(FGI_CALL(fgi_get_state, g_, (uint32_t)due.size(), due.data(), ver.data(), fl.data()), "fgi_get_state");
    std::vector<uint32_t> roots;
    for (size_t i = 0; i < due.size(); ++i)
        if (ver[i] == entries[i].second >> 1 && (fl[i] & FGI_STATE_MASK) == FGI_CONSISTENT &&
            ((fl[i] & FGI_F_INVALIDATION_DELAY_STARTED) || (entries[i].second & 1)))
            roots.push_back(due[i]);
    if (roots.empty()) return 0;
    const std::vector<uint8_t> imm(roots.size(), 1);
    struct Guard {
        bool& b;
        ~Guard() { b = false; }
    } guard{in_timers_};
    in_timers_ = true;
    RunWave(roots.data(), roots.size(), imm.data());   // Invalidate(true), one wave for the batch
    return roots.size();
}

// ---- access reports (ComputedRegistry.ReportAccess, Computed.RenewTimeouts) -----------------------
void ComputedRegistry::ReportAccess(Computed& c, bool is_new) {
    if (!OnAccess) return;
    if (c.IsInvalidated()) return;   // RenewTimeouts returns early for an Invalidated node (Computed.cs:250-251)
    OnAccess(c, is_new);
}

std::shared_ptr<Computed> ComputedRegistry::TryUseExisting(const std::string& input, Computed* usedBy) {
    auto existing = Get(input);
    if (!existing || !existing->IsConsistent()) return nullptr;
    if (usedBy) AddUsed(*usedBy, *existing);
    if (OnAccess) OnAccess(*existing, true);   // Consistent: RenewTimeouts(true) reports it
    return existing;
}

std::shared_ptr<Computed> ComputedRegistry::GetExisting(const std::string& input) {
    Sync();
    const uint32_t s = SlotOf(input, false);
    if (s == FGI_NONE || !current_[s]) return nullptr;
    ReportAccess(*current_[s], false);
    return current_[s];
}

void ComputedRegistry::UseNew(Computed& computed, Computed* usedBy) {
    if (usedBy) AddUsed(*usedBy, computed);
    ReportAccess(computed, true);
}

void ComputedRegistry::InvalidateEverything() {
    Sync();
    uint64_t n = 0;
    last_ = fgi_wave_stats{};
    uint32_t* ids = IdsBuffer(1024);
    fgi_status s = FGI_CALL(fgi_invalidate_all, g_, ids, ids_cap_, &n, &last_);
    if (s == FGI_ECAPACITY) {
        ids = IdsBuffer(n);
        s = FGI_CALL(fgi_last_wave_ids, g_, ids, n, &n);
    }
    Check(s, "fgi_invalidate_all");
    StartTimers(0);
    Dispatch(ids, n);
}

std::pair<uint64_t, uint64_t> ComputedRegistry::Prune() {
    Sync();
    fgi_prune_stats ps{};
    Check(FGI_CALL(fgi_prune, g_, &ps), "fgi_prune");
    return {ps.old_edges, ps.new_edges};
}

bool ComputedRegistry::Owns(const Computed& c) const {
    if (c.gone_) return false;
    if (c.handle_ < n_slots_) return current_[c.handle_].get() == &c;
    auto it = detached_.find(c.handle_);
    return it != detached_.end() && it->second.get() == &c;
}

// ---- Computed --------------------------------------------------------------------------------------
ConsistencyState Computed::State() const { return (ConsistencyState)(Flags() & FGI_STATE_MASK); }

bool Computed::IsConsistent() const {
    reg_->CompletePending();
    return reg_->Owns(*this) && fgi_view_is_consistent(&reg_->view_, handle_);
}

uint32_t Computed::Flags() const {
    reg_->CompletePending();   // the state includes the waves in flight (their handlers run first)
    if (!reg_->Owns(*this)) return FGI_INVALIDATED;   // the slot moved on, or the handle was released: this node is gone
    return fgi_view_flags(&reg_->view_, handle_);
}

void Computed::Invalidate(bool immediately) {
    if (reg_->IsInvalidating()) {
        reg_->scope_roots_.push_back(handle_);
        reg_->scope_imm_.push_back(immediately ? 1 : 0);
    } else {
        const uint8_t imm = immediately ? 1 : 0;
        reg_->RunWave(&handle_, 1, &imm);
    }
}

InvalidatedHandler Computed::OnInvalidated(std::function<void(Computed&)> handler) {
    auto h = std::make_shared<const std::function<void(Computed&)>>(std::move(handler));
    OnInvalidated(h);
    return h;
}

void Computed::OnInvalidated(const InvalidatedHandler& handler) {
    if (fired_ || IsInvalidated()) {   // Computed.cs:84-97: added after invalidation -> fires now
        (*handler)(*this);
        return;
    }
    handlers_.Add(handler);
}

void Computed::RemoveOnInvalidated(const InvalidatedHandler& handler) { handlers_.Remove(handler); }

std::shared_future<void> Computed::WhenInvalidated() {
    if (when_) return when_f_;
    when_ = std::make_shared<std::promise<void>>();
    when_f_ = when_->get_future().share();
    // ComputedExt.cs:101-102: already Invalidated -> completed. Every invalidation of a node the mirror
    // holds goes through its fan-out (fired_), so the test needs no device query — which would complete
    // the asynchronous waves in flight, while the caller wants to await them.
    if (fired_) {
        when_->set_value();
        return when_f_;
    }
    std::shared_ptr<std::promise<void>> p = when_;
    handlers_.Add(std::make_shared<const std::function<void(Computed&)>>([p](Computed&) { p->set_value(); }));
    return when_f_;
}

std::vector<std::pair<uint32_t, LTag>> Computed::UsedBy() const {
    uint64_t n = 0;
    FGI_RCALL(fgi_get_used_by, reg_->g_, handle_, nullptr, nullptr, 0, &n);
    std::vector<uint32_t> d(n);
    std::vector<uint64_t> t(n);
    reg_->Check(FGI_RCALL(fgi_get_used_by, reg_->g_, handle_, d.data(), t.data(), n, &n), "fgi_get_used_by");
    std::vector<std::pair<uint32_t, LTag>> out;
    for (uint64_t i = 0; i < n; ++i) out.emplace_back(d[i], t[i]);
    return out;
}

uint32_t Computed::UsedCount() const {
    uint32_t c = 0;
    reg_->Check(FGI_RCALL(fgi_get_used_count, reg_->g_, handle_, &c), "fgi_get_used_count");
    return c;
}

}  // namespace fusion
