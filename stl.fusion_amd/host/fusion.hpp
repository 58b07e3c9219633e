// fusion.hpp — host-layer mirror of Stl.Fusion's invalidation API over the fgi C-ABI.
//
// This is the layer a Fusion host keeps in front of the engine. It mirrors:
//   ComputedRegistry.Get / Register / InvalidateEverything / OnRegister / OnUnregister / OnAccess
//                                                   (src/Stl.Fusion/ComputedRegistry.cs:34-147, 172-176)
//   ComputedExt.TryUseExisting / UseNew -> RenewTimeouts -> ReportAccess
//                                                   (Internal/ComputedExt.cs:10-76, Computed.cs:248-262)
//   ComputedExt.WhenInvalidated                      (ComputedExt.cs:99-125): a future completed by the
//                                                   node's Invalidated handler, also across asynchronous
//                                                   (pipelined) waves (fgi_invalidate_async_host)
//   Computed.Invalidate() scope, Computed.IsInvalidating()   (Computed.Static.cs:41-47)
//   IComputed.Invalidate(immediately), ConsistencyState, Version, event Invalidated
//                                                   (Computed.cs:11-26, 84-105, 162)
//   InvalidatedHandlerSet                            (Internal/InvalidatedHandlerSet.cs:3-128)
//   ComputeMethodFunctionBase.Compute -> new Computing node (ComputeMethodFunctionBase.cs:19-27)
//   IComputedImpl.AddUsed, TrySetOutput, UsedBy      (Computed.cs:141-160, 327-385)
//   ComputedGraphPruner pass                         (Internal/ComputedGraphPruner.cs:79-94)
//   Delayed invalidation: a Consistent node with an InvalidationDelay that a cascade reaches only gets
//   InvalidationDelayStarted and schedules its own timer, which later calls Invalidate(true)
//                                                   (Computed.cs:186-197, ComputedExt.cs:10-45) — here
//   a timer entry per node the engine reports as flagged (fgi_last_wave_flagged /
//   fgi_wave_wait_flagged), on a registry clock tests can drive: no threads, no sleeping; RunDueTimers
//   invalidates what is due.
//   Auto-invalidation: TrySetOutput -> StartAutoInvalidation (Computed.cs:158, 235-246) schedules Invalidate(true)
//   after ComputedOptions.AutoInvalidationDelay, or TransientErrorInvalidationDelay when the output is a
//   transient error, on the same timer set with AddOrUpdateToEarlier (ComputedExt.cs:10-25) — here a second
//   kind of entry on the same registry clock, or in the engine (fgi_timers_auto_open) with DeviceTimers.
//   RPC replica invalidation: an inbound compute call waits for its computed's invalidation and
//   then sends `$sys-c.Invalidate(callId)` to its peer (Client/Internal/RpcInboundComputeCall.cs:
//   53-62, 102-106) — here a subscription (handle -> peer, call id), delivered per peer in batches
//   after the wave.
// The C# host this stands in for is sketched in INTEGRATION.md ([LibraryImport] stubs); no .NET
// SDK exists in this image, so the mirror is C++ and is exercised by host/test_fusion.cpp.
//
// Threading: one registry = one dispatcher thread (the ABI is externally synchronised). After each
// wave the dispatcher fans the returned ids out (Dispatch):
//   1. in parallel over contiguous id ranges (ids come in ascending order), or over ranges of the
//      wave's invalidated bitmap when the wave returned one (large waves): per-peer call-id lists
//      (subscriptions are consumed: a call completes once), and the ids that have host objects;
//   2. per peer, its call ids in handle order, cut into batches of at most PeerBatch — one sink
//      call per batch (what one `$sys-c.Invalidate` message per peer per batch would carry);
//   3. registry-level batch handlers get the whole id list in chunks of BatchChunk;
//   4. per host object: OnUnregister, then its InvalidatedHandlerSet, each handler exactly once.
#pragma once

#include <chrono>
#include <cstdint>
#include <deque>
#include <functional>
#include <future>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/fgi.h"

namespace fusion {

using LTag = uint64_t;
enum class ConsistencyState : uint32_t { Computing = 0, Consistent = 1, Invalidated = 2 };

class Computed;
class ComputedRegistry;

// ComputedOptions' three delays (ComputedOptions.cs). InvalidationDelay: 0 = none, max() = never. The other two:
// max() = off (TimeSpan.MaxValue, Computed.cs:244); a value <= 0, the reference's "invalidate at once"
// (ComputedExt.cs:15-18), is not built and reads as off. The reference's default
// TransientErrorInvalidationDelay is 1 s; here it is off unless set, so a registry that never sets it behaves
// as it did before auto-invalidation existed.
struct ComputedOptions {
    std::chrono::nanoseconds InvalidationDelay{0};
    std::chrono::nanoseconds AutoInvalidationDelay = std::chrono::nanoseconds::max();
    std::chrono::nanoseconds TransientErrorInvalidationDelay = std::chrono::nanoseconds::max();
};

class FgiError : public std::runtime_error {
   public:
    FgiError(fgi_status s, const std::string& what) : std::runtime_error(what), status(s) {}
    fgi_status status;
};

// A handler's identity is its shared_ptr (the reference compares delegates).
using InvalidatedHandler = std::shared_ptr<const std::function<void(Computed&)>>;

// InvalidatedHandlerSet (Internal/InvalidatedHandlerSet.cs:3-128): empty, one handler, a list of up
// to ListSize, then a hash set. Add of a handler already present is a no-op; Remove keeps the order
// of the rest; Invoke calls each handler once (list order; set order unspecified, as there).
class InvalidatedHandlerSet {
   public:
    static constexpr size_t ListSize = 5;
    void Add(const InvalidatedHandler& h);
    void Remove(const InvalidatedHandler& h);
    void Clear() {
        list_.clear();
        set_.reset();
    }
    size_t Size() const { return set_ ? set_->size() : list_.size(); }
    bool Spilled() const { return (bool)set_; }
    void Invoke(Computed& c) const;

   private:
    std::vector<InvalidatedHandler> list_;                         // <= ListSize entries
    std::unique_ptr<std::unordered_set<InvalidatedHandler>> set_;  // after the list overflows
};

// One Computed instance (a node). Holds the engine handle: the input's slot while it is the
// registered node, or a detached handle once a newer computation displaced it.
class Computed {
   public:
    const std::string& Input() const { return input_; }
    LTag Version() const { return version_; }
    uint32_t Handle() const { return handle_; }
    // The node's state is read from the registry's host-memory state view (fgi_state_view_open): a load,
    // no engine call, once the asynchronous waves in flight are completed (their handlers run first).
    // A node that is gone — its slot holds a newer object, or its detached handle was released — reads
    // as Invalidated; that is decided on the host (the slot's current object, the detached map).
    ConsistencyState State() const;
    uint32_t Flags() const;   // fgi state_flags (InvalidateOnSetOutput, DelayStarted, hasDelay)
    bool IsConsistent() const;   // one load, one bit test
    bool IsInvalidated() const { return State() == ConsistencyState::Invalidated; }
    // IComputed.Invalidate(immediately): inside a Computed.Invalidate() scope the node joins the
    // scope's batch; otherwise one wave runs now.
    void Invalidate(bool immediately = false);
    // event Invalidated += / -= (Computed.cs:84-105): fires once; added after invalidation it fires
    // at once. Returns the handler's identity for RemoveOnInvalidated.
    InvalidatedHandler OnInvalidated(std::function<void(Computed&)> handler);
    void OnInvalidated(const InvalidatedHandler& handler);
    void RemoveOnInvalidated(const InvalidatedHandler& handler);
    std::vector<std::pair<uint32_t, LTag>> UsedBy() const;   // IComputedImpl.UsedBy
    uint32_t UsedCount() const;                               // IComputedImpl.Used.Length
    // ComputedExt.WhenInvalidated (ComputedExt.cs:99-125): ready at once for an Invalidated node, else
    // completed by the node's Invalidated event — after a synchronous wave's fan-out, or when the
    // registry completes the asynchronous wave that invalidated it (Complete / CompletePending). Every call
    // returns the same future.
    std::shared_future<void> WhenInvalidated();

   private:
    friend class ComputedRegistry;
    ComputedRegistry* reg_ = nullptr;
    std::string input_;
    uint32_t slot_ = 0, handle_ = 0;
    LTag version_ = 0;
    bool fired_ = false;
    bool gone_ = false;   // displaced without a detached handle: the slot names the newer node
    InvalidatedHandlerSet handlers_;
    std::chrono::nanoseconds delay_{0};          // ComputedOptions.InvalidationDelay (0: none, max(): never)
    // AutoInvalidationDelay / TransientErrorInvalidationDelay as they hold for this node (max(): off)
    std::chrono::nanoseconds auto_delay_ = std::chrono::nanoseconds::max();
    std::chrono::nanoseconds transient_delay_ = std::chrono::nanoseconds::max();
    std::shared_ptr<std::promise<void>> when_;   // WhenInvalidated's promise, once asked for
    std::shared_future<void> when_f_;
};

// Per-wave fan-out statistics (the last Dispatch).
struct FanoutStats {
    uint64_t ids = 0;            // invalidated handles dispatched
    uint64_t objects = 0;        // of which had host objects (handlers / OnUnregister ran)
    uint64_t calls = 0;          // peer call ids delivered
    uint64_t batches = 0;        // peer sink invocations
    uint32_t peers_hit = 0;      // peers that received at least one batch
    uint32_t threads = 0;        // threads of the parallel phase
    uint32_t bitmap = 0;         // 1: dispatched from the wave's invalidated bitmap (fgi_invalidate_bits)
    double dispatch_ms = 0;      // whole Dispatch
    double gather_ms = 0;        // parallel phase (subscriptions -> per-peer lists)
    uint32_t device = 0;         // 1: the per-peer lists came from the engine's join (DeviceFanout)
    double device_kernel_ms = 0; // ... and the device time of its kernels (fgi_sub_stats.last_kernel_ms)
    std::vector<uint64_t> peer_calls, peer_batches;   // per peer id
};

class ComputedRegistry {
   public:
    ComputedRegistry(uint32_t n_slots, uint32_t n_detached = 1024, int device = 0);
    ~ComputedRegistry();
    ComputedRegistry(const ComputedRegistry&) = delete;
    ComputedRegistry& operator=(const ComputedRegistry&) = delete;

    // ComputedRegistry.Get: the current (registered, not invalidated) node of an input, or null
    std::shared_ptr<Computed> Get(const std::string& input);
    // ComputeMethodFunctionBase.Compute: a new Computing node of `input` replaces (and, per
    // Register, invalidates) the current one
    // has_delay without a duration: the node is flagged like a delayed one (InvalidationDelayStarted), and
    // gets a timer only if the registry has a DefaultInvalidationDelay
    std::shared_ptr<Computed> BeginCompute(const std::string& input, bool has_delay = false);
    // ComputedOptions.InvalidationDelay: 0 = none, nanoseconds::max() = never (TimeSpan.MaxValue,
    // ComputedExt.cs:12: the node is flagged, no timer starts)
    std::shared_ptr<Computed> BeginCompute(const std::string& input, std::chrono::nanoseconds delay);
    // every delay of the node given explicitly; the overloads above take the registry's
    // DefaultAutoInvalidationDelay / DefaultTransientErrorInvalidationDelay
    std::shared_ptr<Computed> BeginCompute(const std::string& input, const ComputedOptions& options);
    // dependant.AddUsed(used); returns the FGI_USED_* outcome (FGI_USED_ESTATE = the reference throws)
    uint32_t AddUsed(Computed& dependant, Computed& used);
    // TrySetOutput: true if the node was Computing; an InvalidateOnSetOutput node cascades at once
    // (Computed.cs:153-156), any other starts its auto-invalidation (Computed.cs:158): after its
    // TransientErrorInvalidationDelay if transient_error, else after its AutoInvalidationDelay
    bool SetOutput(Computed& c, bool transient_error = false);
    void InvalidateEverything();
    // one ComputedGraphPruner pass; returns (old, new) `_usedBy` totals of the pruned nodes
    std::pair<uint64_t, uint64_t> Prune();

    // ComputedExt.TryUseExisting with no call options (Internal/ComputedExt.cs:10-23): the input's
    // Consistent current node, made a dependency of usedBy (nullable) and reported as accessed
    // (RenewTimeouts(true) -> OnAccess); null if there is none (the caller computes it)
    std::shared_ptr<Computed> TryUseExisting(const std::string& input, Computed* usedBy = nullptr);
    // CallOptions.GetExisting (ComputedExt.cs:38-42): the current node in any state, reported as
    // accessed with isNew = false unless it is Invalidated (RenewTimeouts returns early then)
    std::shared_ptr<Computed> GetExisting(const std::string& input);
    // ComputedExt.UseNew (ComputedExt.cs:70-76) after a computation: AddUsed from usedBy, then the access
    // report with isNew = true
    void UseNew(Computed& computed, Computed* usedBy = nullptr);

    // `using (Computed.Invalidate()) { ... }`: roots collected while the scope is open are
    // invalidated as one batched wave when the outermost scope closes.
    class InvalidationScope {
       public:
        explicit InvalidationScope(ComputedRegistry* r) : r_(r) { ++r_->scope_depth_; }
        InvalidationScope(InvalidationScope&& o) noexcept : r_(o.r_) { o.r_ = nullptr; }
        ~InvalidationScope() {
            if (r_ && --r_->scope_depth_ == 0) r_->FlushScope();
        }

       private:
        ComputedRegistry* r_;
    };
    InvalidationScope Invalidate() { return InvalidationScope(this); }
    bool IsInvalidating() const { return scope_depth_ > 0; }
    // The same scope, flushed as an asynchronous wave (fgi_invalidate_async_host): closing the outermost
    // scope queues the wave and returns; the nodes' Invalidated handlers (and WhenInvalidated futures) run
    // when the registry completes the wave — Complete(ticket), CompletePending(), or any other registry
    // call, which completes the waves in flight first. LastTicket() names the last queued wave.
    InvalidationScope InvalidateAsync() {
        if (scope_depth_ == 0) async_scope_ = true;   // only the outermost scope decides how the batch is flushed
        return InvalidationScope(this);
    }
    uint64_t LastTicket() const { return last_ticket_; }
    // Queue one wave from slot / handle roots without waiting (what an async scope's flush does)
    uint64_t InvalidateSlotsAsync(const std::vector<uint32_t>& roots, const std::vector<uint8_t>* immediately = nullptr);
    // Wait for the asynchronous waves up to `ticket` (in order) and fan their results out (Dispatch)
    void Complete(uint64_t ticket);
    void CompletePending();
    size_t PendingWaves() const { return pending_.size(); }
    // ---- delayed invalidation (Computed.cs:186-197 -> ComputedExt.Invalidate(TimeSpan), ComputedExt.cs:10-45) --
    // After every wave the registry runs (RunWave in both output forms, Complete, BeginCompute's displacement
    // cascade, SetOutput's cascade, InvalidateEverything) it reads the wave's flagged set; each handle reported
    // Consistent with InvalidationDelayStarted gets a timer entry (due time, handle, version) — its node's
    // delay, or DefaultInvalidationDelay for a node without one (has_delay only, bulk-registered). Computing
    // nodes in the set need no host action: fgi_set_output cascades them. RunDueTimers invalidates every due
    // entry with immediately = true in one wave; an entry whose node was invalidated meanwhile is removed
    // when that wave is fanned out (ComputedExt.cs:38-45), never fired. It also runs at the start of every
    // registry call that completes the pending waves. Returns the entries fired.
    using TimePoint = std::chrono::steady_clock::time_point;
    std::function<TimePoint()> Clock = [] { return std::chrono::steady_clock::now(); };
    std::chrono::nanoseconds DefaultInvalidationDelay{0};
    // auto-invalidation of the nodes begun without ComputedOptions; max(): off (the reference's transient
    // default is 1 s, see ComputedOptions above)
    std::chrono::nanoseconds DefaultAutoInvalidationDelay = std::chrono::nanoseconds::max();
    std::chrono::nanoseconds DefaultTransientErrorInvalidationDelay = std::chrono::nanoseconds::max();
    size_t RunDueTimers();
    size_t PendingTimers() const;
    // The timers live in the engine (fgi_timers_*, fgi.h): its kernels arm them behind every wave from the
    // flagged records and fgi_timers_run_due fires them, so the registry neither downloads a flagged set nor
    // keeps an entry per node. Set before the first BeginCompute (with DefaultInvalidationDelay, which the
    // engine takes when the timers open) and left alone afterwards. Clock maps to ticks: nanoseconds since the
    // timers opened. BeginCompute(input, delay) sets the slot's delay. PendingTimers() is the engine's stored
    // count, which keeps the entry of a node invalidated before its due time until that time comes.
    bool DeviceTimers = false;
    // `_ = svc.Get(input)` inside a scope: TryUseExisting's Invalidate branch (ComputedExt.cs:29-35)
    void InvalidateInput(const std::string& input);
    // Slot-level roots (inputs already resolved by the host, e.g. bulk-registered nodes)
    void InvalidateSlots(const std::vector<uint32_t>& slots);

    // ---- RPC replica fan-out -----------------------------------------------------------------
    // A peer's sink receives its invalidated call ids, in handle order, PeerBatch at most per call.
    using PeerSink = std::function<void(uint32_t peer, const uint64_t* call_ids, size_t n)>;
    uint32_t AddPeer(PeerSink sink);
    // An inbound compute call of `peer` (call id) now waits for the node `handle`'s invalidation.
    void Subscribe(uint32_t handle, uint32_t peer, uint64_t call_id);
    void Subscribe(size_t n, const uint32_t* handles, const uint32_t* peers, const uint64_t* call_ids);
    size_t PeerBatch = 4096;
    // The subscriptions live in the engine (fgi_subscribe) and a wave's per-peer lists come from its join on
    // the device (fgi_last_wave_fanout; fgi_fanout_ids for an asynchronous ticket's ids) instead of the gather
    // over sub_head_. Set before the first Subscribe and left alone afterwards; at most FGI_MAX_PEERS peers.
    // Subscribing to a node that is Invalidated already delivers its call id at once. Handler objects keep
    // their host path; the delay timers have a switch of their own (DeviceTimers).
    bool DeviceFanout = false;
    uint32_t FanoutThreads = 0;   // 0: hardware concurrency, capped at 16

    // how a wave's invalidated set comes back: 0 auto (the bitmap once the previous wave invalidated
    // more than 1/32 of the handles), 1 the id list, 2 the bitmap (fgi_invalidate_bits)
    int WaveOutput = 0;

    std::function<void(Computed&)> OnRegister, OnUnregister;
    // event OnAccess (ComputedRegistry.cs:36, ReportAccess 172-176): a compute-method node was used —
    // isNew is RenewTimeouts' argument (TryUseExisting / UseNew: true, GetExisting: false)
    std::function<void(Computed&, bool)> OnAccess;
    // registry-level handler class: the wave's invalidated handles, BatchChunk at a time
    std::function<void(const uint32_t* ids, size_t n)> OnInvalidatedBatch;
    size_t BatchChunk = 65536;

    fgi_graph* Graph() const { return g_; }
    // the registry's state view (opened at construction): any thread may read it
    const fgi_state_view& View() const { return view_; }
    // every fgi_* call the mirror has made so far (a state read makes none)
    uint64_t EngineCalls() const { return calls_; }
    const fgi_wave_stats& LastWave() const { return last_; }
    const FanoutStats& LastFanout() const { return fan_; }

   private:
    friend class Computed;
    struct Sub {
        uint64_t call_id;
        uint32_t peer, next;
    };
    void Check(fgi_status s, const char* what) const;
    uint32_t SlotOf(const std::string& input, bool create);
    void RunWave(const uint32_t* roots, size_t n, const uint8_t* imm);
    // the engine's ids of the last call into ids_ (grown without zero-fill, reused across waves)
    uint32_t* IdsBuffer(uint64_t need);
    void Dispatch(const uint32_t* ids, uint64_t n);
    void DispatchBits(const uint64_t* bits, uint64_t words, uint64_t n);
    void DispatchImpl(const uint32_t* ids, const uint64_t* bits, uint64_t words, uint64_t n);
    void FlushScope();
    // CompletePending, then RunDueTimers: the start of every registry call that needs the registry current
    void Sync();
    // the flagged set of the last synchronous call (ticket 0) or of an asynchronous ticket -> timer entries
    void StartTimers(uint64_t ticket);
    void StartTimer(uint32_t handle, LTag version, std::chrono::nanoseconds delay);
    // an auto-invalidation's entry; one of the same version keeps the earlier due time (AddOrUpdateToEarlier)
    void StartAutoTimer(uint32_t handle, LTag version, std::chrono::nanoseconds delay);
    // the timers of the nodes a wave invalidated are removed before its handlers run
    void DropTimers(const uint32_t* ids, const uint64_t* bits, uint64_t words, uint64_t n);
    void ReportAccess(Computed& c, bool is_new);
    LTag NextVersion(LTag current);
    void MoveSubs(uint32_t from, uint32_t to);
    // `c` is the object its handle names: the slot's current node, or the detached map's entry
    bool Owns(const Computed& c) const;

    fgi_graph* g_ = nullptr;
    fgi_state_view view_{};
    mutable uint64_t calls_ = 0;
    uint32_t n_slots_ = 0, n_handles_ = 0;
    std::unordered_map<std::string, uint32_t> slots_;
    std::vector<std::shared_ptr<Computed>> current_;                 // slot -> newest node
    std::unordered_map<uint32_t, std::shared_ptr<Computed>> detached_;  // detached handle -> node
    std::vector<uint8_t> has_obj_;                                   // handle -> host object exists
    std::vector<uint32_t> scope_roots_;
    std::vector<uint8_t> scope_imm_;
    int scope_depth_ = 0;
    bool async_scope_ = false;               // the outermost open scope flushes asynchronously
    struct Timer {
        TimePoint due;
        LTag version;
        bool is_auto = false;   // fires on a Consistent node whether or not its delay has started
    };
    std::unordered_map<uint32_t, Timer> timers_;   // handle -> its pending delayed invalidation
    bool in_timers_ = false;                 // RunDueTimers is running (its own wave does not re-enter it)
    // DeviceTimers: opened by the first registry call; the engine's clock as last set; a lower bound of its next
    // due time, void (maybe_armed_) once a wave or a displacement may have armed an entry; each slot's delay
    // as the engine holds it
    std::shared_ptr<Computed> BeginComputeImpl(const std::string& input, bool has_delay, const ComputedOptions& options);
    ComputedOptions DefaultOptions(std::chrono::nanoseconds delay) const;
    void EnsureTimers();
    // DeviceTimers: the engine's auto-invalidation opens with the first node that has such a delay
    void EnsureAuto();
    bool dev_auto_ = false;
    std::vector<uint64_t> slot_auto_, slot_transient_;   // each slot's auto delays as the engine holds them (0: none)
    uint64_t NowTicks();
    size_t RunDueTimersDevice();
    bool dev_timers_ = false, maybe_armed_ = false;
    TimePoint epoch_{};
    uint64_t ticks_ = 0, next_due_ = ~0ull;
    std::vector<uint64_t> slot_delay_;
    std::deque<uint64_t> pending_;           // asynchronous waves queued, not yet completed (ticket order)
    uint64_t last_ticket_ = 0;
    LTag ltag_ = 0x100000;
    fgi_wave_stats last_{};
    FanoutStats fan_;
    std::unique_ptr<uint32_t[]> ids_;
    uint64_t ids_cap_ = 0;
    std::unique_ptr<uint64_t[]> bits_;   // the last bitmap-mode wave's invalidated bitmap
    uint64_t pred_v_ = 0;                // the previous wave's V_inv (picks the output form)
    // subscriptions: per handle a singly-linked list in one pool (kNone-terminated), free list
    std::vector<PeerSink> peers_;
    std::vector<uint32_t> sub_head_;
    std::vector<Sub> subs_;
    std::vector<uint32_t> sub_free_;
    bool dev_subs_ = false;     // DeviceFanout: the engine holds subscriptions
    bool from_ticket_ = false;  // the Dispatch about to run fans out an asynchronous ticket's ids
    uint64_t* dev_buf_ = nullptr;   // page-locked: a device fan-out's call ids (and a ticket's handles behind them)
    uint64_t dev_buf_cap_ = 0;      // entries
};

}  // namespace fusion
