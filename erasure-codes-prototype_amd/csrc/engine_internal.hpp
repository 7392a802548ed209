// What crosses the engine's own translation units -- engine.cpp (device tier), program_cache.cpp, batch_scope.cpp,
// host_tier.cpp, host_pipeline.cpp -- and nothing else.  codes.cpp, capi.cpp and the check libraries see engine.hpp.
#pragma once
#include <string.h>

#include "engine.hpp"

#pragma GCC visibility push(hidden)  // internal to libecg: none of this joins its dynamic symbols
namespace ecg {

#define ECG_HIP(call)                                                                        \
    do {                                                                                     \
        hipError_t _e = (call);                                                              \
        if (_e != hipSuccess) {                                                              \
            set_last_error(std::string(#call) + ": " + hipGetErrorString(_e));               \
            return ECG_EHIP;                                                                 \
        }                                                                                    \
    } while (0)

constexpr int kMaxDevices = 64;
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The arguments of a launch of S stripes of B bytes over ps's programs, all else zero.  Every launch site
// starts here and sets only what is its own, so a new GfLaunch field is zero everywhere until a site names it.
inline GfLaunch launch_args(const ProgramSet& ps, long long B, int S) {
    GfLaunch a;
    memset(&a, 0, sizeof(a));
    a.tabs = ps.d_tabs;
    a.src_ids = ps.d_src;
    a.dst_ids = ps.d_dst;
    a.B = B;
    a.k = ps.k;
    a.m = ps.m;
    a.S = S;
    a.MT = ps.MT;
    a.rtiles = ps.rtiles;
    a.binary = ps.binary ? 1 : 0;
    return a;
}

// Makes `dev` the calling thread's device (when it is another) and restores the caller's on the way out.
class DeviceGuard {
public:
    explicit DeviceGuard(int dev) {
        (void)hipGetDevice(&caller_);
        switched_ = caller_ != dev && hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched_) (void)hipSetDevice(caller_);
    }
    DeviceGuard(const DeviceGuard&) = delete;

private:
    int caller_ = -1;
    bool switched_ = false;
};

// Host-tier state: a non-blocking stream, a growable device scratch, a pinned staging area and the
// host-batch pipeline's streams and slots.  Contexts are pooled per device and LEASED for the duration
// of one synchronous host-tier call, so these resources are bounded by the number of calls in flight
// at once -- not by the number of threads that ever called.  (The reference's proxy runs every SET on
// a new detached thread, proxy.cpp:416-419; per-thread state would leak a stream, scratch and pinned
// memory per request.)  Contexts live for the process.
struct HostCtx {
    hipStream_t stream = nullptr;
    uint8_t* scratch = nullptr;
    size_t cap = 0;
    // host-batch pipeline: 3 streams, 3 device slots
    hipStream_t pstream[3] = {nullptr, nullptr, nullptr};
    hipEvent_t in_done[3] = {}, comp_done[3] = {}, out_done[3] = {};
    bool pipe_ready = false;
    uint8_t* pslot = nullptr;
    size_t pslot_cap = 0;
    // small host calls: one pinned staging area mirroring the device scratch
    uint8_t* pinned = nullptr;      // host view
    uint8_t* pinned_dev = nullptr;  // device view (mapped, fine-grained)
    size_t pinned_cap = 0;
    // zero-copy calls: completion flags the kernels post and the host polls (mapped, fine-grained)
    unsigned* flags = nullptr;
    unsigned* flags_dev = nullptr;
    unsigned seq = 0;
    unsigned unreaped = 0;  // flagged calls since the stream was last queried
};
constexpr int kFlagSlots = 4096;

class CtxLease {  // host_tier.cpp holds the pool
public:
    explicit CtxLease(int device);
    ~CtxLease();
    CtxLease(const CtxLease&) = delete;
    CtxLease& operator=(const CtxLease&) = delete;
    HostCtx& operator*() { return *c_; }
    int done() {  // the call completed and synchronised its streams
        idle_ = true;
        return ECG_OK;
    }

private:
    int dev_;
    HostCtx* c_;
    bool idle_ = false;
};

// batch_scope.cpp
bool strided_side(const std::vector<const uint8_t* const*>& calls, const std::vector<int>& ids, const uint8_t*& base,
                  long long& sstride, long long& bstride, std::vector<int>& v);

// The calling thread's scope (engine.hpp: batch_begin and the rest).
struct DeferScope {
    bool active = false;
    std::vector<DeferredCall> q;
    ScratchRanges scratch;
    FlushStats stats;
    // the stream and device of the last group the scope launched: a scope flushes several times (every
    // kEagerFlush calls, before a host-tier call, on ecg_batch_flush), and the first group of a flush must
    // wait for the previous flush's last group when it runs on another stream.  That stream is compared,
    // never named: the caller may have destroyed it since (profiles/r04/stream/), so a flush that leaves the
    // scope open records the ordering event behind its last group before it returns (last_recorded).
    hipStream_t last_st = nullptr;
    int last_dev = -1;
    bool last_recorded = false;
    // ordering events, one per device the scope launched on, leased from that device's engine pool for the
    // scope and returned at its end (or at thread exit): none is held per thread between scopes
    std::vector<std::pair<Engine*, hipEvent_t>> order_evs;
    hipEvent_t order_ev(int dev) {
        for (auto& e : order_evs)
            if (e.first->device() == dev) return e.second;
        return nullptr;
    }
    void release_order_evs() {
        for (auto& e : order_evs) e.first->release_event(e.second);
        order_evs.clear();
    }
    // Deferred HOST-tier calls (ecg_batch_defer_host): a call's input blocks are copied into the pinned
    // staging of a host context leased for the scope when the call is made (region A, one slot per block
    // read before written); its outputs get slots in region W and reach the caller's buffers at the flush.
    // The flush moves region A in ONE H2D copy, launches the calls grouped by plan, moves W back in ONE D2H
    // copy and scatters it -- the synchronous per-call round trip (launch + completion + two copies) is paid
    // once per flush instead of once per call.  At most one of the two queues (device-tier q, host-tier hq)
    // holds calls at any time: recording into one flushes the other first.
    bool host_defer = false;
    struct HostCall {
        Engine* eng;
        std::shared_ptr<const std::vector<LinearOp>> ops;
        std::vector<uint8_t*> host;  // the caller's block pointers
        std::vector<int> slot;       // >= 0: region-A slot; <= -2: region-W slot -2 - slot; -1: unused
        std::vector<int> wr;         // block ids the call writes
    };
    std::vector<HostCall> hq;
    int h_up = 0, h_w = 0;
    long long h_B = -1;
    bool h_inplace = false;  // a written block has a region-A slot (read, then written)
    PtrGroups h_out;         // pending output blocks by B-byte bucket (pending_output_overlaps), open addressing
    size_t h_nout = 0;       // entries in h_out (a block is written at most once per batch: a second write flushes)
    std::unique_ptr<CtxLease> h_ctx;
    ~DeferScope() { release_order_evs(); }
};

constexpr size_t kMaxDeferred = 1 << 16;  // calls recorded before an automatic flush
// Without declared scratch, a flush of the calls recorded so far changes nothing but where groups are
// cut, so the scope flushes every kEagerFlush calls: the GPU runs the first calls while the host records
// the rest, instead of idling until the scope ends.  (With scratch, a flush would write pending scratch
// contents for real; such scopes flush only at kMaxDeferred.)
constexpr size_t kEagerFlush = 1024;

// Defined in engine.cpp beside run_device, its hottest reader: a thread_local with a destructor is reached
// from another translation unit through a wrapper call, which every device-tier call would then pay.  The
// host tier (a call of ~10 us) and the flushes take one reference per call instead.
extern thread_local DeferScope t_defer;

inline size_t flush_at(const DeferScope& d) { return d.scratch.empty() ? kEagerFlush : kMaxDeferred; }

}  // namespace ecg
#pragma GCC visibility pop
