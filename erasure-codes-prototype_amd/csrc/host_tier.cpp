// GF(2^8) region engine, host tier: calls whose blocks are host memory.  The pooled contexts such calls lease,
// the calls a batch scope defers (record_host, host_flush) and the synchronous call with its staging, zero-copy
// flags and resident call worker (run_host).  The pipeline for host-resident batches is in host_pipeline.cpp.
#include <emmintrin.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <thread>

#include "engine_internal.hpp"

namespace ecg {

namespace {

std::mutex g_ctx_mu[kMaxDevices];
// never destroyed (process lifetime, like the engines): no teardown-order hazard with late callers
std::vector<HostCtx*>* const g_ctx_free = new std::vector<HostCtx*>[kMaxDevices];
int g_ctx_created[kMaxDevices] = {};

}  // namespace

CtxLease::CtxLease(int device) : dev_(device) {
    std::lock_guard<std::mutex> lk(g_ctx_mu[dev_]);
    if (!g_ctx_free[dev_].empty()) {
        c_ = g_ctx_free[dev_].back();
        g_ctx_free[dev_].pop_back();
    } else {
        c_ = new HostCtx();
        g_ctx_created[dev_]++;
    }
}

CtxLease::~CtxLease() {
    if (!idle_) {
        // a call that failed part-way may have left copies in flight: drain before the next lessee
        if (c_->stream) (void)hipStreamSynchronize(c_->stream);
        for (hipStream_t s : c_->pstream)
            if (s) (void)hipStreamSynchronize(s);
    }
    std::lock_guard<std::mutex> lk(g_ctx_mu[dev_]);
    g_ctx_free[dev_].push_back(c_);
}

int Engine::host_contexts() const {
    std::lock_guard<std::mutex> lk(g_ctx_mu[device_]);
    return g_ctx_created[device_];
}

// ------------------------------------------------------------------------------------------------
// Deferred host-tier calls (DeferScope::hq; ecg_batch_defer_host).

namespace {

// Copy a call's input block into the scope's pinned staging with non-temporal stores.  Region A of a
// host batch grows to tens of MiB (4096 RS(6,4) 4 KiB stripes: 96 MiB), far past the caches, and ordinary
// stores pay a read-for-ownership of every destination line: the plain memcpy moved 7.8 GB/s and was most
// of a recorded call's 3.2 us (tools/defer_cost.cpp, profiles/r04/small_host/).  The flush issues an
// sfence before the H2D copy reads the region.  dst is 256-byte aligned (the slot pitch).
void stream_copy(uint8_t* dst, const uint8_t* src, size_t n) {
    size_t i = 0;
    if (((uintptr_t)dst & 15) == 0)
        for (; i + 64 <= n; i += 64) {
            const __m128i a = _mm_loadu_si128((const __m128i*)(src + i));
            const __m128i b = _mm_loadu_si128((const __m128i*)(src + i + 16));
            const __m128i c = _mm_loadu_si128((const __m128i*)(src + i + 32));
            const __m128i d = _mm_loadu_si128((const __m128i*)(src + i + 48));
            _mm_stream_si128((__m128i*)(dst + i), a);
            _mm_stream_si128((__m128i*)(dst + i + 16), b);
            _mm_stream_si128((__m128i*)(dst + i + 32), c);
            _mm_stream_si128((__m128i*)(dst + i + 48), d);
        }
    if (i < n) memcpy(dst + i, src + i, n - i);
}

constexpr size_t kHostDeferMaxBytes = 64 << 20;  // staging (regions A + W) of one host batch

// Pinned staging of a context with room for `bytes`, keeping its first `keep` bytes.  `amortise`: grow to at
// least twice the old size (region A of a deferred batch grows call by call); a single call sizes it exactly.
int ensure_pinned(HostCtx& c, size_t bytes, size_t keep, bool amortise) {
    if (c.pinned_cap >= bytes) return ECG_OK;
    const size_t cap = std::max(bytes, std::max(amortise ? c.pinned_cap * 2 : 0, (size_t)1 << 20));
    uint8_t* p = nullptr;
    uint8_t* pd = nullptr;
    ECG_HIP(hipHostMalloc((void**)&p, cap, hipHostMallocMapped | hipHostMallocCoherent));
    if (hipHostGetDevicePointer((void**)&pd, p, 0) != hipSuccess) {
        (void)hipHostFree(p);
        set_last_error("hipHostGetDevicePointer(host batch staging) failed");
        return ECG_EHIP;
    }
    if (keep && c.pinned) memcpy(p, c.pinned, keep);
    if (c.pinned) {
        if (c.stream) (void)hipStreamSynchronize(c.stream);
        (void)hipHostFree(c.pinned);
    }
    c.pinned = p;
    c.pinned_dev = pd;
    c.pinned_cap = cap;
    return ECG_OK;
}

// Device scratch of a context with room for `bytes` (contents are not kept).  hipSuccess, or the error of the
// call that failed: *in_alloc says whether that was the hipMalloc or the drain of the stream before it (the
// synchronous call and the deferred batch report the two in their own words).
hipError_t ensure_scratch(HostCtx& c, size_t bytes, bool* in_alloc) {
    *in_alloc = false;
    if (c.cap >= bytes) return hipSuccess;
    hipError_t e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) return e;
    if (c.scratch) (void)hipFree(c.scratch);
    c.scratch = nullptr;
    c.cap = 0;
    *in_alloc = true;
    if ((e = hipMalloc(&c.scratch, bytes)) == hipSuccess) c.cap = bytes;
    return e;
}

void host_queue_reset() {
    DeferScope& d = t_defer;
    d.hq.clear();
    if (d.h_nout) d.h_out.reset(0);
    d.h_nout = 0;
    d.h_up = d.h_w = 0;
    d.h_B = -1;
    d.h_inplace = false;
    d.h_ctx.reset();  // a context whose batch did not complete drains its streams before its next lessee
}

// Pending outputs of the deferred host batch, compared by BYTE RANGE (host blocks of one scope
// may be offsets into one caller buffer).  Every pending output is [p, p + B) with the batch's one block
// size, and pending outputs are pairwise disjoint (a call touching one flushes first), so a B-byte bucket
// holds the start of at most one: h_out maps bucket p / B + 1 to wr = 1 and rd = p % B.  A block [a, a + B)
// overlaps a pending output iff one starts in bucket a / B - 1, a / B or a / B + 1 within B bytes of a.
void note_pending_output(DeferScope& d, const void* blk, long long B) {
    if (B <= 0) return;  // an empty block overlaps nothing
    const uintptr_t p = (uintptr_t)blk, b = (uintptr_t)B;
    GroupMark& s = d.h_out.at((const void*)(p / b + 1));
    s.wr = 1;
    s.rd = (int)(p % b);
}

bool pending_output_overlaps(const DeferScope& d, const void* blk, long long B) {
    if (B <= 0) return false;
    const uintptr_t a = (uintptr_t)blk, b = (uintptr_t)B, q = a / b;
    for (uintptr_t k = q ? q - 1 : 0; k <= q + 1; k++) {
        const GroupMark* s = d.h_out.find((const void*)(k + 1));
        if (!s || !s->wr) continue;
        const uintptr_t p = k * b + (uintptr_t)s->rd;
        if ((p > a ? p - a : a - p) < b) return true;
    }
    return false;
}

}  // namespace

// Record one host-tier call of an open scope with host deferral on.  Returns ECG_OK (recorded), a negative
// status, or 1: not deferrable (blocks above kStagedMaxBlock, or the call alone overflows the staging) --
// the caller runs it synchronously after flushing.  A call whose blocks overlap a pending output of an
// earlier recorded call (by byte range, pending_output_overlaps), or with another block size or engine,
// flushes the batch first.
int record_host(Engine* eng, const std::vector<LinearOp>& ops, uint8_t* const* blocks, int nblocks, long long B) {
    DeferScope& d = t_defer;
    if (B > (long long)kStagedMaxBlock) return 1;
    thread_local BlockUse use;
    if (const int rc = use.classify(ops, blocks, nblocks); rc != ECG_OK) return rc;
    const std::vector<char>&upload = use.upload, &written = use.written, &used = use.used;
    int nup = 0, nw = 0;
    for (int id = 0; id < nblocks; id++) {
        nup += upload[id];
        nw += used[id] && !upload[id];
    }
    const size_t pitch = ((size_t)B + 255) & ~(size_t)255;
    if ((size_t)(nup + nw) * pitch > kHostDeferMaxBytes) return 1;
    if (!d.q.empty())
        if (const int rc = batch_flush(); rc != ECG_OK) return rc;  // at most one queue holds calls
    bool flush = !d.hq.empty() && (d.h_B != B || d.hq.back().eng != eng ||
                                   (size_t)(d.h_up + d.h_w + nup + nw) * pitch > kHostDeferMaxBytes);
#ifndef ECG_TEST_NO_HOST_HAZARD_FLUSH  // test hook: a variant without this flush must fail the random-sequence test
    for (int id = 0; id < nblocks && !flush && d.h_nout; id++)
        flush = used[id] && pending_output_overlaps(d, blocks[id], B);
#endif
    if (flush)
        if (const int rc = host_flush(); rc != ECG_OK) return rc;
    if (!d.h_ctx) {
        d.h_ctx = std::make_unique<CtxLease>(eng->device());
        HostCtx& c = **d.h_ctx;
        if (!c.stream && hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking) != hipSuccess) {
            host_queue_reset();
            set_last_error("hipStreamCreate(host batch) failed");
            return ECG_EHIP;
        }
        d.h_B = B;
    }
    HostCtx& c = **d.h_ctx;
    if (const int rc = ensure_pinned(c, (size_t)(d.h_up + nup) * pitch, (size_t)d.h_up * pitch, true); rc != ECG_OK) {
        host_queue_reset();
        return rc;
    }
    DeferScope::HostCall call;
    call.eng = eng;
    call.host.assign(blocks, blocks + nblocks);
    call.slot.assign(nblocks, -1);
    call.wr.reserve(nblocks);
    for (int id = 0; id < nblocks; id++) {
        if (upload[id]) {
            call.slot[id] = d.h_up;
            stream_copy(c.pinned + (size_t)d.h_up * pitch, blocks[id], (size_t)B);  // inputs read at call time
            d.h_up++;
        } else if (used[id]) {
            call.slot[id] = -2 - d.h_w++;
        }
        if (written[id]) {
            call.wr.push_back(id);
            note_pending_output(d, blocks[id], B);
            d.h_nout++;
            d.h_inplace |= upload[id] != 0;
        }
    }
    if (!d.hq.empty() && same_ops(*d.hq.back().ops, ops)) call.ops = d.hq.back().ops;
    else call.ops = std::make_shared<const std::vector<LinearOp>>(ops);
    d.hq.push_back(std::move(call));
    return ECG_OK;
}

// Run the recorded host-tier calls: one H2D of region A, the calls' launches grouped by plan (consecutive
// calls with one plan: one strided or pointer-table launch per op), one D2H of region W (and of A when a
// call wrote a block it had read), then the outputs copied into the caller's buffers.  The queue is
// emptied whatever happens; on an error the outputs of this batch are undefined.
int host_flush() {
    DeferScope& d = t_defer;
    if (d.hq.empty()) return ECG_OK;
    // The batch is taken out of the scope first: the launches below go through entry points that flush
    // pending calls (run_strided), which must find nothing to flush.
    struct Batch {
        std::vector<DeferScope::HostCall> hq;
        std::unique_ptr<CtxLease> ctx;  // drains the context's streams on every way out but the last
    } bt;
    bt.hq.swap(d.hq);
    bt.ctx = std::move(d.h_ctx);
    const int h_up = d.h_up, h_w = d.h_w;
    const bool h_inplace = d.h_inplace;
    const long long B = d.h_B;
    host_queue_reset();
    HostCtx& c = **bt.ctx;
    hipStream_t st = c.stream;
    Engine* eng = bt.hq[0].eng;
    const size_t pitch = ((size_t)B + 255) & ~(size_t)255;
    const size_t a_bytes = (size_t)h_up * pitch, total = (size_t)(h_up + h_w) * pitch;
    DeviceGuard on_device(eng->device());
    bool in_alloc = false;
    if (ensure_scratch(c, total, &in_alloc) != hipSuccess) {
        if (in_alloc) set_last_error("hipMalloc(host batch scratch) failed");
        return ECG_EHIP;
    }
    if (const int rc = ensure_pinned(c, total, a_bytes, true); rc != ECG_OK) return rc;
    _mm_sfence();  // the region's non-temporal stores (stream_copy) are globally visible before the DMA reads it
    if (a_bytes && hipMemcpyAsync(c.scratch, c.pinned, a_bytes, hipMemcpyHostToDevice, st) != hipSuccess) {
        set_last_error("hipMemcpyAsync(host batch H2D) failed");
        return ECG_EHIP;
    }
    const size_t n = bt.hq.size();
    thread_local std::vector<uint8_t*> dptr;
    thread_local std::vector<size_t> first;
    first.resize(n + 1);
    size_t tot = 0;
    for (size_t i = 0; i < n; i++) {
        first[i] = tot;
        tot += bt.hq[i].slot.size();
    }
    first[n] = tot;
    dptr.assign(tot, nullptr);
    for (size_t i = 0; i < n; i++) {
        const auto& sl = bt.hq[i].slot;
        for (size_t id = 0; id < sl.size(); id++) {
            const int v = sl[id];
            if (v >= 0) dptr[first[i] + id] = c.scratch + (size_t)v * pitch;
            else if (v <= -2) dptr[first[i] + id] = c.scratch + a_bytes + (size_t)(-2 - v) * pitch;
        }
    }
    // Calls of one shape -- the same number of ops, and per op the same (k_in, m_out) -- form one group
    // whatever their coefficients (per-stripe decodes of different erasure patterns): the calls of a host
    // batch touch disjoint staging slots, so any grouping keeps each call's own op order.  Per op, a group
    // with one plan goes out as a strided launch (or a pointer table); mixed plans as ONE pointer-table
    // launch with a program per matrix (run_ptr_batch_multi).
    auto shape_of = [&](size_t i) {
        std::vector<int> sig;
        for (const LinearOp& op : *bt.hq[i].ops) {
            sig.push_back(op.k_in());
            sig.push_back(op.m_out());
        }
        return sig;
    };
    std::map<std::vector<int>, std::vector<size_t>> groups;
    for (size_t i = 0; i < n; i++) groups[shape_of(i)].push_back(i);
    int rc = ECG_OK;
    std::vector<const uint8_t* const*> calls;
    std::vector<const LinearOp*> per_call;
    for (auto& kv : groups) {
        const std::vector<size_t>& G = kv.second;
        if (G.size() == 1) {
            rc = eng->launch_direct(*bt.hq[G[0]].ops, dptr.data() + first[G[0]], B, st);
            if (rc != ECG_OK) break;
            continue;
        }
        calls.clear();
        for (size_t i : G) calls.push_back(dptr.data() + first[i]);
        const size_t nops = bt.hq[G[0]].ops->size();
        for (size_t o = 0; o < nops && rc == ECG_OK; o++) {
            const LinearOp& op0 = (*bt.hq[G[0]].ops)[o];
            bool one_plan = true;
            for (size_t i : G) one_plan &= bt.hq[i].ops.get() == bt.hq[G[0]].ops.get();
            if (op0.k_in() == 0) {  // composed row of zeros: the library writes zero bytes
                for (size_t i : G)
                    if (rc == ECG_OK) rc = eng->launch_direct({(*bt.hq[i].ops)[o]}, dptr.data() + first[i], B, st);
            } else if (one_plan) {
                bool done = false;
                rc = eng->run_calls_strided(op0, calls, B, st, &done);
                if (rc == ECG_OK && !done) rc = eng->run_ptr_batch(op0, calls, B, st);
            } else {
                per_call.clear();
                for (size_t i : G) per_call.push_back(&(*bt.hq[i].ops)[o]);
                rc = eng->run_ptr_batch_multi(per_call, calls, B, st);
            }
        }
        if (rc != ECG_OK) break;
    }
    if (rc != ECG_OK) return rc;
    if (h_w && hipMemcpyAsync(c.pinned + a_bytes, c.scratch + a_bytes, total - a_bytes, hipMemcpyDeviceToHost, st) !=
                     hipSuccess) {
        set_last_error("hipMemcpyAsync(host batch D2H) failed");
        return ECG_EHIP;
    }
    if (h_inplace && hipMemcpyAsync(c.pinned, c.scratch, a_bytes, hipMemcpyDeviceToHost, st) != hipSuccess) {
        set_last_error("hipMemcpyAsync(host batch D2H) failed");
        return ECG_EHIP;
    }
    if (hipStreamSynchronize(st) != hipSuccess) {
        set_last_error("hipStreamSynchronize(host batch) failed");
        return ECG_EHIP;
    }
    for (const DeferScope::HostCall& call : bt.hq)
        for (int id : call.wr) {
            const int v = call.slot[id];
            const size_t off = v >= 0 ? (size_t)v * pitch : a_bytes + (size_t)(-2 - v) * pitch;
            memcpy(call.host[id], c.pinned + off, (size_t)B);
        }
    bt.ctx->done();
    return ECG_OK;
}

// The context's completion-flag page (zero-copy host calls), allocated on first use.
static bool flags_ready(HostCtx& c) {
    if (c.flags) return true;
    if (hipHostMalloc((void**)&c.flags, kFlagSlots * sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent) !=
        hipSuccess) {
        (void)hipGetLastError();
        c.flags = nullptr;
        return false;
    }
    if (hipHostGetDevicePointer((void**)&c.flags_dev, c.flags, 0) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipHostFree(c.flags);
        c.flags = nullptr;
        return false;
    }
    memset(c.flags, 0, kFlagSlots * sizeof(unsigned));
    return true;
}

// Poll flags[0, n) until each holds seq (spinning for the first 200 us, then yielding the core between
// polls).  A flag that does not arrive within 100 ms hands over to the
// stream (a fault is reported there; a slow launch just finishes).  Every 64 flagged calls the stream is
// queried so that the runtime retires the completed launches it never waited for.
static int wait_flags(HostCtx& c, int n, unsigned seq, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n; i++) {
        while (__atomic_load_n(&c.flags[i], __ATOMIC_ACQUIRE) != seq) {
            const auto waited = std::chrono::steady_clock::now() - t0;
            if (waited < std::chrono::microseconds(200))
                __builtin_ia32_pause();
            else
                std::this_thread::yield();  // queued behind other work: stop burning the core
            if (waited > std::chrono::milliseconds(100)) {
                ECG_HIP(hipStreamSynchronize(st));
                for (int j = i; j < n; j++)
                    if (__atomic_load_n(&c.flags[j], __ATOMIC_ACQUIRE) != seq) {
                        set_last_error("zero-copy call: a completion flag never arrived");
                        return ECG_EHIP;
                    }
                c.unreaped = 0;
                return ECG_OK;
            }
        }
    }
    if (++c.unreaped >= 64) {
        c.unreaped = 0;
        const hipError_t e = hipStreamQuery(st);
        if (e != hipSuccess && e != hipErrorNotReady) {
            set_last_error(std::string("hipStreamQuery: ") + hipGetErrorString(e));
            return ECG_EHIP;
        }
    }
    return ECG_OK;
}

namespace {

// Resident call worker of a device (ECG_OPT_CALL_WORKER > 0; gf_kernels.hpp WorkerArgs).
// A small synchronous host-tier call normally pays a kernel launch (~4 us of an ~11 us RS(6,4) 1 KiB call);
// with the worker, a resident kernel polls a descriptor ring in pinned host memory and the call only
// writes its descriptor (profiles/r03/persist/persist_probe.hip: 11.4 -> 4.9 us).  One call at a time goes through it
// (try_lock): concurrent callers take the launch path, so concurrency is never serialised behind it.
// The worker runs on a HIGH-PRIORITY stream: HIP maps streams onto a few hardware queues, and a kernel
// that stays resident on a queue shared with another stream holds that stream's work behind it until it
// exits (measured: 28 ms for one of 8 normal streams, none with the worker on a high-priority stream;
// profiles/r03/persist/queue_interference.log).  A process that issues its own work on high-priority
// streams shares that queue -- hence the option is off by default.  The worker exits by itself after the
// option's idle time without a call, takes no call after 50 ms (the waiting call then starts the next
// generation, so the queue is released at least that often), and stops at process exit.
struct CallWorker {
    static constexpr double kLifeMs = 50.0;
    std::mutex mu;
    bool ready = false, broken = false, running = false;
    int device = 0;
    hipStream_t st = nullptr;
    uint8_t* host = nullptr;  // pinned, mapped: ring [0, 1024), flags [1024, 1280), stop @2048, exit_info @2112
    uint8_t* host_dev = nullptr;
    uint8_t* dmem = nullptr;  // device: mailbox [0, 1024), mailbox seqs + exit word @1024
    unsigned seq = 0, gen = 0;
    int W = 0;
    unsigned long long ticks_per_us = 100;
    long long idle_us = 0, gen_idle_us = 0;  // the option now / the running generation's idle limit
    long long calls = 0, launches = 0, relaunches = 0;
    // A call that does not complete within 100 ms (queued behind a long kernel, e.g.) turns the worker off
    // for a cooldown that doubles per consecutive timeout (1 s .. 64 s); calls take the launch path meanwhile.
    // `broken` stays for what cannot recover: initialisation failed.
    std::chrono::steady_clock::time_point off_until{};
    int timeouts_in_row = 0;
    long long timeouts = 0;
    bool cooling() const { return std::chrono::steady_clock::now() < off_until; }
    void back_off() {
        timeouts++;
        const int sh = std::min(timeouts_in_row++, 6);
        off_until = std::chrono::steady_clock::now() + std::chrono::seconds(1LL << sh);
    }

    WorkerDesc* ring() { return (WorkerDesc*)host; }
    unsigned* flags() { return (unsigned*)(host + 1024); }
    volatile unsigned* stopw() { return (volatile unsigned*)(host + 2048); }
    unsigned* exit_info() { return (unsigned*)(host + 2112); }

    bool init(int dev) {
        device = dev;
        int lo = 0, hi = 0, khz = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) return false;
        if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi) != hipSuccess) return false;
        if (hipHostMalloc((void**)&host, 4096, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return false;
        if (hipHostGetDevicePointer((void**)&host_dev, host, 0) != hipSuccess) return false;
        memset(host, 0, 4096);
        if (hipMalloc((void**)&dmem, 2048) != hipSuccess) return false;
        if (hipMemsetAsync(dmem, 0, 2048, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return false;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) return false;
        ticks_per_us = (unsigned long long)khz / 1000ULL;
        if (ticks_per_us == 0) ticks_per_us = 1;
        ready = true;
        return true;
    }
    // every workgroup of the current generation has exited (it writes `gen` as it leaves)
    bool gone() {
        if (!running) return true;
        for (int w = 0; w < W; w++)
            if (__atomic_load_n(&exit_info()[w], __ATOMIC_ACQUIRE) != gen) return false;
        running = false;
        return true;
    }
    // Start a generation at call `start` (only while none is running).  The call's flags are cleared first:
    // a generation that left (or was stopped) may have posted some of them for this very call, and the new
    // one redoes the call from the start.  Flags left over from it would let the host finish the call
    // while a workgroup of the new generation still rewrites the call's outputs -- into staging memory
    // the host hands to the next call (seen as a wrong decode in the 8-thread x 2000 soak, where call
    // sizes change and generations are restarted often).
    int launch(int workgroups, unsigned start) {
        unsigned* f = flags() + (start % kWorkerSlots) * kWorkerMaxWG;
        for (int w = 0; w < kWorkerMaxWG; w++) __atomic_store_n(&f[w], 0u, __ATOMIC_RELAXED);
        WorkerArgs a;
        memset(&a, 0, sizeof a);
        if (++gen == 0) ++gen;
        a.ring = (const WorkerDesc*)host_dev;
        a.flags = (unsigned*)(host_dev + 1024);
        a.stop = (const unsigned*)(host_dev + 2048);
        a.mbox = (WorkerDesc*)dmem;
        a.mbseq = (unsigned*)(dmem + 1024);
        a.exit_info = (unsigned*)(host_dev + 2112);
        a.start_seq = start;
        a.gen = gen;
        a.max_polls = 1u << 24;
        a.idle_ticks = (unsigned long long)idle_us * ticks_per_us;
        a.life_ticks = (unsigned long long)(kLifeMs * 1000.0) * ticks_per_us;
        *stopw() = 0;
        const hipError_t e = launch_call_worker(a, workgroups, st);
        if (e != hipSuccess) {
            set_last_error(std::string("call worker launch: ") + hipGetErrorString(e));
            return ECG_EHIP;
        }
        W = workgroups;
        gen_idle_us = idle_us;
        running = true;
        launches++;
        return ECG_OK;
    }
    // stop the running generation and wait until it is gone (bounded: it exits at its next poll)
    int stop() {
        if (!running) return ECG_OK;
        *stopw() = 1;
        const auto t0 = std::chrono::steady_clock::now();
        while (!gone()) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
                if (hipStreamSynchronize(st) != hipSuccess) return ECG_EHIP;
                running = false;
                break;
            }
            __builtin_ia32_pause();
        }
        *stopw() = 0;
        return ECG_OK;
    }
    bool done(unsigned slot, unsigned s) {
        const unsigned* f = flags() + slot * kWorkerMaxWG;
        for (int w = 0; w < W; w++)
            if (__atomic_load_n(&f[w], __ATOMIC_ACQUIRE) != s) return false;
        return true;
    }
    // One call: 0 = done, 1 = not taken (use the launch path), < 0 = error.
    int call(int dev_id, const ProgramSet& ps, const LinearOp& op, uint8_t* const* dev, long long B) {
        if (broken || cooling()) return 1;
        if (!ready && !init(dev_id)) {
            broken = true;
            return 1;
        }
        idle_us = get_option(ECG_OPT_CALL_WORKER);
        const int need = (int)std::max(1LL, ((B >> 2) + kLatThreads - 1) / kLatThreads);
        if (need > kWorkerMaxWG) return 1;
        unsigned s = ++seq;
        if (s == 0) s = ++seq;
        const unsigned slot = s % kWorkerSlots;
        // payload, then the four sequence numbers (x86 stores become visible in program order)
        WorkerDesc& d = ring()[slot];
        unsigned pay[60] = {};
        pay[WF_K] = (unsigned)op.k_in();
        pay[WF_M] = (unsigned)op.m_out();
        pay[WF_B] = (unsigned)B;
        pay[WF_BINARY] = ps.binary ? 1u : 0u;
        auto put64 = [&](int q, const void* p) {
            pay[q] = (unsigned)(uintptr_t)p;
            pay[q + 1] = (unsigned)((uintptr_t)p >> 32);
        };
        put64(WF_TABS, ps.d_tabs);
        for (int j = 0; j < op.k_in(); j++) put64(WF_IN + 2 * j, dev[op.src_ids[j]]);
        for (int p = 0; p < op.m_out(); p++) put64(WF_OUT + 2 * p, dev[op.dst_ids[p]]);
        for (int q = 0; q < 60; q++) d.w[worker_pos(q)] = pay[q];
        std::atomic_thread_fence(std::memory_order_release);
        for (int l = 0; l < 4; l++) __atomic_store_n(&d.w[16 * l], s, __ATOMIC_RELEASE);
        // a generation too narrow for this call, or started under another idle limit, makes way for a new one
        if (!gone() && (W < need || gen_idle_us != idle_us) && stop() != ECG_OK) return ECG_EHIP;
        if (!running && launch(std::max(need, 1), s) != ECG_OK) {
            back_off();
            return 1;
        }
        const auto t0 = std::chrono::steady_clock::now();
        auto next_check = t0 + std::chrono::microseconds(20);
        while (!done(slot, s)) {
            const auto t = std::chrono::steady_clock::now();
            if (t > next_check) {
                next_check = t + std::chrono::microseconds(20);
                if (gone() && !done(slot, s)) {  // the generation left before taking the call: a new one takes it
                    relaunches++;
                    if (launch(std::max(need, W), s) != ECG_OK) {
                        back_off();
                        return 1;
                    }
                }
            }
            if (t - t0 > std::chrono::milliseconds(100)) {
                // the generation is gone once stopped and its stream drained; a call it did not finish takes
                // the launch path (its outcome is that path's status, so no error is recorded here)
                (void)stop();
                (void)hipStreamSynchronize(st);
                back_off();
                if (!done(slot, s)) return 1;
                calls++;
                return 0;
            }
            if (t - t0 > std::chrono::microseconds(200)) std::this_thread::yield();
            else __builtin_ia32_pause();
        }
        calls++;
        timeouts_in_row = 0;
        return 0;
    }
};

CallWorker g_worker[kMaxDevices];

// At process exit: tell running workers to stop (a store to pinned host memory) and wait briefly for them
// to leave -- no HIP call, the runtime may already be going down.  They would leave by themselves within
// their idle time anyway.
struct WorkerReaper {
    ~WorkerReaper() {
        for (CallWorker& w : g_worker) {
            // a thread still inside a call (detached threads run on during exit) keeps its worker: that
            // generation leaves by itself within its idle time
            std::unique_lock<std::mutex> lk(w.mu, std::try_to_lock);
            if (!lk.owns_lock() || !w.ready || !w.running) continue;
            *w.stopw() = 1;
            const auto t0 = std::chrono::steady_clock::now();
            while (!w.gone() && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(20)) __builtin_ia32_pause();
        }
    }
} g_worker_reaper;

}  // namespace

int call_worker_stats(long long* calls, long long* launches, long long* relaunches, int* disabled) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= kMaxDevices) return ECG_EINVAL;
    CallWorker& w = g_worker[dev];
    std::lock_guard<std::mutex> lk(w.mu);
    if (calls) *calls = w.calls;
    if (launches) *launches = w.launches;
    if (relaunches) *relaunches = w.relaunches;
    if (disabled) *disabled = (w.broken || w.cooling()) ? 1 : 0;
    return ECG_OK;
}

// Host-buffer tier (the reference's per-stripe calls on host memory).  Device slots are assigned to the
// blocks that must be uploaded first (read before any op writes them), then to the rest, so the
// inputs form one contiguous range.  Small calls (the proxy's 1 KiB - 64 KiB blocks) gather those
// inputs into the leased context's pinned staging area with memcpy and move them with ONE H2D copy, and bring
// every written block back with ONE D2H copy: two DMA transfers per call instead of one pageable copy
// per block (each pageable copy is a driver-staged round trip).  Large calls copy block by block.
int Engine::run_host(const std::vector<LinearOp>& ops, uint8_t* const* blocks, int nblocks, long long B) {
    if (B < 0) return ECG_EINVAL;
    if (const DeferScope& d = t_defer; d.active && d.host_defer && !ops.empty() && B > 0) {
        const int rc = record_host(this, ops, blocks, nblocks, B);
        if (rc <= 0) return rc;  // recorded (or refused); 1 = not deferrable: run it now, below
    }
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;  // keep call order with recorded calls
    if (ops.empty() || B == 0) return ECG_OK;
    CtxLease lease(device_);
    HostCtx& c = *lease;
    if (!c.stream) ECG_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    hipStream_t st = c.stream;
    // per-call bookkeeping in per-thread buffers (a 1 KiB call costs ~10 us of which the host's share is
    // what allocation would add to)
    thread_local BlockUse use;
    thread_local std::vector<int> slot;
    thread_local std::vector<uint8_t*> dev;
    if (const int rc = use.classify(ops, blocks, nblocks); rc != ECG_OK) return rc;
    const std::vector<char>&upload = use.upload, &written = use.written, &used = use.used;
    slot.assign(nblocks, -1);
    int nslots = 0, n_up = 0;
    for (int id = 0; id < nblocks; id++)
        if (upload[id]) slot[id] = nslots++;
    n_up = nslots;
    for (int id = 0; id < nblocks; id++)
        if (used[id] && slot[id] < 0) slot[id] = nslots++;
    const size_t pitch = ((size_t)B + 255) & ~(size_t)255;
    bool in_alloc = false;
    if (const hipError_t e = ensure_scratch(c, pitch * nslots, &in_alloc); e != hipSuccess) {
        const char* what = in_alloc ? "hipMalloc(&c.scratch, pitch * nslots): " : "hipStreamSynchronize(st): ";
        set_last_error(std::string(what) + hipGetErrorString(e));
        return ECG_EHIP;
    }
    dev.assign(nblocks, nullptr);
    for (int id = 0; id < nblocks; id++)
        if (slot[id] >= 0) dev[id] = c.scratch + (size_t)slot[id] * pitch;
    const bool staged = (size_t)B <= kStagedMaxBlock && pitch * nslots <= kStagedMaxBytes;
    if (staged)
        if (const int rc = ensure_pinned(c, pitch * nslots, 0, false); rc != ECG_OK) return rc;
    // zero-copy: the kernel streams the (tiny) blocks straight over PCIe from / to the mapped staging area
    const long long zc_max = get_option(ECG_OPT_ZEROCOPY_BYTES);
    if (staged && zc_max > 0 && (long long)(pitch * nslots) <= zc_max) {
        for (int id = 0; id < nblocks; id++) {
            if (slot[id] < 0) continue;
            dev[id] = c.pinned_dev + (size_t)slot[id] * pitch;
            if (upload[id]) memcpy(c.pinned + (size_t)slot[id] * pitch, blocks[id], (size_t)B);
        }
        // Completion by flags: every workgroup posts a flag once its stores are visible to the host, and the
        // host polls the flags instead of synchronizing the stream -- the runtime's completion round trip is
        // ~4 us of a ~14 us call (profiles/r02/small_call/small_call.cpp).  Only for launches whose
        // vector path covers every byte and that fit the flag page; anything else synchronizes as before.
        // the resident call worker, when enabled: one op of at most 16 inputs and 4 outputs, blocks of at
        // most 16 KiB in 4-byte lanes, tables already resident; anything else takes the launch path below
        if (ops.size() == 1 && B > 0 && (B % 4) == 0 && get_option(ECG_OPT_CALL_WORKER) > 0) {
            const LinearOp& op = ops[0];
            if (op.k_in() >= 1 && op.k_in() <= kWorkerMaxSrc && op.m_out() >= 1 && op.m_out() <= kWorkerMaxRows) {
                CallWorker& wk = g_worker[device_];
                std::unique_lock<std::mutex> lk(wk.mu, std::try_to_lock);
                if (lk.owns_lock()) {
                    int status = ECG_OK;
                    std::shared_ptr<ProgramSet> ps = program_set(&op, 1, &status, st);
                    if (!ps) return status;
                    if (ps->ready.load(std::memory_order_acquire) || hipEventQuery(ps->ready_ev) == hipSuccess) {
                        (void)ps->ensure_ready(st);  // marks the set ready (its upload has completed)
                        const int rc = wk.call(device_, *ps, op, dev.data(), B);
                        if (rc < 0) return rc;
                        if (rc == 0) {
                            for (int id = 0; id < nblocks; id++)
                                if (written[id]) memcpy(blocks[id], c.pinned + (size_t)slot[id] * pitch, (size_t)B);
                            return lease.done();
                        }
                    }
                }
            }
        }
        bool flagged = (B % 16) == 0 && flags_ready(c);
        for (const LinearOp& op : ops)
            flagged &= op.k_in() > 0 && op.k_in() <= kInlineSrc && op.m_out() <= kInlineDst;
        const unsigned seq = ++c.seq == 0 ? ++c.seq : c.seq;  // flags start at 0: never post 0
        int nflags = 0;
        for (const LinearOp& op : ops) {
            // >= workgroups x row tiles of either latency kernel (4 bytes per lane is the finer grid)
            const long long wg_max = ((B / 4 + kLatThreads - 1) / kLatThreads) * op.m_out();
            const bool f = flagged && nflags + wg_max <= kFlagSlots;
            flagged = f;
            int posted = 0;
            int rc = launch_one(op, dev.data(), B, st, /*host_tier=*/true, /*latency=*/true,
                                f ? c.flags_dev + nflags : nullptr, seq, &posted);
            if (rc != ECG_OK) {
                (void)hipStreamSynchronize(st);
                return rc;
            }
            nflags += posted;
        }
        if (flagged) {
            if (const int rc = wait_flags(c, nflags, seq, st); rc != ECG_OK) return rc;
        } else {
            ECG_HIP(hipStreamSynchronize(st));
        }
        for (int id = 0; id < nblocks; id++)
            if (written[id]) memcpy(blocks[id], c.pinned + (size_t)slot[id] * pitch, (size_t)B);
        return lease.done();
    }
    if (staged) {
        for (int id = 0; id < nblocks; id++)
            if (upload[id]) memcpy(c.pinned + (size_t)slot[id] * pitch, blocks[id], (size_t)B);
        if (n_up > 0) ECG_HIP(hipMemcpyAsync(c.scratch, c.pinned, pitch * n_up, hipMemcpyHostToDevice, st));
    }
    // large blocks: pageable copies, one per run of blocks that are contiguous both in host memory and in
    // the device scratch (the proxy's k slices of one value buffer, proxy.cpp:337-339, move as ONE copy:
    // a single large pageable copy runs at the pinned rate, per-block 1 MiB copies at half of it).
    // The caller's pages are deliberately NOT registered (hipHostRegister) for the call: the runtime
    // then treats every copy that touches those pages as pinned -- including other threads' copies of
    // neighbouring heap objects -- and unregistering under such a copy faulted the GPU
    // (tests/test_gpu_stress.py).
    if (!staged) {
        int id = 0;
        while (id < nblocks) {
            if (!upload[id]) {
                id++;
                continue;
            }
            int j = id + 1;
            while (j < nblocks && upload[j] && blocks[j] == blocks[j - 1] + B && dev[j] == dev[j - 1] + B) j++;
            ECG_HIP(hipMemcpyAsync(dev[id], blocks[id], (size_t)B * (j - id), hipMemcpyHostToDevice, st));
            id = j;
        }
    }
    for (const LinearOp& op : ops) {
        int rc = launch_one(op, dev.data(), B, st, /*host_tier=*/true);
        if (rc != ECG_OK) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
    }
    if (staged) {
        int lo = nslots, hi = -1;
        for (int id = 0; id < nblocks; id++)
            if (written[id]) {
                lo = std::min(lo, slot[id]);
                hi = std::max(hi, slot[id]);
            }
        if (hi >= lo) {
            ECG_HIP(hipMemcpyAsync(c.pinned + (size_t)lo * pitch, c.scratch + (size_t)lo * pitch,
                                   (size_t)(hi - lo) * pitch + (size_t)B, hipMemcpyDeviceToHost, st));
            ECG_HIP(hipStreamSynchronize(st));
            for (int id = 0; id < nblocks; id++)
                if (written[id]) memcpy(blocks[id], c.pinned + (size_t)slot[id] * pitch, (size_t)B);
        } else {
            ECG_HIP(hipStreamSynchronize(st));
        }
        return lease.done();
    }
    int id = 0;
    while (id < nblocks) {
        if (!written[id]) {
            id++;
            continue;
        }
        int j = id + 1;
        while (j < nblocks && written[j] && blocks[j] == blocks[j - 1] + B && dev[j] == dev[j - 1] + B) j++;
        ECG_HIP(hipMemcpyAsync(blocks[id], dev[id], (size_t)B * (j - id), hipMemcpyDeviceToHost, st));
        id = j;
    }
    ECG_HIP(hipStreamSynchronize(st));
    return lease.done();
}

}  // namespace ecg
