// Deferred-batch scope (engine.hpp): opening and closing it, declaring scratch, and the flush that turns the
// recorded device-tier calls into grouped launches.  The planning it relies on is in batch_plan.hpp.
#include <numeric>

#include "engine_internal.hpp"

namespace ecg {

// One side (the inputs or the outputs of `ids`) of a run of recorded calls in the strided form
// base + call * sstride + v[j] * bstride.  True only if EVERY pointer of every call is exactly that, so
// a strided launch touches exactly the bytes the pointer-table launch would.  A per-stripe loop over
// one [S][n][B] batch in HBM (the reference's proxy loop on device buffers) has this form.
bool strided_side(const std::vector<const uint8_t* const*>& calls, const std::vector<int>& ids,
                  const uint8_t*& base, long long& sstride, long long& bstride, std::vector<int>& v) {
    const size_t R = calls.size(), n = ids.size();
    if (R < 2 || n == 0) return false;
    uintptr_t lo = UINTPTR_MAX;
    for (int id : ids) lo = std::min(lo, (uintptr_t)calls[0][id]);
    unsigned long long g = 0;
    for (int id : ids) g = std::gcd(g, (unsigned long long)((uintptr_t)calls[0][id] - lo));
    v.resize(n);
    for (size_t j = 0; j < n; j++) {
        const unsigned long long q = g ? ((uintptr_t)calls[0][ids[j]] - lo) / g : 0;
        if (q > 0x7fffffffULL) return false;
        v[j] = (int)q;
    }
    const uintptr_t p00 = (uintptr_t)calls[0][ids[0]], p10 = (uintptr_t)calls[1][ids[0]];
    if (p10 <= p00 || p10 - p00 > (uintptr_t)(1ULL << 40)) return false;
    const uintptr_t st = p10 - p00;
    for (size_t c = 0; c < R; c++)
        for (size_t j = 0; j < n; j++)
            if ((uintptr_t)calls[c][ids[j]] != (uintptr_t)calls[0][ids[j]] + c * st) return false;
    base = (const uint8_t*)lo;
    sstride = (long long)st;
    bstride = (long long)g;
    return true;
}

// Fast path of a flush: every recorded call has the same plan (one interned object), stream, engine and
// block size, and the blocks of all calls form one strided batch in which no two (call, block) pairs
// overlap -- a per-stripe loop over one [S][n][B] batch, or over a block-major [n][S][B] one.  Then no call
// reads or writes a block another call touches, so they form ONE group: what schedule_groups would
// return, without hashing every block address.  Overlap-free when either
//   (a) blocks of a call are >= B apart and whole stripes are apart: ss >= (vmax - vmin) * bs + B, or
//   (b) calls are >= B apart and whole block rows are apart: bs >= (R - 1) * ss + B.
static bool one_disjoint_strided_group(const std::vector<DeferredCall>& q) {
    const size_t R = q.size();
    if (R < 2) return false;
    const DeferredCall& a = q[0];
    for (const DeferredCall& c : q)
        if (c.ops.get() != a.ops.get() || c.st != a.st || c.B != a.B || c.eng != a.eng) return false;
    thread_local std::vector<int> ids, v;
    thread_local std::vector<const uint8_t* const*> calls;
    ids.clear();
    for (const LinearOp& op : *a.ops) {
        ids.insert(ids.end(), op.src_ids.begin(), op.src_ids.end());
        ids.insert(ids.end(), op.dst_ids.begin(), op.dst_ids.end());
    }
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    calls.resize(R);
    for (size_t c = 0; c < R; c++) calls[c] = q[c].blocks.data();
    const uint8_t* base = nullptr;
    long long ss = 0, bs = 0;
    if (!strided_side(calls, ids, base, ss, bs, v)) return false;
    const long long B = a.B;
    const int vmin = *std::min_element(v.begin(), v.end()), vmax = *std::max_element(v.begin(), v.end());
    if (vmax == vmin) return ss >= B;  // one block per call (or every id the same block)
    if (bs < B) return false;
    return ss >= (long long)(vmax - vmin) * bs + B || (ss >= B && bs >= (long long)(R - 1) * ss + B);
}

int batch_begin() {
    DeferScope& d = t_defer;
    if (d.active) return ECG_EINVAL;  // scopes do not nest
    d.active = true;
    d.q.clear();
    d.scratch.clear();
    d.last_st = nullptr;
    d.last_dev = -1;
    d.last_recorded = false;
    d.host_defer = false;
    return ECG_OK;
}

int batch_defer_host(int on) {
    if (!t_defer.active) return ECG_EINVAL;
    if (!on && !t_defer.hq.empty()) {
        const int rc = host_flush();
        if (rc != ECG_OK) return rc;
    }
    t_defer.host_defer = on != 0;
    return ECG_OK;
}

int batch_scratch(const void* p, size_t bytes) {
    if (!t_defer.active || !p) return ECG_EINVAL;
    if (bytes == 0) return ECG_OK;
    if ((uintptr_t)p + bytes < (uintptr_t)p) return ECG_EINVAL;
    t_defer.scratch.add((uintptr_t)p, (uintptr_t)p + bytes);
    return ECG_OK;
}

FlushStats last_flush_stats() { return t_defer.stats; }

// Record the scope's ordering event of device `dev` (the current device) behind the work enqueued on `st` so
// far; `st` is a stream of the flush in progress, alive for the duration of the call.
int order_after(hipStream_t st, int dev) {
    if (dev < 0 || dev >= kMaxDevices) return ECG_EINVAL;
    DeferScope& d = t_defer;
    hipEvent_t ev = d.order_ev(dev);
    if (!ev) {
        Engine& eng = Engine::instance();  // the engine of the current device, dev
        if (!(ev = eng.acquire_event())) {
            set_last_error("batch flush: hipEventCreate failed");
            return ECG_EHIP;
        }
        d.order_evs.emplace_back(&eng, ev);
    }
    if (hipEventRecord(ev, st) != hipSuccess) {
        set_last_error("batch flush: hipEventRecord failed");
        return ECG_EHIP;
    }
    return ECG_OK;
}

int batch_flush() {
    DeferScope& d = t_defer;
    if (d.q.empty()) return ECG_OK;
    std::vector<DeferredCall> q;
    q.swap(d.q);
    FlushStats st;
    st.recorded = (long long)q.size();
    if (!d.scratch.empty()) q = compose_scratch(std::move(q), d.scratch, /*scope_end=*/!d.active, &st.materialised);
    st.composed = (long long)q.size();
    std::vector<std::vector<size_t>> groups;
    std::vector<int> plan_id;  // per call: its plan (by content); empty on the fast path (one plan)
    if (d.scratch.empty() && one_disjoint_strided_group(q)) {  // the per-stripe loop over one batch
        groups.emplace_back(q.size());
        std::iota(groups[0].begin(), groups[0].end(), (size_t)0);
    } else {
        PlanClasses classes;
        std::vector<int> cls(q.size());
        plan_id.resize(q.size());
        for (size_t c = 0; c < q.size(); c++) {
            cls[c] = classes.of(q[c]);
            plan_id[c] = classes.plan_of_last();
        }
        auto reads = [&](size_t c, auto&& f) {
            for (const LinearOp& op : *q[c].ops)
                for (int id : op.src_ids) f(q[c].blocks[id]);
        };
        auto writes = [&](size_t c, auto&& f) {
            for (const LinearOp& op : *q[c].ops)
                for (int id : op.dst_ids) f(q[c].blocks[id]);
        };
        groups = schedule_groups(q.size(), [&](size_t c) { return cls[c]; }, reads, writes);
    }
    st.groups = (long long)groups.size();
    int caller_dev = -1, cur_dev = -1;
    (void)hipGetDevice(&caller_dev);
    cur_dev = caller_dev;
    int rc = ECG_OK;
    // the previous group: the last one of the scope's previous flush, if any (its ordering event is then
    // already recorded: that flush's stream is not named again)
    hipStream_t prev_st = d.last_st;
    int prev_dev = d.last_dev;
    bool prev_recorded = d.last_recorded;
    auto set_dev = [&](int dev) {
        if (dev == cur_dev) return ECG_OK;
        if (hipSetDevice(dev) != hipSuccess) {
            set_last_error("batch flush: hipSetDevice failed");
            return ECG_EHIP;
        }
        cur_dev = dev;
        return ECG_OK;
    };
    for (size_t g = 0; g < groups.size() && rc == ECG_OK; g++) {
        const std::vector<size_t>& G = groups[g];
        const DeferredCall& c0 = q[G[0]];
        Engine* eng = c0.eng;
        // Groups run in program order across streams and devices: where the stream changes from one group
        // to the next, the new stream waits for an event recorded behind the previous group (so a chain
        // A, B, A orders every group after all earlier ones).  The calls were recorded in one order; a group
        // on stream B may read blocks an earlier group on A writes, or a scratch combination recorded on A
        // (compose_scratch joins those to the op that forces them).  The chain runs across the scope's
        // flushes too: the first group of a flush follows the last group of the previous one
        // (test_batch_scope_orders_streams_across_eager_flushes).  One stream: no event at all.
        // (prev_dev, not prev_st, says whether there was a previous group: the null stream -- torch's default
        // stream -- is a stream like any other here)
        const bool switch_st = prev_dev >= 0 && (c0.st != prev_st || eng->device() != prev_dev);
        if (switch_st && !prev_recorded) {  // the event is recorded behind the previous group, on its device
            if ((rc = set_dev(prev_dev)) != ECG_OK || (rc = order_after(prev_st, prev_dev)) != ECG_OK) break;
        }
        if ((rc = set_dev(eng->device())) != ECG_OK) break;  // a group launches on its calls' device
        if (switch_st && hipStreamWaitEvent(c0.st, d.order_ev(prev_dev), 0) != hipSuccess) {
            set_last_error("batch flush: hipStreamWaitEvent failed");
            rc = ECG_EHIP;
            break;
        }
        prev_st = c0.st;
        prev_dev = eng->device();
        prev_recorded = false;
        if (G.size() == 1) {
            rc = eng->launch_direct(*c0.ops, c0.blocks.data(), c0.B, c0.st);
            st.launches += (long long)c0.ops->size();
            continue;
        }
        std::vector<const uint8_t* const*> calls;
        calls.reserve(G.size());
        for (size_t c : G) calls.push_back(q[c].blocks.data());
        bool mixed = false;  // single-op plans of one shape, several matrices (PlanClasses)
        if (!plan_id.empty())
            for (size_t c : G) mixed |= plan_id[c] != plan_id[G[0]];
        if (mixed) {
            std::vector<const LinearOp*> per_call;
            per_call.reserve(G.size());
            for (size_t c : G) per_call.push_back(&(*q[c].ops)[0]);
            rc = eng->run_ptr_batch_multi(per_call, calls, c0.B, c0.st);
            st.launches++;
            continue;
        }
        for (const LinearOp& op : *c0.ops) {
            if (op.k_in() == 0) {  // composed row of zeros: the library writes zero bytes
                for (size_t c : G) {
                    rc = eng->launch_direct({op}, q[c].blocks.data(), q[c].B, q[c].st);
                    st.launches++;
                    if (rc != ECG_OK) break;
                }
            } else {
                bool done = false;
                rc = eng->run_calls_strided(op, calls, c0.B, c0.st, &done);
                if (rc == ECG_OK && !done) rc = eng->run_ptr_batch(op, calls, c0.B, c0.st);
                st.launches++;
            }
            if (rc != ECG_OK) break;
        }
    }
    // the scope stays open: the next flush may start on another stream, so the last group's ordering event
    // is recorded now, while its stream is certainly alive (one event record per flush)
    if (rc == ECG_OK && d.active && prev_dev >= 0 && !prev_recorded) {
        if ((rc = set_dev(prev_dev)) == ECG_OK) rc = order_after(prev_st, prev_dev);
        prev_recorded = rc == ECG_OK;
    }
    if (cur_dev != caller_dev && caller_dev >= 0) (void)hipSetDevice(caller_dev);
    d.last_st = prev_st;
    d.last_dev = prev_dev;
    d.last_recorded = prev_recorded;
    d.stats = st;
    // the next recording reuses this queue's capacity (a scope of thousands of calls regrew it every flush)
    q.clear();
    if (d.q.empty() && d.q.capacity() < q.capacity()) d.q.swap(q);
    return rc;
}

int batch_flush_all() {
    const int rh = t_defer.hq.empty() ? ECG_OK : host_flush();
    const int rd = batch_flush();
    return rh != ECG_OK ? rh : rd;
}

int batch_end() {
    DeferScope& d = t_defer;
    if (!d.active) return ECG_EINVAL;
    d.active = false;  // the flush below is the scope's end: unconsumed scratch is not written
    const int rc = batch_flush_all();
    d.host_defer = false;
    d.q.clear();
    d.scratch.clear();
    d.release_order_evs();  // a later wait on one refers to its record at the time of the wait
    return rc;
}

}  // namespace ecg
