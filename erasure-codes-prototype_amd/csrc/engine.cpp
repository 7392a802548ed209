// GF(2^8) region engine, device tier: the engine of a device, the direct launch of one op, the pointer-table
// launches and the strided launch.  See engine.hpp; the program-table cache is in program_cache.cpp, the batch
// scope in batch_scope.cpp (its planning in batch_plan.cpp), the host tier in host_tier.cpp and host_pipeline.cpp.
#include "engine_internal.hpp"

namespace ecg {

namespace {

thread_local std::string t_last_error;

std::mutex g_engines_mu;
std::atomic<Engine*> g_engines[kMaxDevices] = {};

// One call's outputs lie apart from its inputs: none inside the span of its input blocks or the m blocks
// just past it (where an encode into [k+m][B] stripes or an in-place decode writes).  The pointer-table
// launch's grid-map hint (gf_kernels.hip outputs_in_stripe): speed only, never correctness.
static bool outputs_apart(const uint8_t* const* src, int k, const uint8_t* const* dst, int m, long long B) {
    uintptr_t lo = UINTPTR_MAX, hi = 0;
    for (int j = 0; j < k; j++) {
        lo = std::min(lo, (uintptr_t)src[j]);
        hi = std::max(hi, (uintptr_t)src[j] + (uintptr_t)B);
    }
    for (int q = 0; q < m; q++) {
        const uintptr_t d = (uintptr_t)dst[q];
        if (d + (uintptr_t)B > lo && d < hi + (uintptr_t)m * (uintptr_t)B) return false;
    }
    return true;
}

}  // namespace

const char* last_error_string() { return t_last_error.c_str(); }
void set_last_error(const std::string& s) { t_last_error = s; }

Engine::Engine(int device) : device_(device) {}

Engine& Engine::instance() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= kMaxDevices) dev = 0;
    if (Engine* e = g_engines[dev].load(std::memory_order_acquire)) return *e;  // every call: no lock
    std::lock_guard<std::mutex> lk(g_engines_mu);
    if (!g_engines[dev].load(std::memory_order_relaxed))
        g_engines[dev].store(new Engine(dev), std::memory_order_release);  // lives for the process
    return *g_engines[dev].load(std::memory_order_relaxed);
}

// One op over block pointers (device addresses), any k_in / m_out.  Ops that fit the kernel arguments
// carry their pointers inline; wider ones (k_in > 128 or m_out > 32) go through an uploaded pointer
// table (run_ptr_batch with one call), still asynchronous.
int Engine::launch_one(const LinearOp& op, uint8_t* const* blocks, long long B, hipStream_t st, bool host_tier,
                       bool latency, unsigned* flags, unsigned seq, int* n_flags) {
    if (n_flags) *n_flags = 0;
    if (op.m_out() == 0 || B == 0) return ECG_OK;
    if (op.k_in() == 0) {  // composed row of zeros: the library writes zero bytes
        for (int d : op.dst_ids) ECG_HIP(hipMemsetAsync(blocks[d], 0, (size_t)B, st));
        return ECG_OK;
    }
    if (op.k_in() > kInlineSrc || op.m_out() > kInlineDst) return run_ptr_batch(op, {blocks}, B, st);
    int status = ECG_OK;
    std::shared_ptr<ProgramSet> ps = program_set(&op, 1, &status, st);
    if (!ps) return status;
    if (const int rc = ps->ensure_ready(st); rc != ECG_OK) return rc;
    GfLaunch a = launch_args(*ps, B, 1);
    bool vec_ok = true;
    for (int d : op.dst_ids) vec_ok &= aligned16(blocks[d]);
    for (int s : op.src_ids) vec_ok &= aligned16(blocks[s]);
    for (int j = 0; j < op.k_in(); j++) a.isrc[j] = blocks[op.src_ids[j]];
    for (int p = 0; p < op.m_out(); p++) a.idst[p] = blocks[op.dst_ids[p]];
    a.done_flags = latency ? flags : nullptr;
    a.done_seq = seq;
    // A single small call fills a few dozen workgroups: its time is the latency chain, not bandwidth, so
    // small blocks take the latency kernel (every load in flight at once) on the device tier as well.
    const bool lat = latency || (B <= get_option(ECG_OPT_LAT_DWORD_BYTES) && op.k_in() <= kLatMaxSrc);
    ECG_HIP(launch_gf(a, lat ? GF_MODE_INLINE_LAT : GF_MODE_INLINE, vec_ok, st, n_flags));
    if (!host_tier) note_launch(*ps, st);
    return ECG_OK;
}

// here, beside its per-call readers (batch_flush_pending, run_device): see engine_internal.hpp
thread_local DeferScope t_defer;

bool batch_active() { return t_defer.active; }

int batch_flush_pending() {
    if (!t_defer.hq.empty()) return host_flush();  // at most one queue holds calls
    return t_defer.q.empty() ? ECG_OK : batch_flush();
}

namespace {

// Pointer tables for pointer-table launches: a per-device ring of pinned host + device slots shared by
// all threads (process lifetime, so no per-thread leak), each slot locked while it is filled and its
// launch enqueued, and reused only after that launch has completed (its event).
struct TableSlot {
    std::mutex mu;
    void* host = nullptr;
    void* dev = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    hipEvent_t up_ev = nullptr;  // the upload's completion, on the upload stream (upload_table)
    bool pending = false;
};
constexpr int kTableSlots = 16;
TableSlot g_tables[kMaxDevices][kTableSlots];
std::atomic<unsigned> g_table_next[kMaxDevices];

// Pointer tables go to the device ahead of the launch that reads them.  On the launch's own stream the copy
// waits for every earlier kernel there and the launch then waits for the copy: a DMA round trip between two
// kernels.  ECG_TABLE_UPLOAD=1 puts the copy on a per-device upload stream instead, so it runs while the launch
// stream's earlier kernels do, and the launch waits for it through an event (A/B switch, read once).  The slot's
// memory is rewritten only after its previous launch completed (TableSlot::ev), which waited for its upload.
bool table_upload_stream() {
    static const bool on = getenv("ECG_TABLE_UPLOAD") && atoi(getenv("ECG_TABLE_UPLOAD")) == 1;
    return on;
}
std::mutex g_upload_mu;
hipStream_t g_upload_stream[kMaxDevices];

hipError_t upload_table(int dev, TableSlot& t, size_t bytes, hipStream_t st) {
    if (!table_upload_stream()) return hipMemcpyAsync(t.dev, t.host, bytes, hipMemcpyHostToDevice, st);
    hipStream_t u;
    {
        std::lock_guard<std::mutex> lk(g_upload_mu);
        if (!g_upload_stream[dev]) {
            const hipError_t e = hipStreamCreateWithFlags(&g_upload_stream[dev], hipStreamNonBlocking);
            if (e != hipSuccess) return e;
        }
        u = g_upload_stream[dev];
    }
    hipError_t e;
    if (!t.up_ev && (e = hipEventCreateWithFlags(&t.up_ev, hipEventDisableTiming)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(t.dev, t.host, bytes, hipMemcpyHostToDevice, u)) != hipSuccess) return e;
    if ((e = hipEventRecord(t.up_ev, u)) != hipSuccess) {
        (void)hipStreamSynchronize(u);
        return e;
    }
    return hipStreamWaitEvent(st, t.up_ev, 0);
}

// The pointer-table launch itself: S calls over ps's programs, call s running program d_prog[s] (null: the
// set's one program), its k source pointers at d_src + s * k and its m destination pointers at d_dst + s * m.
int launch_ptrs(Engine& eng, ProgramSet& ps, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* d_prog,
                int S, long long B, bool aligned, hipStream_t st, bool apart) {
    GfLaunch a = launch_args(ps, B, S);
    a.src_ptrs = d_src;
    a.dst_ptrs = d_dst;
    a.prog_of_stripe = d_prog;
    a.grid_map = apart ? 2 : 0;  // the auto map's layout hint (gf_kernels.hip outputs_in_stripe)
    const hipError_t e = launch_gf(a, GF_MODE_PTRS, aligned, st);
    if (e != hipSuccess) {
        const char* what = d_prog ? "launch_gf(pointer table, multi): " : "launch_gf(a, GF_MODE_PTRS, aligned, st): ";
        set_last_error(std::string(what) + hipGetErrorString(e));
        return ECG_EHIP;
    }
    eng.note_launch(ps, st);
    return ECG_OK;
}

// One pointer-table launch over S calls of one op shape (k sources, m destinations), the same for one plan and
// for mixed plans: takes the next slot of the device's ring and waits for the launch that last used it, fills
// it -- every call's k source pointers, then every call's m destination pointers (call c's ids are
// op_of(c)'s), then the calls' program ids `pid` if there are any --, uploads it, runs
// launch(d_src, d_dst, d_pid, aligned, apart) on the table's device view and records the slot's event behind
// it, whatever the launch returned (the upload may still be reading the slot).
template <class OpOf, class Launch>
int ptr_table_launch(int dev, const std::vector<const uint8_t* const*>& calls, int k, int m, long long B,
                     hipStream_t st, OpOf op_of, const int* pid, Launch launch) {
    const int S = (int)calls.size();
    const size_t ptr_bytes = (size_t)S * (k + m) * sizeof(void*);
    const size_t bytes = ptr_bytes + (pid ? (size_t)S * sizeof(int) : 0);
    TableSlot& t = g_tables[dev][g_table_next[dev].fetch_add(1, std::memory_order_relaxed) % kTableSlots];
    std::lock_guard<std::mutex> lk(t.mu);
    if (t.pending) {
        ECG_HIP(hipEventSynchronize(t.ev));
        t.pending = false;
    }
    if (!t.ev) ECG_HIP(hipEventCreateWithFlags(&t.ev, hipEventDisableTiming));
    if (t.cap < bytes) {
        if (t.host) (void)hipHostFree(t.host);
        if (t.dev) (void)hipFree(t.dev);
        t.host = t.dev = nullptr;
        t.cap = 0;
        const size_t cap = std::max(bytes, (size_t)64 << 10);
        ECG_HIP(hipHostMalloc(&t.host, cap, hipHostMallocDefault));
        ECG_HIP(hipMalloc(&t.dev, cap));
        t.cap = cap;
    }
    const uint8_t** h = (const uint8_t**)t.host;
    bool aligned = true, apart = true;
    for (int c = 0; c < S; c++) {
        const LinearOp& op = op_of(c);
        for (int j = 0; j < k; j++) {
            const uint8_t* p = calls[c][op.src_ids[j]];
            aligned &= aligned16(p);
            h[(size_t)c * k + j] = p;
        }
        for (int q = 0; q < m; q++) {
            const uint8_t* p = calls[c][op.dst_ids[q]];
            aligned &= aligned16(p);
            h[(size_t)S * k + (size_t)c * m + q] = p;
        }
        if (apart) apart = outputs_apart(h + (size_t)c * k, k, h + (size_t)S * k + (size_t)c * m, m, B);
    }
    if (pid) memcpy((uint8_t*)t.host + ptr_bytes, pid, (size_t)S * sizeof(int));
    ECG_HIP(upload_table(dev, t, bytes, st));
    const int rc = launch((const uint8_t* const*)t.dev, (uint8_t* const*)((const uint8_t**)t.dev + (size_t)S * k),
                          pid ? (const int*)((uint8_t*)t.dev + ptr_bytes) : nullptr, aligned, apart);
    ECG_HIP(hipEventRecord(t.ev, st));
    t.pending = true;
    return rc;
}

}  // namespace

// A run of recorded calls whose blocks form one strided batch goes out as a strided launch (the
// batched tier's kernel: no pointer table, 10-15 % less kernel time on the config-2 batch); any other
// run keeps the pointer-table launch.  *done = false: not strided, nothing launched.
int Engine::run_calls_strided(const LinearOp& op, const std::vector<const uint8_t* const*>& calls, long long B,
                              hipStream_t st, bool* done) {
    *done = false;
    const uint8_t *ib = nullptr, *ob = nullptr;
    long long iss = 0, ibs = 0, oss = 0, obs = 0;
    std::vector<int> vi, vo;
    if (!strided_side(calls, op.src_ids, ib, iss, ibs, vi) || !strided_side(calls, op.dst_ids, ob, oss, obs, vo))
        return ECG_OK;
    if ((((uintptr_t)ib | (uintptr_t)ob) & 15) || ((iss | ibs | oss | obs) & 15)) return ECG_OK;
    LinearOp s2 = op;
    s2.src_ids = vi;
    s2.dst_ids = vo;
    *done = true;
    return run_strided({s2}, nullptr, (int)calls.size(), ib, iss, ibs, (void*)ob, oss, obs, B, st);
}

int Engine::run_ptr_batch(const LinearOp& op, const std::vector<const uint8_t* const*>& calls, long long B,
                          hipStream_t st) {
    return ptr_table_launch(
        device_, calls, op.k_in(), op.m_out(), B, st, [&](int) -> const LinearOp& { return op; }, nullptr,
        [&](const uint8_t* const* d_src, uint8_t* const* d_dst, const int*, bool aligned, bool apart) {
            return run_ptrs(op, d_src, d_dst, (int)calls.size(), B, aligned, st, apart);
        });
}

// S calls of one op shape (k_in, m_out), call s running *ops[s] over its blocks calls[s]: ONE pointer-table
// launch with one program per distinct coefficient matrix (prog_of_stripe), instead of one launch per
// plan.  Programs are kept with canonical ids (the pointer table carries each call's own blocks), so calls
// that differ only in which blocks they name share a program.
int Engine::run_ptr_batch_multi(const std::vector<const LinearOp*>& ops, const std::vector<const uint8_t* const*>& calls,
                                long long B, hipStream_t st) {
    const int S = (int)calls.size();
    if (S == 0 || B == 0) return ECG_OK;
    if (ops.size() != calls.size()) return ECG_EINVAL;
    const int k = ops[0]->k_in(), m = ops[0]->m_out();
    if (k < 1 || m < 1) return ECG_EINVAL;
    thread_local std::vector<LinearOp> progs;
    thread_local std::vector<int> pid;
    progs.clear();
    pid.assign((size_t)S, 0);
    const LinearOp* last = nullptr;
    int last_id = -1;
    for (int c = 0; c < S; c++) {
        const LinearOp& op = *ops[c];
        if (op.k_in() != k || op.m_out() != m) return ECG_EINVAL;
        if (&op == last) {
            pid[c] = last_id;
            continue;
        }
        int id = -1;
        for (size_t p = 0; p < progs.size() && id < 0; p++)
            if (progs[p].coef == op.coef) id = (int)p;
        if (id < 0) {
            LinearOp canon;
            canon.coef = op.coef;
            for (int j = 0; j < k; j++) canon.src_ids.push_back(j);
            for (int q = 0; q < m; q++) canon.dst_ids.push_back(k + q);
            progs.push_back(std::move(canon));
            id = (int)progs.size() - 1;
        }
        pid[c] = last_id = id;
        last = &op;
    }
    auto op_of = [&](int c) -> const LinearOp& { return *ops[c]; };
    if (progs.size() == 1)  // one matrix: the plain pointer-table launch (the table holds each call's own blocks)
        return ptr_table_launch(
            device_, calls, k, m, B, st, op_of, nullptr,
            [&](const uint8_t* const* d_src, uint8_t* const* d_dst, const int*, bool aligned, bool apart) {
                return run_ptrs(progs[0], d_src, d_dst, S, B, aligned, st, apart);
            });
    // One set of matrices is one cache entry, whatever order the calls met them in (per-stripe
    // decodes of one batch in another order would otherwise build, and retire, a new program set each time).
    {
        thread_local std::vector<int> order, rank;
        order.resize(progs.size());
        for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
        std::sort(order.begin(), order.end(), [](int a, int b) { return progs[a].coef < progs[b].coef; });
        rank.resize(progs.size());
        bool moved = false;
        for (size_t r = 0; r < order.size(); r++) {
            rank[order[r]] = (int)r;
            moved |= order[r] != (int)r;
        }
        if (moved) {
            thread_local std::vector<LinearOp> sorted;
            sorted.clear();
            for (int i : order) sorted.push_back(std::move(progs[i]));
            progs.swap(sorted);
            for (int& x : pid) x = rank[x];
        }
    }
    int status = ECG_OK;
    std::shared_ptr<ProgramSet> ps = program_set(progs, &status, st);
    if (!ps) return status;
    if (const int rc = ps->ensure_ready(st); rc != ECG_OK) return rc;
    return ptr_table_launch(
        device_, calls, k, m, B, st, op_of, pid.data(),
        [&](const uint8_t* const* d_src, uint8_t* const* d_dst, const int* d_pid, bool aligned, bool apart) {
            return launch_ptrs(*this, *ps, d_src, d_dst, d_pid, S, B, aligned, st, apart);
        });
}

int Engine::launch_direct(const std::vector<LinearOp>& ops, uint8_t* const* blocks, long long B, hipStream_t st) {
    for (const LinearOp& op : ops) {
        int rc = launch_one(op, blocks, B, st, /*host_tier=*/false);
        if (rc != ECG_OK) return rc;
    }
    return ECG_OK;
}

static int check_ids(const std::vector<LinearOp>& ops, uint8_t* const* blocks, int nblocks) {
    return walk_block_ids(ops, blocks, nblocks, [](int) {}, [](int) {});
}

int Engine::run_device(const std::vector<LinearOp>& ops, uint8_t* const* blocks, int nblocks, long long B,
                       hipStream_t st) {
    if (B < 0) return ECG_EINVAL;
    if (const int rc = check_ids(ops, blocks, nblocks); rc != ECG_OK) return rc;
    if (t_defer.active) {
        if (ops.empty() || B == 0) return ECG_OK;
        if (!t_defer.hq.empty())
            if (const int rc = host_flush(); rc != ECG_OK) return rc;
        std::shared_ptr<const std::vector<LinearOp>> shared;
        if (!t_defer.q.empty() && same_ops(*t_defer.q.back().ops, ops)) shared = t_defer.q.back().ops;
        else shared = std::make_shared<const std::vector<LinearOp>>(ops);
        t_defer.q.push_back(DeferredCall{this, st, B, std::move(shared), std::vector<uint8_t*>(blocks, blocks + nblocks)});
        return t_defer.q.size() >= flush_at(t_defer) ? batch_flush() : ECG_OK;
    }
    return launch_direct(ops, blocks, B, st);
}

int Engine::run_device(const std::shared_ptr<const std::vector<LinearOp>>& ops, uint8_t* const* blocks, int nblocks,
                       long long B, hipStream_t st) {
    if (B < 0 || !ops) return ECG_EINVAL;
    if (const int rc = check_ids(*ops, blocks, nblocks); rc != ECG_OK) return rc;
    if (t_defer.active) {  // recorded with the caller's (interned) plan: no copy
        if (ops->empty() || B == 0) return ECG_OK;
        if (!t_defer.hq.empty())
            if (const int rc = host_flush(); rc != ECG_OK) return rc;
        t_defer.q.push_back(DeferredCall{this, st, B, ops, std::vector<uint8_t*>(blocks, blocks + nblocks)});
        return t_defer.q.size() >= flush_at(t_defer) ? batch_flush() : ECG_OK;
    }
    return launch_direct(*ops, blocks, B, st);
}

// Row split of a batched launch (ECG_OPT_ROW_SPLIT, include/ecg.h): when every program's output rows read
// disjoint input sets of one size, each (stripe, row) runs as its own launch stripe over that row's inputs
// only.  A PC merge's 40 -> 5 XOR then streams 8 blocks per workgroup instead of 40 (the fused form ran
// at 0.72 of HBM peak against 0.76 for rows, profiles/r03/final/workloads/bench_pc-merge.log).  Rows
// then run in different workgroups, so no output block may be an input block of the same stripe: the
// split is taken only when the outputs provably overlap no input (disjoint spans, or, for equal stripe
// strides, no output within B bytes of an input of its stripe).  Returns R = rows per program (0 = no
// split) and the split programs, program p * R + r = row r of program p.
static int row_split(const std::vector<LinearOp>& progs, int S, const void* in_base, long long iss, long long ibs,
                     const void* out_base, long long oss, long long obs, long long B, bool has_stripe_of,
                     std::vector<LinearOp>& rows) {
    const long long min_k = get_option(ECG_OPT_ROW_SPLIT);
    const int k = progs[0].k_in(), m = progs[0].m_out();
    if (min_k <= 0 || k < min_k || m < 2 || k % m || (long long)S * m > 0x7fffffffLL) return 0;
    // the disjointness tests below bound spans by their last block, which needs non-negative strides
    if (iss < 0 || ibs < 0 || oss < 0 || obs < 0) return 0;
    const int kr = k / m;
    int max_src = 0, max_dst = 0;
    for (const LinearOp& op : progs) {
        if (op.k_in() != k || op.m_out() != m || op.coef.size() != (size_t)k * m) return 0;
        for (int j = 0; j < k; j++) {
            int users = 0;
            for (int r = 0; r < m; r++) users += op.coef[(size_t)r * k + j] != 0;
            if (users != 1) return 0;
        }
        for (int r = 0; r < m; r++) {
            int n = 0;
            for (int j = 0; j < k; j++) n += op.coef[(size_t)r * k + j] != 0;
            if (n != kr) return 0;
        }
        for (int id : op.src_ids) max_src = std::max(max_src, id);
        for (int id : op.dst_ids) max_dst = std::max(max_dst, id);
    }
    const uintptr_t ib = (uintptr_t)in_base, ob = (uintptr_t)out_base;
    bool safe = false;
    if (!has_stripe_of) {
        const uintptr_t i1 = ib + (uintptr_t)((S - 1) * iss + max_src * ibs + B);
        const uintptr_t o1 = ob + (uintptr_t)((S - 1) * oss + max_dst * obs + B);
        safe = i1 <= ob || o1 <= ib;
    }
    if (!safe && iss == oss) {
        safe = true;
        for (const LinearOp& op : progs)
            for (int d : op.dst_ids)
                for (int j : op.src_ids) {
                    const long long delta = (long long)(ob + (uintptr_t)(d * obs)) - (long long)(ib + (uintptr_t)(j * ibs));
                    if (delta > -B && delta < B) safe = false;
                }
    }
    if (!safe) return 0;
    rows.clear();
    for (const LinearOp& op : progs)
        for (int r = 0; r < m; r++) {
            LinearOp one;
            one.dst_ids.push_back(op.dst_ids[r]);
            for (int j = 0; j < k; j++)
                if (const uint8_t c = op.coef[(size_t)r * k + j]) {
                    one.src_ids.push_back(op.src_ids[j]);
                    one.coef.push_back(c);
                }
            rows.push_back(std::move(one));
        }
    return m;
}

int Engine::run_strided(const std::vector<LinearOp>& progs, const int* d_prog_of_stripe, int S,
                        const void* in_base, long long in_sstride, long long in_bstride, void* out_base,
                        long long out_sstride, long long out_bstride, long long B, hipStream_t st,
                        const int* d_stripe_of) {
    if (S < 0 || B < 0) return ECG_EINVAL;
    if (S == 0 || B == 0) return ECG_OK;  // empty batch: nothing to read or write
    if (!in_base || !out_base) return ECG_EINVAL;
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;
    if (progs.size() > 1 && !d_prog_of_stripe) return ECG_EINVAL;
    thread_local std::vector<LinearOp> rows;
    const int R = row_split(progs, S, in_base, in_sstride, in_bstride, out_base, out_sstride, out_bstride, B,
                            d_stripe_of != nullptr, rows);
    int status = ECG_OK;
    std::shared_ptr<ProgramSet> ps = R ? program_set(rows, &status, st) : program_set(progs, &status, st);
    if (!ps) return status;
    if (const int rc = ps->ensure_ready(st); rc != ECG_OK) return rc;
    GfLaunch a = launch_args(*ps, B, R ? S * R : S);
    a.prog_of_stripe = progs.size() > 1 ? d_prog_of_stripe : nullptr;
    a.stripe_of = d_stripe_of;
    a.in_base = (const uint8_t*)in_base;
    a.out_base = (uint8_t*)out_base;
    a.in_sstride = in_sstride;
    a.in_bstride = in_bstride;
    a.out_sstride = out_sstride;
    a.out_bstride = out_bstride;
    a.row_split = R;
    const bool vec_ok = aligned16(in_base) && aligned16(out_base) && (in_sstride % 16 == 0) &&
                        (in_bstride % 16 == 0) && (out_sstride % 16 == 0) && (out_bstride % 16 == 0);
    ECG_HIP(launch_gf(a, GF_MODE_STRIDED, vec_ok, st));
    note_launch(*ps, st);
    return ECG_OK;
}

int Engine::run_ptrs(const LinearOp& prog, const uint8_t* const* d_src, uint8_t* const* d_dst, int S, long long B,
                     bool aligned, hipStream_t st, bool apart) {
    if (S < 0 || B < 0) return ECG_EINVAL;
    if (S == 0 || B == 0) return ECG_OK;
    if (!d_src || !d_dst) return ECG_EINVAL;
    int status = ECG_OK;
    std::shared_ptr<ProgramSet> ps = program_set(&prog, 1, &status, st);
    if (!ps) return status;
    if (const int rc = ps->ensure_ready(st); rc != ECG_OK) return rc;
    return launch_ptrs(*this, *ps, d_src, d_dst, nullptr, S, B, aligned, st, apart);
}

}  // namespace ecg
