// Program-table cache of the region engine: building and uploading a program set, the pools its memory and
// events come from, and the retirement of evicted sets.  See engine.hpp (ProgramSet, Engine).
#include "engine_internal.hpp"
#include "gf256.hpp"

namespace ecg {

// Freed without waiting: a set that was ever launched is destroyed only by sweep_retired(), after its
// launches completed; any other (a lost insertion race, a failed build) was never launched.
ProgramSet::~ProgramSet() {
    if (ready_ev) {
        // a set dropped before its upload was seen complete (a lost insertion race): the copy must land
        // before the memory is reused
        if (!ready.load(std::memory_order_acquire)) (void)hipEventSynchronize(ready_ev);
        (void)hipEventDestroy(ready_ev);
    }
    if (pinned) owner->release_pinned(pinned, pinned_class);
    if (mem) owner->release_tables(mem, mem_class);
}

// A retirement cover: an event recorded on one stream after the set was retired; back to the pool when the
// last set it covers is freed (it has fired by then, or the device was synchronized).
struct ProgramSet::CoverEvent {
    Engine* eng;
    hipEvent_t ev;
    ~CoverEvent() { eng->release_event(ev); }
};

// A cover recorded on st now (null: no event to be had, or the record failed).
static std::shared_ptr<ProgramSet::CoverEvent> record_cover(Engine* eng, hipStream_t st) {
    hipEvent_t ev = eng->acquire_event();
    if (ev && hipEventRecord(ev, st) == hipSuccess)
        return std::make_shared<ProgramSet::CoverEvent>(ProgramSet::CoverEvent{eng, ev});
    if (ev) eng->release_event(ev);
    return nullptr;
}

hipEvent_t Engine::acquire_event() {
    {
        std::lock_guard<std::mutex> lk(pmu_);
        if (!event_pool_.empty()) {
            hipEvent_t ev = event_pool_.back();
            event_pool_.pop_back();
            return ev;
        }
    }
    hipEvent_t ev = nullptr;
    return hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess ? ev : nullptr;
}

void Engine::release_event(hipEvent_t ev) {
    std::lock_guard<std::mutex> lk(pmu_);
    event_pool_.push_back(ev);
}

// Before a launch on `st` reads the set's tables: once the upload event has fired the set is ready for
// every stream; until then a launch on another stream than the uploading one waits for the event.
int ProgramSet::ensure_ready(hipStream_t st) {
    if (ready.load(std::memory_order_acquire)) return ECG_OK;
    const hipError_t q = hipEventQuery(ready_ev);
    if (q == hipSuccess) {
        std::lock_guard<std::mutex> lk(smu);  // one thread hands the pinned source back
        if (!ready.load(std::memory_order_relaxed)) {
            if (pinned) owner->release_pinned(pinned, pinned_class);
            pinned = nullptr;
            ready.store(true, std::memory_order_release);
        }
        return ECG_OK;
    }
    if (q != hipErrorNotReady) return ECG_EHIP;
    if (stream_key(st) != first_stream && hipStreamWaitEvent(st, ready_ev, 0) != hipSuccess) return ECG_EHIP;
    return ECG_OK;
}

namespace {

using BlockPool = std::unordered_map<size_t, std::vector<void*>>;  // power-of-two class -> free blocks

// The class that holds `bytes`, and a pooled block of it if there is one (the caller allocates otherwise).
void* pool_take(std::mutex& mu, BlockPool& pool, size_t& pooled, size_t bytes, size_t* cls) {
    size_t c = 256;
    while (c < bytes) c <<= 1;
    *cls = c;
    std::lock_guard<std::mutex> lk(mu);
    auto it = pool.find(c);
    if (it == pool.end() || it->second.empty()) return nullptr;
    void* p = it->second.back();
    it->second.pop_back();
    pooled -= c;
    return p;
}

// Back into the pool while it holds at most `cap` bytes; false: the caller frees the block.
bool pool_give(std::mutex& mu, BlockPool& pool, size_t& pooled, size_t cap, void* p, size_t cls) {
    std::lock_guard<std::mutex> lk(mu);
    if (pooled + cls > cap) return false;
    pool[cls].push_back(p);
    pooled += cls;
    return true;
}

}  // namespace

void* Engine::acquire_tables(size_t bytes, size_t* cls, hipError_t* err) {
    *err = hipSuccess;
    void* p = pool_take(pmu_, pool_, pooled_bytes_, bytes, cls);
    if (!p) *err = hipMalloc(&p, *cls);
    return *err == hipSuccess ? p : nullptr;
}

void* Engine::acquire_pinned(size_t bytes, size_t* cls, hipError_t* err) {
    *err = hipSuccess;
    void* p = pool_take(pmu_, pinned_pool_, pinned_pooled_bytes_, bytes, cls);
    if (!p) *err = hipHostMalloc(&p, *cls, hipHostMallocDefault);
    return *err == hipSuccess ? p : nullptr;
}

void Engine::release_pinned(void* p, size_t cls) {
    if (!pool_give(pmu_, pinned_pool_, pinned_pooled_bytes_, (size_t)16 << 20, p, cls)) (void)hipHostFree(p);
}

void Engine::release_tables(void* p, size_t cls) {
    // beyond 64 MiB, blocks are freed (rare: a cache of large programs)
    if (!pool_give(pmu_, pool_, pooled_bytes_, (size_t)64 << 20, p, cls)) (void)hipFree(p);
}

void Engine::retire(std::vector<std::shared_ptr<ProgramSet>>&& evicted) {
#ifndef ECG_TEST_TSAN_SEEDED_RACE  // test hook: tools/tsan_host.sh seeded must report this unlocked push as a race
    std::lock_guard<std::mutex> lk(rmu_);
#endif
    for (auto& ps : evicted) retired_.push_back(std::move(ps));
}

hipStream_t stream_key(hipStream_t st) {
#ifdef ECG_TEST_PER_THREAD_SHARED_KEY  // test hook: round 4's one key for every thread's per-thread stream
    return st;                         // (tools/tsan_host.sh sharedkey must report a device-time hazard)
#endif
    if (st != hipStreamPerThread) return st;
    static std::atomic<uintptr_t> next{1};
    static thread_local const uintptr_t key = (next.fetch_add(1, std::memory_order_relaxed) << 1) | 1;
    return (hipStream_t)key;
}

// One pass over the retired sets (ProgramSet's retirement comment):
//   1. every unheld set's uncovered stream that may be named now -- `current` (a stream the caller handed
//      the library in the call in progress) or a stream that is never destroyed -- gets a cover event,
//      one record per stream per pass;
//   2. sets whose covers (and upload) have all fired are freed;
//   3. the cover mask is rebuilt from the streams still waiting;
//   4. unheld sets that cannot be covered (streams not seen again, overflow) beyond ECG_OPT_GRAVEYARD: the
//      caller synchronizes the device outside the lock and frees them (sync_and_free_unheld).
void Engine::sweep_retired(hipStream_t current, bool has_current) {
    bool over = false;
    {
        std::vector<std::shared_ptr<ProgramSet>> dead;  // destroyed after the lock is released
        std::lock_guard<std::mutex> lk(rmu_);
        over = sweep_locked(current, has_current, dead);
    }
    if (over) (void)sync_and_free_unheld();  // the graveyard outgrew ECG_OPT_GRAVEYARD
}

// A launch on st hit the cover mask: cover the unheld retired sets that wait for st's key (one event record
// on st, the caller's handle: for hipStreamPerThread, this thread's stream, the one the key names).
void Engine::cover_retired(hipStream_t st) {
    const hipStream_t key = stream_key(st);
    std::lock_guard<std::mutex> lk(rmu_);
    auto it = waiting_.find(key);
    if (it == waiting_.end()) return;  // another stream with the same mask bit
    std::shared_ptr<ProgramSet::CoverEvent> cover;
    auto& v = it->second;
    for (size_t i = 0; i < v.size();) {
        std::shared_ptr<ProgramSet> ps = v[i].lock();
        if (ps && ps.use_count() > 2) {  // still held by a caller (beyond retired_ and `ps`)
            i++;
            continue;
        }
        if (ps) {
            if (!cover && !(cover = record_cover(this, st))) return;
            std::lock_guard<std::mutex> sk(ps->smu);
            for (int e = 0; e < ps->nslots; e++)
                if (ps->slots[e].st == key && !ps->slots[e].cover) ps->slots[e].cover = cover;
        }
        v[i] = std::move(v.back());
        v.pop_back();
    }
    if (v.empty()) {
        waiting_.erase(it);
        uint64_t mask = 0;
        for (auto& kv : waiting_) mask |= stream_bit(kv.first);
        cover_mask_.store(mask, std::memory_order_relaxed);
    }
}

bool Engine::sweep_locked(hipStream_t current, bool has_current, std::vector<std::shared_ptr<ProgramSet>>& dead) {
    if (retired_.empty()) {
        waiting_.clear();
        cover_mask_.store(0, std::memory_order_relaxed);
        return false;
    }
    // slots hold stream keys: a slot is covered on `current` (the caller's handle, which names the slot's
    // stream in this thread) when its key is current's, and at once when it is the null stream
    const hipStream_t cur_key = has_current ? stream_key(current) : nullptr;
    std::shared_ptr<ProgramSet::CoverEvent> made[2];  // current, null stream
    auto cover_for = [&](hipStream_t key) -> std::shared_ptr<ProgramSet::CoverEvent> {
        const int i = (has_current && key == cur_key) ? 0 : key == nullptr ? 1 : -1;
        if (i < 0) return nullptr;
        if (!made[i]) made[i] = record_cover(this, i == 0 ? current : nullptr);
        return made[i];
    };
    size_t graveyard = 0;
    waiting_.clear();
    for (size_t i = 0; i < retired_.size();) {
        ProgramSet& ps = *retired_[i];
        const bool unheld = retired_[i].use_count() == 1;
        bool done = unheld;
        {
            std::lock_guard<std::mutex> sk(ps.smu);
            for (int e = 0; e < ps.nslots; e++) {
                ProgramSet::StreamSlot& sl = ps.slots[e];
                if (!sl.cover && unheld && (sl.st == nullptr || (has_current && sl.st == cur_key)))
                    sl.cover = cover_for(sl.st);
                if (!sl.cover) {
                    if (unheld) waiting_[sl.st].push_back(retired_[i]);
                    done = false;
                } else if (done) {
                    done = hipEventQuery(sl.cover->ev) == hipSuccess;
                }
            }
            if (ps.overflow) done = false;
            if (done && !ps.ready.load(std::memory_order_acquire)) done = hipEventQuery(ps.ready_ev) == hipSuccess;
        }
        if (done) {
            dead.push_back(std::move(retired_[i]));
            retired_[i] = std::move(retired_.back());
            retired_.pop_back();
            continue;
        }
        if (unheld) graveyard++;
        i++;
    }
    uint64_t mask = 0;
    for (auto& kv : waiting_) mask |= stream_bit(kv.first);
    cover_mask_.store(mask, std::memory_order_relaxed);
    return graveyard > (size_t)get_option(ECG_OPT_GRAVEYARD);
}

// Synchronize the engine's device WITHOUT holding the retirement lock (launches that hit the cover mask
// take it), then free the sets that nobody held before the synchronize began: their launches were all
// enqueued by then.  Sets are named by serial number, not address (a freed set's address may be reused).
size_t Engine::sync_and_free_unheld() {
    std::vector<uint64_t> before;
    {
        std::lock_guard<std::mutex> lk(rmu_);
        for (auto& ps : retired_)
            if (ps.use_count() == 1) before.push_back(ps->serial);
    }
    bool synced;
    {
        DeviceGuard on(device_);
        synced = hipDeviceSynchronize() == hipSuccess;
    }
    std::vector<std::shared_ptr<ProgramSet>> dead;
    std::lock_guard<std::mutex> lk(rmu_);
    if (synced) {
        std::sort(before.begin(), before.end());
        for (size_t i = 0; i < retired_.size();) {
            if (std::binary_search(before.begin(), before.end(), retired_[i]->serial)) {
                dead.push_back(std::move(retired_[i]));
                retired_[i] = std::move(retired_.back());
                retired_.pop_back();
                continue;
            }
            i++;
        }
    }
    (void)sweep_locked(nullptr, false, dead);  // rebuilds the waiting index and the cover mask
    return retired_.size();
}

size_t Engine::retired_pending() {
    std::vector<std::shared_ptr<ProgramSet>> dead;
    std::lock_guard<std::mutex> lk(rmu_);
    (void)sweep_locked(nullptr, false, dead);
    return retired_.size();
}

size_t Engine::reclaim() { return sync_and_free_unheld(); }

size_t Engine::cache_size() {
    std::shared_lock<std::shared_mutex> lk(mu_);
    return cache_.size();
}

std::shared_ptr<ProgramSet> Engine::program_set(const std::vector<LinearOp>& progs, int* status, hipStream_t st) {
    return program_set(progs.data(), progs.size(), status, st);
}

std::shared_ptr<ProgramSet> Engine::program_set(const LinearOp* progs, size_t nprogs, int* status, hipStream_t st) {
    *status = ECG_OK;
    if (nprogs == 0) {
        *status = ECG_EINVAL;
        return nullptr;
    }
    const int k = progs[0].k_in(), m = progs[0].m_out();
    if (k < 1 || m < 1) {
        *status = ECG_EINVAL;
        return nullptr;
    }
    thread_local std::string key;  // per thread: no allocation per lookup
    key.clear();
    key.reserve(16 + nprogs * (size_t)(k * m + 4 * (k + m)));
    auto put = [&](const void* p, size_t n) { key.append((const char*)p, n); };
    const int np = (int)nprogs;
    put(&k, 4);
    put(&m, 4);
    put(&np, 4);
    bool binary = true;
    for (size_t pi = 0; pi < nprogs; pi++) {
        const LinearOp& op = progs[pi];
        if (op.k_in() != k || op.m_out() != m || op.coef.size() != (size_t)k * m) {
            *status = ECG_EINVAL;
            return nullptr;
        }
        put(op.coef.data(), op.coef.size());
        put(op.src_ids.data(), op.src_ids.size() * 4);
        put(op.dst_ids.data(), op.dst_ids.size() * 4);
        binary &= op_is_binary(op);
    }
    {
        std::shared_lock<std::shared_mutex> lk(mu_);
        auto it = cache_.find(key);
        if (it != cache_.end()) {
            it->second.last_use->store(tick_.fetch_add(1, std::memory_order_relaxed) + 1, std::memory_order_relaxed);
            return it->second.ps;
        }
    }
    auto ps = std::make_shared<ProgramSet>();
    static std::atomic<uint64_t> serials{0};
    ps->serial = ++serials;
    ps->nprog = np;
    ps->k = k;
    ps->m = m;
    ps->MT = std::min(m, binary ? kMaxMTBin : kMaxMT);
    ps->rtiles = (m + ps->MT - 1) / ps->MT;
    ps->binary = binary;
    const size_t per_prog = (size_t)ps->rtiles * k * ps->MT;
    std::vector<CoefTab> tabs(per_prog * np);
    std::vector<int> src((size_t)np * k), dst((size_t)np * m);
    for (int pi = 0; pi < np; pi++) {
        const LinearOp& op = progs[pi];
        for (int rt = 0; rt < ps->rtiles; rt++)
            for (int j = 0; j < k; j++)
                for (int p = 0; p < ps->MT; p++) {
                    const int row = rt * ps->MT + p;
                    const int c = row < m ? op.coef[(size_t)row * k + j] : 0;
                    make_coef_tab(c, &tabs[pi * per_prog + ((size_t)rt * k + j) * ps->MT + p]);
                }
        std::copy(op.src_ids.begin(), op.src_ids.end(), src.begin() + (size_t)pi * k);
        std::copy(op.dst_ids.begin(), op.dst_ids.end(), dst.begin() + (size_t)pi * m);
    }
    auto fail = [&](hipError_t e, const char* what) {
        set_last_error(std::string(what) + ": " + hipGetErrorString(e));
        *status = ECG_EHIP;
        return nullptr;
    };
    hipError_t e;
    // one device block: tables, then source ids, then destination ids
    const size_t tab_bytes = tabs.size() * sizeof(CoefTab), src_off = tab_bytes,
                 dst_off = src_off + ((src.size() * sizeof(int) + 15) & ~(size_t)15),
                 total = dst_off + dst.size() * sizeof(int);
    std::vector<uint8_t> host(total, 0);
    memcpy(host.data(), tabs.data(), tab_bytes);
    memcpy(host.data() + src_off, src.data(), src.size() * sizeof(int));
    memcpy(host.data() + dst_off, dst.data(), dst.size() * sizeof(int));
    ps->owner = this;
    ps->mem = acquire_tables(total, &ps->mem_class, &e);
    if (!ps->mem) return fail(e, "hipMalloc(program tables)");
    ps->d_tabs = (CoefTab*)ps->mem;
    ps->d_src = (int*)((uint8_t*)ps->mem + src_off);
    ps->d_dst = (int*)((uint8_t*)ps->mem + dst_off);
    // The upload goes on the requesting stream, asynchronously, ahead of the launch that needs it: no
    // host wait, and no other stream involved (streams share the runtime's few hardware queues, so a
    // private upload stream could sit behind another thread's queued work).  Launches on other streams
    // wait for `ready_ev` until it has fired (ensure_ready).  The host bytes stay with the set until then.
    if ((e = hipEventCreateWithFlags(&ps->ready_ev, hipEventDisableTiming)) != hipSuccess)
        return fail(e, "hipEventCreate(program tables)");
    ps->pinned = acquire_pinned(total, &ps->pinned_class, &e);
    if (!ps->pinned) return fail(e, "hipHostMalloc(program tables)");
    memcpy(ps->pinned, host.data(), total);
    ps->first_stream = stream_key(st);
    if ((e = hipMemcpyAsync(ps->mem, ps->pinned, total, hipMemcpyHostToDevice, st)) != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return fail(e, "hipMemcpyAsync(program tables)");
    }
    if ((e = hipEventRecord(ps->ready_ev, st)) != hipSuccess) {
        (void)hipStreamSynchronize(st);  // the copy may be in flight: the memory must not go back yet
        ps->ready.store(true);
        return fail(e, "hipEventRecord(program tables)");
    }
    std::vector<std::shared_ptr<ProgramSet>> evicted;  // retired outside the lock
    {
        std::unique_lock<std::shared_mutex> lk(mu_);
        auto it = cache_.find(key);
        if (it != cache_.end()) {  // another thread won the race
            it->second.last_use->store(++tick_, std::memory_order_relaxed);
            return it->second.ps;
        }
        const size_t cap = (size_t)std::max(2LL, get_option(ECG_OPT_PROGRAM_CACHE));
        if (cache_.size() >= cap) {  // keep the cap / 2 most recently used programs
            std::vector<uint64_t> uses;
            uses.reserve(cache_.size());
            for (auto& kv : cache_) uses.push_back(kv.second.last_use->load(std::memory_order_relaxed));
            const size_t drop = cache_.size() - cap / 2;
            std::nth_element(uses.begin(), uses.begin() + drop, uses.end());
            const uint64_t cut = uses[drop];
            for (auto i = cache_.begin(); i != cache_.end();) {
                if (i->second.last_use->load(std::memory_order_relaxed) < cut) {
                    evicted.push_back(std::move(i->second.ps));
                    i = cache_.erase(i);
                } else {
                    ++i;
                }
            }
        }
        cache_.emplace(key, CacheEntry{ps, std::make_unique<std::atomic<uint64_t>>(++tick_)});
    }
    if (!evicted.empty()) retire(std::move(evicted));
    sweep_retired(st, true);  // st: the caller's stream, alive for this call
    return ps;
}

}  // namespace ecg
