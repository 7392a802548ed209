// Planning of a batch-scope flush and of a host-tier call: pure host logic (recorded calls, scratch ranges and
// composition, the group scheduler, plan classes, block classification), fuzzed on the CPU by
// tests/sanitize/host_fuzz.cpp.  Nothing here calls HIP; the one runtime include is for hipStream_t, which
// recorded calls carry as an opaque value that is only ever compared.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <memory>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/ecg.h"  // status codes ECG_*
#include "matrix.hpp"

namespace ecg {

class Engine;  // named by recorded calls, never dereferenced here

// One recorded device-tier call: its plan (shared by calls with an equal plan) over its block space.
struct DeferredCall {
    Engine* eng;
    hipStream_t st;
    long long B;
    std::shared_ptr<const std::vector<LinearOp>> ops;
    std::vector<uint8_t*> blocks;  // device pointers
};

// Scratch ranges of a scope (merged, disjoint).  A block [p, p + B) is scratch if one range holds it.
class ScratchRanges {
public:
    void add(uintptr_t lo, uintptr_t hi);
    bool holds(const void* p, long long B) const;
    bool empty() const { return r_.empty(); }
    void clear() { r_.clear(); }

private:
    std::vector<std::pair<uintptr_t, uintptr_t>> r_;  // sorted by start, disjoint, [lo, hi)
};

// Scratch composition (pure host logic, no HIP; fuzzed in tests/sanitize/host_fuzz.cpp against a
// sequential interpreter).  Walks the recorded calls in order, keeping for every scratch block written
// so far the linear combination of real blocks it holds (an "expression").  A call reading a scratch
// block with an expression reads that combination's blocks instead (coefficients multiplied out over
// GF(2^8)); a call writing a scratch block only records the expression.  An expression is written for
// real ("materialised") before any block it reads is overwritten, when a reader runs on another
// stream / device / block size, and -- unless `scope_end` -- for every expression left at the end
// (a mid-scope flush must leave memory as the sequential calls would).  At scope end unconsumed
// scratch contents are undefined: that is the contract of batch_scratch.  Blocks are compared by
// address, as in the hazard check (blocks of one scope are identical or disjoint).  Calls that touch
// neither scratch nor an expression pass through unchanged (their plan pointer kept).
std::vector<DeferredCall> compose_scratch(std::vector<DeferredCall>&& q, const ScratchRanges& scratch,
                                          bool scope_end, long long* materialised);

// Block addresses are often aligned to the block size (1 MiB and up): a full 64-bit mix (splitmix64's
// finaliser) so that their low bits, which pick the slot, are not mostly zero.
inline size_t ptr_hash(uintptr_t p) {
    unsigned long long x = (unsigned long long)p;
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return (size_t)x;
}

// Open-addressing map block address -> V for one flush; V{} is "never touched" and entries are never erased
// (one flush touches few distinct addresses).  At least kMinSlots slots, at most half of them used.
template <class V, size_t kMinSlots>
class PtrMap {
public:
    V& at(const void* ptr) {
        if ((count_ + 1) * 2 > slots_.size()) grow();
        const uintptr_t p = (uintptr_t)ptr;
        for (size_t i = ptr_hash(p) & mask_;; i = (i + 1) & mask_) {
            if (slots_[i].p == p) return slots_[i].v;
            if (slots_[i].p == 0) {
                slots_[i] = Slot{p, V{}};
                count_++;
                return slots_[i].v;
            }
        }
    }
    const V* find(const void* ptr) const {
        if (slots_.empty()) return nullptr;
        const uintptr_t p = (uintptr_t)ptr;
        for (size_t i = ptr_hash(p) & mask_;; i = (i + 1) & mask_) {
            if (slots_[i].p == p) return &slots_[i].v;
            if (slots_[i].p == 0) return nullptr;
        }
    }
    // empty, with room for n addresses without growing (the flush's scheduler reuses one per thread)
    void reset(size_t n) {
        size_t want = kMinSlots;
        while (want < 4 * n) want <<= 1;
        if (slots_.size() < want) {
            slots_.assign(want, Slot{0, V{}});
            mask_ = want - 1;
        } else if (count_) {
            std::fill(slots_.begin(), slots_.end(), Slot{0, V{}});
        }
        count_ = 0;
    }
    template <class F>
    void for_each(F f) const {
        for (const Slot& s : slots_)
            if (s.p) f((uint8_t*)s.p, s.v);
    }

private:
    struct Slot {
        uintptr_t p;
        V v;
    };
    void grow() {
        std::vector<Slot> old;
        old.swap(slots_);
        slots_.assign(old.empty() ? kMinSlots : old.size() * 2, Slot{0, V{}});
        mask_ = slots_.size() - 1;
        count_ = 0;
        for (const Slot& s : old)
            if (s.p) at((const void*)s.p) = s.v;
    }
    std::vector<Slot> slots_;
    size_t mask_ = 0, count_ = 0;
};

// Block address -> the latest group (index + 1) that read / wrote it, for the flush's scheduler.
struct GroupMark {
    int rd = 0, wr = 0;
};
class PtrGroups : public PtrMap<GroupMark, 1024> {
public:
    int last_write(const void* ptr) const { const GroupMark* s = find(ptr); return s ? s->wr : 0; }
    int last_touch(const void* ptr) const { const GroupMark* s = find(ptr); return s ? std::max(s->rd, s->wr) : 0; }
};

// Grouping of the flush (pure host logic, no HIP; fuzzed against a quadratic legality check in
// tests/sanitize/host_fuzz.cpp).  Calls [0, n) in program order; key(c) >= 0 names the call's plan
// class (same plan or single-op shape, block size, stream, device).  Each call joins the EARLIEST group of
// its key that comes after every group holding an earlier call it depends on (one that writes a block it
// reads or writes, or reads a block it writes); if there is none it opens a new group at the end.
// Launching the groups in index order, each group's calls in one launch, therefore respects every
// dependence of the program order (two dependent calls always sit in groups i < j), and independent calls
// of one plan -- the reference's per-stripe loop, even with several plans interleaved per stripe -- share a
// launch.  Earliest, not latest: in a two-block repair whose second plan reads the block its first plan
// rebuilt (handle_repair.cpp per plan), every stripe's first plan shares one group and every second plan
// the next, instead of a new pair of groups per stripe (a launch per stripe).  A call placed before a later
// group of its key depends on nothing in between, and calls after it see its group in `seen`.
// reads(c, f) / writes(c, f) call f(address) per block call c reads / writes.  Returns the groups,
// each listing its calls in program order.
template <class Key, class Reads, class Writes>
std::vector<std::vector<size_t>> schedule_groups(size_t n, Key key, Reads reads, Writes writes) {
    std::vector<std::vector<size_t>> groups;
    std::vector<std::vector<int>> of_key;  // key -> its groups' index + 1, ascending
    thread_local PtrGroups seen;
    seen.reset(4 * n);
    for (size_t c = 0; c < n; c++) {
        int lo = 0;  // the call must go into a group with index + 1 > lo
        reads(c, [&](const void* p) { lo = std::max(lo, seen.last_write(p)); });
        writes(c, [&](const void* p) { lo = std::max(lo, seen.last_touch(p)); });
        const int kc = key(c);
        if ((size_t)kc >= of_key.size()) of_key.resize((size_t)kc + 1);
        std::vector<int>& mine = of_key[(size_t)kc];
        const auto it = std::upper_bound(mine.begin(), mine.end(), lo);
        int g1;
        if (it != mine.end()) {
            g1 = *it;
        } else {
            groups.emplace_back();
            g1 = (int)groups.size();
            mine.push_back(g1);
        }
        groups[(size_t)g1 - 1].push_back(c);
        reads(c, [&](const void* p) { GroupMark& s = seen.at(p); s.rd = std::max(s.rd, g1); });
        writes(c, [&](const void* p) { GroupMark& s = seen.at(p); s.wr = std::max(s.wr, g1); });
    }
    return groups;
}

#pragma GCC visibility push(hidden)  // the rest is the engine's own: not among libecg's dynamic symbols

bool same_ops(const std::vector<LinearOp>& a, const std::vector<LinearOp>& b);

// Plan classes of a flush: calls with equal plans (by content), block size, stream and device share a
// class.  Recording shares the plan pointer between consecutive equal calls, so most lookups hit the
// pointer cache; composed calls are interned by content.  Single-op plans of one shape (k_in, m_out) share a
// class whatever their coefficients: the per-stripe repairs of a batch (a pattern per stripe, each composing
// to its own matrix) then go out as ONE multi-program pointer-table launch per scope instead of a launch per
// pattern (families workload: RS(12,4) repairs 16 patterns x 4 scopes -> 4 launches).
class PlanClasses {
public:
    int plan_of_last() const { return last_plan_; }
    int of(const DeferredCall& c) {
        auto pk = by_ptr_.find(c.ops.get());
        int plan;
        if (pk != by_ptr_.end()) {
            plan = pk->second;
        } else {
            size_t h = 1469598103934665603ull;
            auto mix = [&](const void* p, size_t n) {
                const uint8_t* b = (const uint8_t*)p;
                for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
            };
            for (const LinearOp& op : *c.ops) {
                mix(op.src_ids.data(), op.src_ids.size() * 4);
                mix(op.dst_ids.data(), op.dst_ids.size() * 4);
                mix(op.coef.data(), op.coef.size());
                mix("|", 1);
            }
            plan = -1;
            for (int id : by_hash_[h])
                if (same_ops(*plans_[id], *c.ops)) plan = id;
            if (plan < 0) {
                plan = (int)plans_.size();
                plans_.push_back(c.ops);
                by_hash_[h].push_back(plan);
            }
            by_ptr_[c.ops.get()] = plan;
        }
        last_plan_ = plan;
        int cls_plan = plan;
        if (c.ops->size() == 1 && (*c.ops)[0].k_in() > 0) {
            const auto sk = std::make_pair((*c.ops)[0].k_in(), (*c.ops)[0].m_out());
            auto si = shapes_.find(sk);
            if (si == shapes_.end()) si = shapes_.emplace(sk, (int)shapes_.size()).first;
            cls_plan = -1 - si->second;
        }
        const auto key = std::make_tuple(cls_plan, c.eng, c.st, c.B);
        auto it = cls_.find(key);
        if (it != cls_.end()) return it->second;
        const int id = (int)cls_.size();
        cls_.emplace(key, id);
        return id;
    }

private:
    std::unordered_map<const void*, int> by_ptr_;
    std::unordered_map<size_t, std::vector<int>> by_hash_;
    std::vector<std::shared_ptr<const std::vector<LinearOp>>> plans_;
    std::map<std::pair<int, int>, int> shapes_;
    std::map<std::tuple<int, Engine*, hipStream_t, long long>, int> cls_;
    int last_plan_ = -1;
};

// Walks a call's ops in order and names every block id it reads (read(id)) and writes (write(id)).
// ECG_EINVAL at the first id outside [0, nblocks) or block that is null.  Every tier validates its calls
// through this (the device tier with nothing to note), so "a valid call" is one rule.
template <class Read, class Write>
int walk_block_ids(const std::vector<LinearOp>& ops, uint8_t* const* blocks, int nblocks, Read read, Write write) {
    for (const LinearOp& op : ops) {
        for (int id : op.src_ids) {
            if (id < 0 || id >= nblocks || !blocks[id]) return ECG_EINVAL;
            read(id);
        }
        for (int id : op.dst_ids) {
            if (id < 0 || id >= nblocks || !blocks[id]) return ECG_EINVAL;
            write(id);
        }
    }
    return ECG_OK;
}

// What the host tier does with each block of a call: `upload` -- read before any op of the call wrote it, so
// the caller's bytes must reach the device first; `written` -- comes back to the caller; `used` -- touched at
// all, so it needs a device slot.  This decides which host blocks are uploaded: a block wrongly left out is
// computed from stale device bytes.  The synchronous call and the deferred recording each keep one of these
// per thread (no allocation per call).
struct BlockUse {
    std::vector<char> upload, written, used;
    int classify(const std::vector<LinearOp>& ops, uint8_t* const* blocks, int nblocks) {
        upload.assign(nblocks, 0);
        written.assign(nblocks, 0);
        used.assign(nblocks, 0);
        return walk_block_ids(
            ops, blocks, nblocks,
            [&](int id) {
                if (!written[id]) upload[id] = 1;
                used[id] = 1;
            },
            [&](int id) { written[id] = used[id] = 1; });
    }
};

#pragma GCC visibility pop
}  // namespace ecg
