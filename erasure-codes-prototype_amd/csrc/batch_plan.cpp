// Scratch ranges and scratch composition of a batch-scope flush.  See batch_plan.hpp.
#include "batch_plan.hpp"

#include "gf256.hpp"

namespace ecg {

bool same_ops(const std::vector<LinearOp>& a, const std::vector<LinearOp>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].src_ids != b[i].src_ids || a[i].dst_ids != b[i].dst_ids || a[i].coef != b[i].coef) return false;
    return true;
}

// ScratchRanges: sorted disjoint [lo, hi); add() merges overlapping and touching ranges.
void ScratchRanges::add(uintptr_t lo, uintptr_t hi) {
    auto it = std::lower_bound(r_.begin(), r_.end(), std::make_pair(lo, (uintptr_t)0));
    if (it != r_.begin() && std::prev(it)->second >= lo) --it;
    auto e = it;
    while (e != r_.end() && e->first <= hi) {
        lo = std::min(lo, e->first);
        hi = std::max(hi, e->second);
        ++e;
    }
    it = r_.erase(it, e);
    r_.insert(it, {lo, hi});
}

bool ScratchRanges::holds(const void* p, long long B) const {
    const uintptr_t a = (uintptr_t)p;
    auto it = std::upper_bound(r_.begin(), r_.end(), std::make_pair(a, UINTPTR_MAX));
    if (it == r_.begin()) return false;
    --it;
    return a >= it->first && a + (uintptr_t)B <= it->second;
}

namespace {

// A linear combination of real blocks over GF(2^8): (block, coefficient) terms, coefficients != 0 once
// normalised.  Small (a partial repair combines <= k' blocks), so a flat vector.
using Term = std::pair<uint8_t*, uint8_t>;
using Terms = std::vector<Term>;

void add_term(Terms& t, uint8_t* p, int c) {
    if (!c) return;
    for (auto& x : t)
        if (x.first == p) {
            x.second ^= (uint8_t)c;
            return;
        }
    t.emplace_back(p, (uint8_t)c);
}

void drop_zero_terms(Terms& t) {
    t.erase(std::remove_if(t.begin(), t.end(), [](const Term& x) { return x.second == 0; }), t.end());
}

// Block address -> int, -1 = absent (an entry is "erased" by setting it to -1; the map lives for one flush).
class PtrInt {
public:
    int get(const void* ptr) const { const Idx* s = m_.find(ptr); return s ? s->v : -1; }
    int& ref(const void* ptr) { return m_.at(ptr).v; }
    void reset(size_t n) { m_.reset(n); }
    template <class F>
    void for_each(F f) const {
        m_.for_each([&](uint8_t* p, const Idx& s) {
            if (s.v >= 0) f(p, s.v);
        });
    }

private:
    struct Idx {
        int v = -1;
    };
    PtrMap<Idx, 256> m_;
};

// compose_scratch's state (engine.hpp).  Expressions live in a slab indexed from `ex_`; `users_` maps a
// real block to a list of (expression, generation) nodes that read it -- a node whose generation is no
// longer its slot's is stale.  Composed plans are interned by content, so the flush's plan classes see
// one plan pointer per distinct composed map.
class Composer {
public:
    std::vector<DeferredCall> out;
    long long nmat = 0;

    // One Composer per thread, reused by every flush (its tables and buffers keep their capacity).
    void reset(const ScratchRanges& s, size_t ncalls) {
        scratch_ = &s;
        out.clear();
        out.reserve(ncalls);
        nmat = 0;
        slab_used_ = 0;
        free_.clear();
        uses_.clear();
        ex_.reset(ncalls);
        users_.reset(4 * ncalls);
        if (plans_.size() > 4096) plans_.clear();  // interned composed plans: bounded
    }

    void call(DeferredCall&& c) {
        bool touches = false;
        for (const LinearOp& op : *c.ops) {
            for (int id : op.src_ids) touches = touches || ex_.get(c.blocks[id]) >= 0;
            for (int id : op.dst_ids) touches = touches || scratch_->holds(c.blocks[id], c.B);
        }
        if (!touches) {
            // expressions reading blocks this call overwrites go out first, together as one op
            if (!uses_.empty()) {
                fast_.clear();
                start_collect(&fast_, c.eng, c.B);
                for (const LinearOp& op : *c.ops)
                    for (int id : op.dst_ids) before_write(c.blocks[id]);
                collect_ = nullptr;
                if (fast_.n) emit(c.eng, c.st, c.B, fast_);
            }
            out.push_back(std::move(c));
            return;
        }
        for (const LinearOp& op : *c.ops) one_op(c, op);
    }

    void finish(bool scope_end) {
        if (scope_end) return;  // unconsumed scratch contents are undefined after the scope
        std::vector<uint8_t*> left;  // a mid-scope flush leaves memory as the sequential calls would
        ex_.for_each([&](uint8_t* p, int) { left.push_back(p); });
        std::sort(left.begin(), left.end());
        write_out(left);
    }

private:
    struct Expr {
        Engine* eng;
        hipStream_t st;
        long long B;
        uint8_t* self;
        uint32_t gen;
        Terms t;
    };
    struct Use {
        int expr;
        uint32_t gen;
        int next;
    };
    // rows (block, terms) of one op being built; elements keep their capacity across uses
    struct RowBuf {
        std::vector<std::pair<uint8_t*, Terms>> v;
        size_t n = 0;
        void clear() { n = 0; }
        Terms& add(uint8_t* d) {
            if (n == v.size()) v.emplace_back();
            v[n].first = d;
            return v[n++].second;
        }
    };

    void one_op(const DeferredCall& c, const LinearOp& op) {
        const int k = op.k_in(), m = op.m_out();
        // inputs whose expression was recorded on another stream / device / block size are written for
        // real first -- before any row is built, since writing them out can overwrite blocks other
        // expressions (and so the rows) read
        std::vector<uint8_t*> foreign;
        for (int id : op.src_ids) {
            const int e = ex_.get(c.blocks[id]);
            if (e >= 0 && !(slab_[e].eng == c.eng && slab_[e].st == c.st && slab_[e].B == c.B))
                foreign.push_back(c.blocks[id]);
        }
        if (!foreign.empty()) write_out(foreign);
        if ((int)rows_.size() < m) rows_.resize((size_t)m);
        for (int p = 0; p < m; p++) {
            Terms& t = rows_[p];
            t.clear();
            for (int j = 0; j < k; j++) {
                const int cf = op.coef[(size_t)p * k + j];
                if (!cf) continue;
                uint8_t* src = c.blocks[op.src_ids[j]];
                const int e = ex_.get(src);
                if (e >= 0) {
                    for (const Term& x : slab_[e].t) add_term(t, x.first, gf::mul(cf, x.second));
                    continue;
                }
                add_term(t, src, cf);
            }
            drop_zero_terms(t);
        }
        // virtual writes first: a new expression may read a block this same op overwrites, and the real
        // writes below then write it out (into this op) like any other expression reading it.  A virtual
        // write leaves d's memory as it is, so expressions reading the real d stay valid.
        for (int p = 0; p < m; p++) {
            uint8_t* d = c.blocks[op.dst_ids[p]];
            if (!scratch_->holds(d, c.B)) continue;
            int& slot = ex_.ref(d);
            if (slot < 0) {
                if (!free_.empty()) {
                    slot = free_.back();
                    free_.pop_back();
                } else {
                    if (slab_used_ == slab_.size()) slab_.emplace_back();
                    slot = (int)slab_used_++;
                }
            }
            const int e = slot;
            Expr& x = slab_[e];
            x.eng = c.eng;
            x.st = c.st;
            x.B = c.B;
            x.self = d;
            x.gen = ++gen_;
            x.t.assign(rows_[p].begin(), rows_[p].end());
            for (const Term& u : x.t) {
                int& head = users_.ref(u.first);
                uses_.push_back(Use{e, x.gen, head});
                head = (int)uses_.size() - 1;
            }
        }
        real_.clear();
        start_collect(&real_, c.eng, c.B);
        for (int p = 0; p < m; p++) {
            uint8_t* d = c.blocks[op.dst_ids[p]];
            if (scratch_->holds(d, c.B)) continue;
            before_write(d);
            real_.add(d).assign(rows_[p].begin(), rows_[p].end());
        }
        collect_ = nullptr;
        if (real_.n) emit(c.eng, c.st, c.B, real_);
    }

    // While a call's writes are processed, expressions written out because the call overwrites a block
    // they read join the call's own op (`collect_`): one op reads every input before it writes any
    // output, so neither side sees the other's writes (a separate earlier call writing scratch block s
    // would clobber an s the op itself still reads).  An expression recorded on another stream of the same
    // device joins too: the flush orders its groups across streams (batch_flush), so the op is ordered
    // after the other stream's writes to the blocks the expression reads.  Written out on its own stream
    // instead, it would break the op's read-before-write when the two read each other's blocks (the
    // sequential interpreter of tests/sanitize/host_fuzz.cpp finds such cycles).
    void start_collect(RowBuf* rows, Engine* eng, long long B) {
        collect_ = rows;
        ceng_ = eng;
        cB_ = B;
    }

    void materialise(uint8_t* s) {
        int& slot = ex_.ref(s);
        if (slot < 0) return;
        const int e = slot;
        slot = -1;
        Expr& x = slab_[e];
        const Engine* eng = x.eng;
        Engine* eng_mut = x.eng;
        hipStream_t st = x.st;
        const long long B = x.B;
        Terms t;
        t.swap(x.t);
        x.gen = ++gen_;  // every node still naming this slot is stale now
        free_.push_back(e);
        before_write(s);
        if (collect_ && eng == ceng_ && B == cB_) {
            collect_->add(s).swap(t);
        } else {
            RowBuf one;
            one.add(s).swap(t);
            emit(eng_mut, st, B, one);
        }
        nmat++;
    }

    // Top level: write the expressions of `ss` out, with every expression they drag along, as ONE op
    // (expressions can read each other's real blocks both ways once a scratch block's expression read
    // its own old contents, so written one by one the second would read the first's new bytes).
    void write_out(const std::vector<uint8_t*>& ss) {
        RowBuf& rows = wo_;
        rows.clear();
        Engine* eng = nullptr;
        hipStream_t st = nullptr;
        long long B = 0;
        for (uint8_t* s : ss) {
            const int e = ex_.get(s);
            if (e < 0) continue;
            if (!collect_) {
                eng = slab_[e].eng;
                st = slab_[e].st;
                B = slab_[e].B;
                start_collect(&rows, eng, B);
            }
            materialise(s);
        }
        collect_ = nullptr;
        if (rows.n) emit(eng, st, B, rows);
    }

    // d is about to be overwritten: every expression still reading d is written out first
    void before_write(uint8_t* d) {
        if (uses_.empty()) return;
        const int h = users_.get(d);
        if (h < 0) return;
        users_.ref(d) = -1;
        for (int u = h; u >= 0; u = uses_[u].next) {
            const Use nd = uses_[u];
            Expr& x = slab_[nd.expr];
            if (x.gen != nd.gen) continue;  // stale: the slot was rewritten or written out since
            for (const Term& t : x.t)
                if (t.first == d) {
                    materialise(x.self);
                    break;
                }
        }
    }

    // One composed call writing rows[i].first = rows[i].second: inputs in first-appearance order (the same
    // for every stripe of one call pattern, so equal patterns intern to one plan), rows that combine to
    // nothing become a k_in = 0 op (zero bytes, what the sequential calls leave there).  A block written
    // twice by one op holds its last row (every row reads before any row writes).
    void emit(Engine* eng, hipStream_t st, long long B, const RowBuf& buf) {
        DeferredCall c{eng, st, B, nullptr, {}};
        const std::pair<uint8_t*, Terms>* rows = buf.v.data();
        const size_t nrows = buf.n;
        keep_.assign(nrows, 1);
        for (size_t i = 0; i < nrows; i++)
            for (size_t j = i + 1; j < nrows && keep_[i]; j++)
                if (rows[j].first == rows[i].first) keep_[i] = 0;
        ins_.clear();
        for (size_t i = 0; i < nrows; i++)
            if (keep_[i])
                for (const Term& x : rows[i].second)
                    if (std::find(ins_.begin(), ins_.end(), x.first) == ins_.end()) ins_.push_back(x.first);
        const int n = (int)ins_.size();
        // content key: n, then per kept row a zero flag or its n coefficients
        key_.assign((const uint8_t*)&n, (const uint8_t*)&n + sizeof n);
        c.blocks.reserve(ins_.size() + nrows);
        c.blocks.assign(ins_.begin(), ins_.end());
        for (size_t i = 0; i < nrows; i++) {
            if (!keep_[i]) continue;
            c.blocks.push_back(rows[i].first);
            key_.push_back(rows[i].second.empty() ? 0 : 1);
            if (rows[i].second.empty()) continue;
            const size_t base = key_.size();
            key_.resize(base + (size_t)n, 0);
            for (const Term& x : rows[i].second)
                key_[base + (size_t)(std::find(ins_.begin(), ins_.end(), x.first) - ins_.begin())] = x.second;
        }
        uint64_t h = 1469598103934665603ull;
        for (uint8_t b : key_) h = (h ^ b) * 1099511628211ull;
        auto& bucket = plans_[h];
        for (auto& pl : bucket)
            if (pl.first == key_) {
                c.ops = pl.second;
                out.push_back(std::move(c));
                return;
            }
        auto ops = std::make_shared<std::vector<LinearOp>>();
        LinearOp full, zero;
        for (int j = 0; j < n; j++) full.src_ids.push_back(j);
        int id = n;
        size_t at = sizeof n;
        for (size_t i = 0; i < nrows; i++) {
            if (!keep_[i]) continue;
            const bool nz = key_[at++];
            if (!nz) {
                zero.dst_ids.push_back(id++);
                continue;
            }
            full.dst_ids.push_back(id++);
            full.coef.insert(full.coef.end(), key_.begin() + (long)at, key_.begin() + (long)at + n);
            at += (size_t)n;
        }
        if (full.m_out() > 0) ops->push_back(std::move(full));
        if (zero.m_out() > 0) ops->push_back(std::move(zero));
        c.ops = ops;
        bucket.emplace_back(key_, std::move(ops));
        out.push_back(std::move(c));
    }

    const ScratchRanges* scratch_ = nullptr;
    std::vector<Expr> slab_;
    size_t slab_used_ = 0;
    std::vector<int> free_;
    PtrInt ex_, users_;
    std::vector<Use> uses_;
    uint32_t gen_ = 0;
    RowBuf* collect_ = nullptr;
    RowBuf real_, fast_, wo_;
    const Engine* ceng_ = nullptr;
    long long cB_ = 0;
    std::vector<Terms> rows_;
    std::vector<uint8_t*> ins_;
    std::vector<char> keep_;
    std::vector<uint8_t> key_;
    std::unordered_map<uint64_t, std::vector<std::pair<std::vector<uint8_t>, std::shared_ptr<const std::vector<LinearOp>>>>>
        plans_;
};

}  // namespace

std::vector<DeferredCall> compose_scratch(std::vector<DeferredCall>&& q, const ScratchRanges& scratch, bool scope_end,
                                          long long* materialised) {
    thread_local Composer cp;
    cp.reset(scratch, q.size());
    for (DeferredCall& c : q) cp.call(std::move(c));
    cp.finish(scope_end);
    if (materialised) *materialised = cp.nmat;
    std::vector<DeferredCall> out;
    out.swap(cp.out);
    return out;
}

}  // namespace ecg
