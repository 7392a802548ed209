// The candidate plan of a check matrix H, the heal plan on top of it, and the host steps from a plan to its launch
// descriptor, shared by the entry points that test "does block b alone explain this syndrome?": locate.cpp
// (libecg_locate.so), heal.cpp (libecg_heal.so) and heal2.cpp (libecg_heal2.so).  Header-only; no kernel launch and no
// state.
#pragma once
#include <string.h>

#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "check_common.hpp"
#include "gf256.hpp"
#include "locate_kernels.hpp"

namespace ecg {

struct CandidatePlan {
    Check chk;
    LinearOp ratio;  // r x n: H[q][b] / H[p0(b)][b]; an all-zero column for a zero column of H
    unsigned p0[kInlineSrc / 8];
    int n = 0, r = 0;
};

inline CandidatePlan make_plan(int n, int r, const int* H, const int* src_ids, bool consecutive) {
    CandidatePlan pl;
    pl.n = n;
    pl.r = r;
    pl.chk = make_check(n, r, H, src_ids, consecutive);
    pl.ratio.src_ids = iota(n);
    pl.ratio.dst_ids = iota(r);
    pl.ratio.coef.assign((size_t)r * n, 0);
    memset(pl.p0, 0, sizeof(pl.p0));
    for (int b = 0; b < n; b++) {
        int p0 = 0;
        while (p0 < r && (H[(size_t)p0 * n + b] & 0xff) == 0) p0++;
        pl.p0[b >> 3] |= (p0 < r ? (unsigned)p0 : kNoPivot) << ((b & 7) * 4);
        if (p0 == r) continue;
        const int lead = H[(size_t)p0 * n + b] & 0xff;
        for (int q = p0; q < r; q++) pl.ratio.coef[(size_t)q * n + b] = (uint8_t)gf::div(H[(size_t)q * n + b], lead);
    }
    return pl;
}

inline unsigned pivot_of(const CandidatePlan& pl, int b) { return (pl.p0[b >> 3] >> ((b & 7) * 4)) & 15u; }

// What a correction needs on top of the candidate test: the error value is s_p0 / H[p0(b)][b].
struct HealPlan {
    CandidatePlan cand;
    LinearOp inv;  // 1 x n: 1 / H[p0(b)][b]; 0 for a zero column of H
};

inline HealPlan make_heal_plan(int n, int r, const int* H, const int* src_ids, bool consecutive) {
    HealPlan hp;
    hp.cand = make_plan(n, r, H, src_ids, consecutive);
    hp.inv.src_ids = iota(n);
    hp.inv.dst_ids = iota(1);
    hp.inv.coef.assign((size_t)n, 0);
    for (int b = 0; b < n; b++) {
        const unsigned p0 = pivot_of(hp.cand, b);
        if (p0 != kNoPivot) hp.inv.coef[b] = (uint8_t)gf::inv(H[(size_t)p0 * n + b] & 0xff);
    }
    return hp;
}

// ECG_OK for a check one lane can hold (r <= kMaxMT, n <= kInlineSrc), else its refusal in the words of library `lib`;
// `tail` ends the advice.
struct TooLarge {
    const char *lib, *tail;
    int operator()(long long n, int r) const {
        if (r <= kMaxMT && n <= kInlineSrc) return ECG_OK;
        set_last_error(std::string(lib) + ": r = " + std::to_string(r) + ", n = " + std::to_string(n) +
                       " exceeds r <= " + std::to_string(kMaxMT) + ", n <= " + std::to_string(kInlineSrc) +
                       " (one lane holds all r syndromes); product codes stay with ecg_scrub_suspects" + tail);
        return ECG_EINVAL;
    }
};

// The table sets a candidate launch reads: the check's, the ratios', then those of the caller's further ops.
struct CandidateTables {
    std::shared_ptr<ProgramSet> set[4];
    int count = 0;
    const ProgramSet& extra(int i) const { return *set[2 + i]; }
    void note_launch(hipStream_t st) const {
        for (int i = 0; i < count; i++) Engine::instance().note_launch(*set[i], st);
    }
};

// The LocateLaunch of a plan, up to the launch: flush the thread's batch scope, fetch the tables of the check, of the
// ratios and of `extra` (at most two ops, one row tile each) into `t`, fill `a` (`fill` sets its sources) and zero the
// S x ncounters counters; `zeroing` labels a failure of that.
template <class Fill>
int prepare_launch(const CandidatePlan& pl, std::initializer_list<const LinearOp*> extra, int ncounters, long long B,
                   int S, const int* d_stripe_ids, unsigned* d_counters, const char* zeroing, hipStream_t st, Fill fill,
                   LocateLaunch& a, CandidateTables& t) {
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;
    const LinearOp* ops[4] = {&pl.chk.op, &pl.ratio};
    t.count = 2;
    for (const LinearOp* op : extra) ops[t.count++] = op;
    int status = ECG_OK;
    for (int i = 0; i < t.count; i++) {
        t.set[i] = Engine::instance().program_set(ops[i], 1, &status, st);
        if (!t.set[i]) return status;
    }
    for (int i = 0; i < t.count; i++)
        if (const int rc = t.set[i]->ensure_ready(st); rc != ECG_OK) return rc;
    const ProgramSet &ps = *t.set[0], &rs = *t.set[1];
    if (ps.MT != pl.r || ps.rtiles != 1) return ECG_EINVAL;
    for (int i = 1; i < t.count; i++)
        if (t.set[i]->MT != (int)ops[i]->dst_ids.size() || t.set[i]->rtiles != 1 ||
            t.set[i]->k != (int)ops[i]->src_ids.size())
            return ECG_EINVAL;
    memset(&a, 0, sizeof(a));
    a.g.tabs = ps.d_tabs;
    a.g.src_ids = ps.d_src;
    a.g.dst_ids = ps.d_dst;
    a.g.stripe_of = d_stripe_ids;
    a.g.B = B;
    a.g.k = ps.k;
    a.g.m = ps.m;
    a.g.S = S;
    a.g.MT = ps.MT;
    a.g.rtiles = ps.rtiles;
    a.g.binary = 0;  // the GENERAL flavour always: the tables of 0 and 1 are exact
    a.votes = d_counters;
    a.ident = pl.chk.ident;
    a.ident_base = pl.chk.ident_base;
    a.ratios = rs.d_tabs;
    a.n = pl.n;
    memcpy(a.p0, pl.p0, sizeof(a.p0));
    fill(a.g);
    if (const hipError_t e = hipMemsetAsync(d_counters, 0, (size_t)S * (size_t)ncounters * sizeof(unsigned), st);
        e != hipSuccess)
        return hip_fail(e, zeroing);
    return ECG_OK;
}

}  // namespace ecg
