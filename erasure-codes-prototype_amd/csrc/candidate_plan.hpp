// The candidate plan of a check matrix H, and the host steps from a plan to its launch descriptor, shared by the entry
// points that test "does block b alone explain this syndrome?": locate.cpp (libecg_locate.so) and heal.cpp
// (libecg_heal.so).  Header-only; no kernel launch and no state.
#pragma once
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "capi_handle.hpp"
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

// The refusal of a check one lane cannot hold, in the words of library `lib`; `tail` ends its advice.
struct TooLarge {
    const char *lib, *tail;
    int operator()(long long n, int r) const {
        set_last_error(std::string(lib) + ": r = " + std::to_string(r) + ", n = " + std::to_string(n) +
                       " exceeds r <= " + std::to_string(kMaxMT) + ", n <= " + std::to_string(kInlineSrc) +
                       " (one lane holds all r syndromes); product codes stay with ecg_scrub_suspects" + tail);
        return ECG_EINVAL;
    }
};

// The check matrix of an ErasureCode handle, r x n: ECG_OK, the code's own error, or the refusal of too large a one.
inline int ec_check(ecg_ec* ec, const TooLarge& too_large, std::vector<int>& H, int& n, int& r) {
    r = ec->impl->check_matrix(H);
    if (r < 0) return r;
    if (r < 1) return ECG_EINVAL;
    n = (int)(H.size() / (size_t)r);
    return r > kMaxMT || n > kInlineSrc ? too_large(n, r) : ECG_OK;
}

// The table sets a candidate launch reads; the caller notes the launch on each (Engine::note_launch).
struct CandidateTables {
    std::shared_ptr<ProgramSet> chk, ratio;
};

// The LocateLaunch of a plan, up to the launch: flush the thread's batch scope, fetch the check's and the ratios'
// tables, fill `a` (`fill` sets its sources) and zero the S x (n + 2) counters; `zeroing` labels a failure of that.
template <class Fill>
int prepare_launch(const CandidatePlan& pl, long long B, int S, const int* d_stripe_ids, unsigned* d_counters,
                   const char* zeroing, hipStream_t st, Fill fill, LocateLaunch& a, CandidateTables& t) {
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;
    Engine& eng = Engine::instance();
    int status = ECG_OK;
    t.chk = eng.program_set(&pl.chk.op, 1, &status, st);
    if (!t.chk) return status;
    t.ratio = eng.program_set(&pl.ratio, 1, &status, st);
    if (!t.ratio) return status;
    if (const int rc = t.chk->ensure_ready(st); rc != ECG_OK) return rc;
    if (const int rc = t.ratio->ensure_ready(st); rc != ECG_OK) return rc;
    const ProgramSet &ps = *t.chk, &rs = *t.ratio;
    if (ps.MT != pl.r || ps.rtiles != 1 || rs.MT != pl.r || rs.rtiles != 1 || rs.k != pl.n) return ECG_EINVAL;
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
    if (const hipError_t e = hipMemsetAsync(d_counters, 0, (size_t)S * (size_t)(pl.n + 2) * sizeof(unsigned), st);
        e != hipSuccess)
        return hip_fail(e, zeroing);
    return ECG_OK;
}

}  // namespace ecg
