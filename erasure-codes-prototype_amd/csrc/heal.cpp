// extern "C" entry points declared in include/ecg_heal.h (libecg_heal.so): the host side of in-place correction.
// A heal reads three table sets, all LinearOps kept by the engine's program cache (Engine::program_set): the check
// and the candidate ratios, as the locate builds them (candidate_plan.hpp make_plan), and the pivot inverses
// 1 / H[p0(b)][b] as a 1 x n "product" whose tables the kernel reads by candidate (heal_kernels.hpp).
#include <string.h>

#include <string>
#include <vector>

#include "../../include/ecg_heal.h"
#include "candidate_plan.hpp"
#include "capi_handle.hpp"
#include "check_common.hpp"
#include "engine.hpp"
#include "gf256.hpp"
#include "heal_kernels.hpp"

using namespace ecg;

namespace {

struct HealPlan {
    CandidatePlan cand;
    LinearOp inv;  // 1 x n: 1 / H[p0(b)][b]; 0 for a zero column of H
};

unsigned pivot_of(const CandidatePlan& pl, int b) { return (pl.p0[b >> 3] >> ((b & 7) * 4)) & 15u; }

HealPlan make_heal_plan(int n, int r, const int* H, const int* src_ids, bool consecutive) {
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

// Two nonzero columns of H are proportional exactly when they have the same pivot row and the same ratio column.
// Returns false, with a < b the first such pair, or true when every bad position has at most one explaining block.
bool columns_distinct(const CandidatePlan& pl, int& a_out, int& b_out) {
    const int n = pl.n, r = pl.r;
    for (int a = 0; a < n; a++) {
        if (pivot_of(pl, a) == kNoPivot) continue;
        for (int b = a + 1; b < n; b++) {
            if (pivot_of(pl, b) != pivot_of(pl, a)) continue;
            bool same = true;
            for (int q = 0; same && q < r; q++) same = pl.ratio.coef[(size_t)q * n + a] == pl.ratio.coef[(size_t)q * n + b];
            if (same) {
                a_out = a;
                b_out = b;
                return false;
            }
        }
    }
    return true;
}

int too_large(long long n, int r) {
    set_last_error("heal: r = " + std::to_string(r) + ", n = " + std::to_string(n) + " exceeds r <= " +
                   std::to_string(kMaxMT) + ", n <= " + std::to_string(kInlineSrc) +
                   " (one lane holds all r syndromes); product codes stay with ecg_scrub_suspects and a decode");
    return ECG_EINVAL;
}

// ANY mode corrects every block that explains a position: refused unless at most one can.
int check_any(const CandidatePlan& pl) {
    int a = 0, b = 0;
    if (columns_distinct(pl, a, b)) return ECG_OK;
    set_last_error("heal: columns " + std::to_string(a) + " and " + std::to_string(b) +
                   " of the check matrix are proportional (r = " + std::to_string(pl.r) +
                   "): ANY mode cannot tell their blocks apart; name the block with d_targets");
    return ECG_EINVAL;
}

// Flush the thread's batch scope, fetch the table sets, zero the report, launch.  `fill` sets the launch's sources.
template <class Fill>
int run_heal(const HealPlan& hp, int mode, long long B, int S, const int* d_stripe_ids, const int* d_targets,
             int target, bool any, unsigned* d_report, bool vec_ok, hipStream_t st, Fill fill) {
    const CandidatePlan& pl = hp.cand;
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;
    Engine& eng = Engine::instance();
    int status = ECG_OK;
    std::shared_ptr<ProgramSet> ps = eng.program_set(&pl.chk.op, 1, &status, st);
    if (!ps) return status;
    std::shared_ptr<ProgramSet> rs = eng.program_set(&pl.ratio, 1, &status, st);
    if (!rs) return status;
    std::shared_ptr<ProgramSet> is = eng.program_set(&hp.inv, 1, &status, st);
    if (!is) return status;
    if (const int rc = ps->ensure_ready(st); rc != ECG_OK) return rc;
    if (const int rc = rs->ensure_ready(st); rc != ECG_OK) return rc;
    if (const int rc = is->ensure_ready(st); rc != ECG_OK) return rc;
    if (ps->MT != pl.r || ps->rtiles != 1 || rs->MT != pl.r || rs->rtiles != 1 || rs->k != pl.n || is->MT != 1 ||
        is->rtiles != 1 || is->k != pl.n)
        return ECG_EINVAL;
    HealLaunch h;
    memset(&h, 0, sizeof(h));
    LocateLaunch& a = h.l;
    a.g.tabs = ps->d_tabs;
    a.g.src_ids = ps->d_src;
    a.g.dst_ids = ps->d_dst;
    a.g.stripe_of = d_stripe_ids;
    a.g.B = B;
    a.g.k = ps->k;
    a.g.m = ps->m;
    a.g.S = S;
    a.g.MT = ps->MT;
    a.g.rtiles = ps->rtiles;
    a.g.binary = 0;  // the GENERAL flavour always: the tables of 0 and 1 are exact
    a.votes = d_report;
    a.ident = pl.chk.ident;
    a.ident_base = pl.chk.ident_base;
    a.ratios = rs->d_tabs;
    a.n = pl.n;
    memcpy(a.p0, pl.p0, sizeof(a.p0));
    h.invlead = is->d_tabs;
    h.targets = d_targets;
    h.target = target;
    h.any = any ? 1 : 0;
    fill(a.g);
    if (const hipError_t e = hipMemsetAsync(d_report, 0, (size_t)S * (size_t)(pl.n + 2) * sizeof(unsigned), st);
        e != hipSuccess)
        return hip_fail(e, "hipMemsetAsync(heal report)");
    if (const hipError_t e = launch_heal(h, mode, vec_ok, st); e != hipSuccess) return hip_fail(e, "launch_heal");
    eng.note_launch(*ps, st);
    eng.note_launch(*rs, st);
    eng.note_launch(*is, st);
    return ECG_OK;
}

// The strided forms after their own argument checks: the ANY refusal, the no-op, the launch.
int run_strided_heal(int n, int r, const int* H, const int* src_ids, void* d_base, long long sstride,
                     long long bstride, long long B, const int* d_stripe_ids, const int* d_targets, int S,
                     unsigned* d_report, hipStream_t st) {
    const HealPlan hp = make_heal_plan(n, r, H, src_ids, true);
    if (!d_targets)
        if (const int rc = check_any(hp.cand); rc != ECG_OK) return rc;
    if (S == 0 || B == 0) return ECG_OK;
    const bool vec_ok = aligned16(d_base) && sstride % 16 == 0 && bstride % 16 == 0;
    return run_heal(hp, GF_MODE_STRIDED, B, S, d_stripe_ids, d_targets, -1, d_targets == nullptr, d_report, vec_ok, st,
                    [&](GfLaunch& g) {
                        g.in_base = (const uint8_t*)d_base;
                        g.in_sstride = sstride;
                        g.in_bstride = bstride;
                    });
}

}  // namespace

extern "C" {

int ecg_heal_matrix_batch(int n, int r, const int* H, const int* src_ids, void* d_base, long long sstride,
                          long long bstride, long long B, const int* d_stripe_ids, const int* d_targets, int S_sel,
                          unsigned* d_report, void* stream) {
    if (n < 1 || r < 1 || bad_sizes(B, S_sel) || !H || !src_ids || !d_base || !d_report) return ECG_EINVAL;
    if (r > kMaxMT || n > kInlineSrc) return too_large(n, r);
    return run_strided_heal(n, r, H, src_ids, d_base, sstride, bstride, B, d_stripe_ids, d_targets, S_sel, d_report,
                            (hipStream_t)stream);
}

int ecg_heal_encode_batch(int k, int m, const int* matrix, void* d_stripes, long long sstride, long long bstride,
                          long long B, const int* d_stripe_ids, const int* d_targets, int S_sel, unsigned* d_report,
                          void* stream) {
    if (k < 1 || m < 1 || bad_sizes(B, S_sel) || !matrix || !d_stripes || !d_report) return ECG_EINVAL;
    if (m > kMaxMT || k > kInlineSrc - m) return too_large((long long)k + m, m);
    const std::vector<int> H = encode_check(k, m, matrix), ids = iota(k + m);
    return run_strided_heal(k + m, m, H.data(), ids.data(), d_stripes, sstride, bstride, B, d_stripe_ids, d_targets,
                            S_sel, d_report, (hipStream_t)stream);
}

int ecg_heal_ec_batch(ecg_ec* ec, void* d_stripes, long long sstride, long long bstride, long long B,
                      const int* d_stripe_ids, const int* d_targets, int S_sel, unsigned* d_report, void* stream) {
    if (!ec || bad_sizes(B, S_sel) || !d_stripes || !d_report || ec->impl->mem != ECG_MEM_DEVICE) return ECG_EINVAL;
    std::vector<int> H;
    const int r = ec->impl->check_matrix(H);
    if (r < 0) return r;
    if (r < 1) return ECG_EINVAL;
    const int n = (int)(H.size() / (size_t)r);
    if (r > kMaxMT || n > kInlineSrc) return too_large(n, r);
    const std::vector<int> ids = iota(n);
    return run_strided_heal(n, r, H.data(), ids.data(), d_stripes, sstride, bstride, B, d_stripe_ids, d_targets, S_sel,
                            d_report, (hipStream_t)stream);
}

int ecg_heal_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size, int target,
                unsigned* d_report) {
    if (!ec || block_size < 0 || !d_data_ptrs || !d_coding_ptrs || !d_report || ec->impl->mem != ECG_MEM_DEVICE)
        return ECG_EINVAL;
    std::vector<int> H;
    const int r = ec->impl->check_matrix(H);
    if (r < 0) return r;
    if (r < 1) return ECG_EINVAL;
    const int k = ec->impl->k, n = (int)(H.size() / (size_t)r);
    if (r > kMaxMT || n > kInlineSrc) return too_large(n, r);
    if (target < -1 || target >= n) return ECG_EINVAL;
    for (int b = 0; b < n; b++)
        if (!(b < k ? d_data_ptrs[b] : d_coding_ptrs[b - k])) return ECG_EINVAL;
    const std::vector<int> ids = iota(n);
    const HealPlan hp = make_heal_plan(n, r, H.data(), ids.data(), false);
    if (target < 0)
        if (const int rc = check_any(hp.cand); rc != ECG_OK) return rc;
    if (block_size == 0) return ECG_OK;
    bool vec_ok = true;
    for (int b = 0; b < n; b++) vec_ok &= aligned16(b < k ? d_data_ptrs[b] : d_coding_ptrs[b - k]);
    return run_heal(hp, GF_MODE_INLINE, block_size, 1, nullptr, nullptr, target, target < 0, d_report, vec_ok,
                    ec->impl->stream, [&](GfLaunch& g) {
                        for (int b = 0; b < n; b++)
                            g.isrc[b] = (const uint8_t*)(b < k ? d_data_ptrs[b] : d_coding_ptrs[b - k]);
                    });
}

int ecg_heal_counters(long long* launches, long long* bytes) {
    heal_traffic(launches, bytes);
    return ECG_OK;
}

int ecg_heal_last_launch(int* v, int cap) { return heal_last_launch(v, cap); }

}  // extern "C"
