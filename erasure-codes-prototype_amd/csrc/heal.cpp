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

constexpr TooLarge too_large{"heal", " and a decode"};

// ANY mode corrects every block that explains a position: refused unless at most one can.
int check_any(const CandidatePlan& pl) {
    int a = 0, b = 0;
    if (columns_distinct(pl, a, b)) return ECG_OK;
    set_last_error("heal: columns " + std::to_string(a) + " and " + std::to_string(b) +
                   " of the check matrix are proportional (r = " + std::to_string(pl.r) +
                   "): ANY mode cannot tell their blocks apart; name the block with d_targets");
    return ECG_EINVAL;
}

// The locate's launch descriptor with the report zeroed (candidate_plan.hpp prepare_launch, which fetches the pivot
// inverses' tables with the others), the candidate set on top of it, then the launch.  `fill` sets the launch's sources.
template <class Fill>
int run_heal(const HealPlan& hp, int mode, long long B, int S, const int* d_stripe_ids, const int* d_targets,
             int target, bool any, unsigned* d_report, bool vec_ok, hipStream_t st, Fill fill) {
    HealLaunch h;
    CandidateTables t;
    if (const int rc = prepare_launch(hp.cand, {&hp.inv}, hp.cand.n + 2, B, S, d_stripe_ids, d_report,
                                      "hipMemsetAsync(heal report)", st, fill, h.l, t);
        rc != ECG_OK)
        return rc;
    h.invlead = t.extra(0).d_tabs;
    h.targets = d_targets;
    h.target = target;
    h.any = any ? 1 : 0;
    if (const hipError_t e = launch_heal(h, mode, vec_ok, st); e != hipSuccess) return hip_fail(e, "launch_heal");
    t.note_launch(st);
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
    const StridedSrc src{d_base, sstride, bstride};
    return run_heal(hp, GF_MODE_STRIDED, B, S, d_stripe_ids, d_targets, -1, d_targets == nullptr, d_report,
                    src.vec_ok(), st, src);
}

}  // namespace

extern "C" {

int ecg_heal_matrix_batch(int n, int r, const int* H, const int* src_ids, void* d_base, long long sstride,
                          long long bstride, long long B, const int* d_stripe_ids, const int* d_targets, int S_sel,
                          unsigned* d_report, void* stream) {
    if (n < 1 || r < 1 || bad_sizes(B, S_sel) || !H || !src_ids || !d_base || !d_report) return ECG_EINVAL;
    if (const int rc = too_large(n, r); rc != ECG_OK) return rc;
    return run_strided_heal(n, r, H, src_ids, d_base, sstride, bstride, B, d_stripe_ids, d_targets, S_sel, d_report,
                            (hipStream_t)stream);
}

int ecg_heal_encode_batch(int k, int m, const int* matrix, void* d_stripes, long long sstride, long long bstride,
                          long long B, const int* d_stripe_ids, const int* d_targets, int S_sel, unsigned* d_report,
                          void* stream) {
    if (k < 1 || m < 1 || bad_sizes(B, S_sel) || !matrix || !d_stripes || !d_report) return ECG_EINVAL;
    if (const int rc = too_large((long long)k + m, m); rc != ECG_OK) return rc;
    const std::vector<int> H = encode_check(k, m, matrix), ids = iota(k + m);
    return run_strided_heal(k + m, m, H.data(), ids.data(), d_stripes, sstride, bstride, B, d_stripe_ids, d_targets,
                            S_sel, d_report, (hipStream_t)stream);
}

int ecg_heal_ec_batch(ecg_ec* ec, void* d_stripes, long long sstride, long long bstride, long long B,
                      const int* d_stripe_ids, const int* d_targets, int S_sel, unsigned* d_report, void* stream) {
    if (!ec || bad_sizes(B, S_sel) || !d_stripes || !d_report || ec->impl->mem != ECG_MEM_DEVICE) return ECG_EINVAL;
    std::vector<int> H;
    int n, r;
    if (const int rc = ec_check(ec, too_large, H, n, r); rc != ECG_OK) return rc;
    const std::vector<int> ids = iota(n);
    return run_strided_heal(n, r, H.data(), ids.data(), d_stripes, sstride, bstride, B, d_stripe_ids, d_targets, S_sel,
                            d_report, (hipStream_t)stream);
}

int ecg_heal_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size, int target,
                unsigned* d_report) {
    if (!ec || block_size < 0 || !d_data_ptrs || !d_coding_ptrs || !d_report || ec->impl->mem != ECG_MEM_DEVICE)
        return ECG_EINVAL;
    std::vector<int> H;
    int n, r;
    if (const int rc = ec_check(ec, too_large, H, n, r); rc != ECG_OK) return rc;
    if (target < -1 || target >= n) return ECG_EINVAL;
    const BlockPtrs src{ec->impl->k, n, d_data_ptrs, d_coding_ptrs};
    if (src.any_null()) return ECG_EINVAL;
    const std::vector<int> ids = iota(n);
    const HealPlan hp = make_heal_plan(n, r, H.data(), ids.data(), false);
    if (target < 0)
        if (const int rc = check_any(hp.cand); rc != ECG_OK) return rc;
    if (block_size == 0) return ECG_OK;
    return run_heal(hp, GF_MODE_INLINE, block_size, 1, nullptr, nullptr, target, target < 0, d_report, src.vec_ok(),
                    ec->impl->stream, src);
}

int ecg_heal_counters(long long* launches, long long* bytes) {
    heal_traffic(launches, bytes);
    return ECG_OK;
}

int ecg_heal_last_launch(int* v, int cap) { return heal_last_launch(v, cap); }

}  // extern "C"
