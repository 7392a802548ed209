// extern "C" entry points declared in include/ecg_locate.h (libecg_locate.so): the host side of corruption
// localisation.  A locate reads two table sets, both LinearOps kept by the engine's program cache
// (Engine::program_set: built once per distinct H, uploaded, retired only when no launch can still read them): the
// check itself, as the scrub builds it (check_common.hpp make_check), and the candidate ratios
// H[q][b] / H[p0(b)][b] as an r x n "product" whose tables the kernel reads by candidate (locate_kernels.hpp).
#include <string.h>

#include <string>
#include <vector>

#include "../../include/ecg_locate.h"
#include "candidate_plan.hpp"
#include "capi_handle.hpp"
#include "check_common.hpp"
#include "engine.hpp"
#include "gf256.hpp"
#include "locate_kernels.hpp"

using namespace ecg;

namespace {

using Plan = CandidatePlan;  // candidate_plan.hpp: make_plan, shared with heal.cpp

constexpr TooLarge too_large{"locate", ""};

// The launch descriptor with the votes zeroed (candidate_plan.hpp prepare_launch), then the launch.  `fill` sets the
// launch's sources.
template <class Fill>
int run_locate(const Plan& pl, int mode, long long B, int S, const int* d_stripe_ids, unsigned* d_votes, bool vec_ok,
               hipStream_t st, Fill fill) {
    LocateLaunch a;
    CandidateTables t;
    if (const int rc = prepare_launch(pl, {}, pl.n + 2, B, S, d_stripe_ids, d_votes, "hipMemsetAsync(locate votes)", st,
                                      fill, a, t);
        rc != ECG_OK)
        return rc;
    if (const hipError_t e = launch_locate(a, mode, vec_ok, st); e != hipSuccess) return hip_fail(e, "launch_locate");
    t.note_launch(st);
    return ECG_OK;
}

int run_strided_locate(const Plan& pl, const void* d_base, long long sstride, long long bstride, long long B,
                       const int* d_stripe_ids, int S, unsigned* d_votes, hipStream_t st) {
    const StridedSrc src{d_base, sstride, bstride};
    return run_locate(pl, GF_MODE_STRIDED, B, S, d_stripe_ids, d_votes, src.vec_ok(), st, src);
}

}  // namespace

extern "C" {

int ecg_locate_matrix_batch(int n, int r, const int* H, const int* src_ids, const void* d_base, long long sstride,
                            long long bstride, long long B, const int* d_stripe_ids, int S_sel, unsigned* d_votes,
                            void* stream) {
    if (n < 1 || r < 1 || bad_sizes(B, S_sel) || !H || !src_ids || !d_base || !d_votes) return ECG_EINVAL;
    if (const int rc = too_large(n, r); rc != ECG_OK) return rc;
    if (S_sel == 0 || B == 0) return ECG_OK;
    return run_strided_locate(make_plan(n, r, H, src_ids, true), d_base, sstride, bstride, B, d_stripe_ids, S_sel,
                              d_votes, (hipStream_t)stream);
}

int ecg_locate_encode_batch(int k, int m, const int* matrix, const void* d_stripes, long long sstride,
                            long long bstride, long long B, const int* d_stripe_ids, int S_sel, unsigned* d_votes,
                            void* stream) {
    if (k < 1 || m < 1 || bad_sizes(B, S_sel) || !matrix || !d_stripes || !d_votes) return ECG_EINVAL;
    if (const int rc = too_large((long long)k + m, m); rc != ECG_OK) return rc;
    if (S_sel == 0 || B == 0) return ECG_OK;
    const std::vector<int> H = encode_check(k, m, matrix), ids = iota(k + m);
    return run_strided_locate(make_plan(k + m, m, H.data(), ids.data(), true), d_stripes, sstride, bstride, B,
                              d_stripe_ids, S_sel, d_votes, (hipStream_t)stream);
}

int ecg_locate_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B,
                        const int* d_stripe_ids, int S_sel, unsigned* d_votes, void* stream) {
    if (!ec || bad_sizes(B, S_sel) || !d_stripes || !d_votes || ec->impl->mem != ECG_MEM_DEVICE) return ECG_EINVAL;
    std::vector<int> H;
    int n, r;
    if (const int rc = ec_check(ec, too_large, H, n, r); rc != ECG_OK) return rc;
    if (S_sel == 0 || B == 0) return ECG_OK;
    const std::vector<int> ids = iota(n);
    return run_strided_locate(make_plan(n, r, H.data(), ids.data(), true), d_stripes, sstride, bstride, B,
                              d_stripe_ids, S_sel, d_votes, (hipStream_t)stream);
}

int ecg_locate_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size, unsigned* d_votes) {
    if (!ec || block_size < 0 || !d_data_ptrs || !d_coding_ptrs || !d_votes || ec->impl->mem != ECG_MEM_DEVICE)
        return ECG_EINVAL;
    std::vector<int> H;
    int n, r;
    if (const int rc = ec_check(ec, too_large, H, n, r); rc != ECG_OK) return rc;
    const BlockPtrs src{ec->impl->k, n, d_data_ptrs, d_coding_ptrs};
    if (src.any_null()) return ECG_EINVAL;
    if (block_size == 0) return ECG_OK;
    const std::vector<int> ids = iota(n);
    return run_locate(make_plan(n, r, H.data(), ids.data(), false), GF_MODE_INLINE, block_size, 1, nullptr, d_votes,
                      src.vec_ok(), ec->impl->stream, src);
}

int ecg_locate_verdict(int n, const unsigned* h_votes, int* ids, int cap, int* n_ids) {
    if (n < 1 || !h_votes || cap < 0 || (cap > 0 && !ids)) return ECG_EINVAL;
    const unsigned bad = h_votes[n];
    int voted = 0, full = 0, who = -1;
    for (int b = 0; b < n; b++) {
        if (h_votes[b] == 0) continue;
        voted++;
        if (h_votes[b] == bad) {
            full++;
            if (who < 0) who = b;
        }
    }
    if (n_ids) *n_ids = voted;
    if (voted > 0 && voted <= cap) {
        int w = 0;
        for (int b = 0; b < n; b++)
            if (h_votes[b] != 0) ids[w++] = b;
    }
    if (bad == 0) return ECG_LOCATE_CLEAN;
    if (full > 1) return ECG_LOCATE_AMBIGUOUS;
    if (full == 1 && h_votes[n + 1] == 0) return who;
    return ECG_LOCATE_MULTIPLE;
}

int ecg_locate_counters(long long* launches, long long* bytes) {
    locate_traffic(launches, bytes);
    return ECG_OK;
}

int ecg_locate_last_launch(int* v, int cap) { return locate_last_launch(v, cap); }

}  // extern "C"
