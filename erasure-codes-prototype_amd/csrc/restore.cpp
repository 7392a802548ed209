// extern "C" entry points declared in include/ecg_restore.h (libecg_restore.so): the host side of named-block
// restoration.  A restore reads the check's tables as the locate builds them (candidate_plan.hpp make_plan; the
// engine's program cache keeps them) and a plan per stripe: the strided forms have the plan kernel write it into the
// caller's scratch on the stream, the per-stripe form solves on the host (solve_plan, over gf256.hpp) and passes the
// plan in the kernel arguments.
#include <string.h>

#include <string>
#include <vector>

#include "../../include/ecg_restore.h"
#include "candidate_plan.hpp"
#include "capi_handle.hpp"
#include "check_common.hpp"
#include "engine.hpp"
#include "gf256.hpp"
#include "restore_kernels.hpp"

using namespace ecg;

namespace {

constexpr TooLarge too_large{"restore", " and a decode"};

int refuse(const std::string& why) {
    set_last_error("restore: " + why);
    return ECG_EINVAL;
}

// The plan of one stripe from its flags, on the host: Gauss-Jordan on H[:, E] with row pivoting (the first row that was
// no pivot yet and is nonzero in the column), no row swaps, and the row transform beside it (restore_kernels.hpp).
void solve_plan(int n, int r, const int* H, const unsigned char* named, RestorePlan& pl) {
    memset(&pl, 0, sizeof(pl));
    int t = 0;
    for (int c = 0; c < kMaxMT; c++) pl.ids[c] = pl.rows[c] = -1;
    for (int j = 0; j < n; j++)
        if (named[j]) {
            if (t < kMaxMT) pl.ids[t] = j;
            t++;
        }
    pl.t = t;
    pl.state = t == 0 ? kRestoreNone : t > r ? kRestoreTooMany : kRestoreUsable;
    for (int i = 0; i < kMaxMT * kMaxMT; i++) make_coef_tab(0, &pl.A[i]);
    if (pl.state != kRestoreUsable) return;
    int a[kMaxMT][kMaxMT] = {}, T[kMaxMT][kMaxMT] = {};
    bool used[kMaxMT] = {};
    for (int q = 0; q < r; q++) {
        T[q][q] = 1;
        for (int c = 0; c < t; c++) a[q][c] = H[(size_t)q * n + pl.ids[c]] & 0xff;
    }
    for (int c = 0; c < t; c++) {
        int p = 0;
        while (p < r && (used[p] || a[p][c] == 0)) p++;
        if (p == r) {
            pl.state = kRestoreDependent;
            for (int i = 0; i < kMaxMT; i++) pl.rows[i] = -1;
            return;
        }
        used[p] = true;
        pl.rows[c] = p;
        const int iv = gf::inv(a[p][c]);
        for (int j = 0; j < kMaxMT; j++) {
            a[p][j] = gf::mul(a[p][j], iv);
            T[p][j] = gf::mul(T[p][j], iv);
        }
        for (int q = 0; q < r; q++) {
            const int f = a[q][c];
            if (q == p || f == 0) continue;
            for (int j = 0; j < kMaxMT; j++) {
                a[q][j] ^= gf::mul(a[p][j], f);
                T[q][j] ^= gf::mul(T[p][j], f);
            }
        }
    }
    int w = t;
    for (int q = 0; q < r; q++)
        if (!used[q]) pl.rows[w++] = q;
    for (int p = 0; p < r; p++)
        for (int i = 0; i < r; i++) make_coef_tab(T[pl.rows[i]][p], &pl.A[p * r + i]);
}

// The locate's launch descriptor with the n + 3 counters zeroed (candidate_plan.hpp prepare_launch), then the launch.
// `fill` sets the launch's sources and `plan` the descriptor's plan.
template <class Fill, class Plan>
int run_restore(const CandidatePlan& cp, int mode, long long B, int S, const int* d_stripe_ids, unsigned* d_report,
                bool vec_ok, hipStream_t st, Fill fill, Plan plan) {
    RestoreLaunch ra;
    CandidateTables t;
    if (const int rc = prepare_launch(cp, {}, cp.n + 3, B, S, d_stripe_ids, d_report, "hipMemsetAsync(restore report)",
                                      st, fill, ra.l, t);
        rc != ECG_OK)
        return rc;
    ra.plans = nullptr;
    ra.post_state = 0;
    if (const int rc = plan(ra); rc != ECG_OK) return rc;
    if (const hipError_t e = launch_restore(ra, mode, vec_ok, st); e != hipSuccess)
        return hip_fail(e, "launch_restore");
    t.note_launch(st);
    return ECG_OK;
}

// The strided forms after their own argument checks: the scratch, the no-op, the plan kernel and the launch.
int run_strided_restore(int n, int r, const int* H, const int* src_ids, void* d_base, long long sstride,
                        long long bstride, long long B, const int* d_stripe_ids, const unsigned char* d_named, int S,
                        void* d_work, unsigned* d_report, hipStream_t st) {
    if (!d_named) return refuse("d_named is NULL");
    if (S > 0 && !d_work) return refuse("d_work is NULL (ecg_restore_work_bytes(S_sel) bytes of device scratch)");
    if (((uintptr_t)d_work & 31u) != 0) return refuse("d_work is not 32-byte aligned");
    if (S == 0 || B == 0) return ECG_OK;
    const CandidatePlan cp = make_plan(n, r, H, src_ids, true);
    const StridedSrc src{d_base, sstride, bstride};
    const bool vec_ok = src.vec_ok();
    return run_restore(cp, GF_MODE_STRIDED, B, S, d_stripe_ids, d_report, vec_ok, st, src, [&](RestoreLaunch& ra) {
        RestorePlanLaunch p;
        memset(&p, 0, sizeof(p));
        p.named = d_named;
        p.plans = (RestorePlan*)d_work;
        p.n = n;
        p.r = r;
        p.S = S;
        for (int i = 0; i < r * n; i++) p.H[i] = (uint8_t)(H[i] & 0xff);
        if (const hipError_t e = launch_restore_plan(p, st); e != hipSuccess)
            return hip_fail(e, "launch_restore_plan");
        ra.plans = p.plans;
        return (int)ECG_OK;
    });
}

int bad_common(long long B, long long S, const void* d_base, const void* d_report) {
    if (B < 0 || S < 0)
        return refuse("negative size (B = " + std::to_string(B) + ", S_sel = " + std::to_string(S) + ")");
    if (B >= (1LL << 31)) return refuse("B = " + std::to_string(B) + " is not below 2^31");
    if (!d_base) return refuse("the stripes' base is NULL");
    if (!d_report) return refuse("d_report is NULL");
    return ECG_OK;
}

}  // namespace

extern "C" {

int ecg_restore_matrix_batch(int n, int r, const int* H, const int* src_ids, void* d_base, long long sstride,
                             long long bstride, long long B, const int* d_stripe_ids, const unsigned char* d_named,
                             int S_sel, void* d_work, unsigned* d_report, void* stream) {
    if (n < 1 || r < 1)
        return refuse("n = " + std::to_string(n) + ", r = " + std::to_string(r) + ": both must be >= 1");
    if (!H || !src_ids) return refuse(!H ? "H is NULL" : "src_ids is NULL");
    if (const int rc = bad_common(B, S_sel, d_base, d_report); rc != ECG_OK) return rc;
    if (const int rc = too_large(n, r); rc != ECG_OK) return rc;
    return run_strided_restore(n, r, H, src_ids, d_base, sstride, bstride, B, d_stripe_ids, d_named, S_sel, d_work,
                               d_report, (hipStream_t)stream);
}

int ecg_restore_encode_batch(int k, int m, const int* matrix, void* d_stripes, long long sstride, long long bstride,
                             long long B, const int* d_stripe_ids, const unsigned char* d_named, int S_sel,
                             void* d_work, unsigned* d_report, void* stream) {
    if (k < 1 || m < 1)
        return refuse("k = " + std::to_string(k) + ", m = " + std::to_string(m) + ": both must be >= 1");
    if (!matrix) return refuse("matrix is NULL");
    if (const int rc = bad_common(B, S_sel, d_stripes, d_report); rc != ECG_OK) return rc;
    if (const int rc = too_large((long long)k + m, m); rc != ECG_OK) return rc;
    const std::vector<int> H = encode_check(k, m, matrix), ids = iota(k + m);
    return run_strided_restore(k + m, m, H.data(), ids.data(), d_stripes, sstride, bstride, B, d_stripe_ids, d_named,
                               S_sel, d_work, d_report, (hipStream_t)stream);
}

int ecg_restore_ec_batch(ecg_ec* ec, void* d_stripes, long long sstride, long long bstride, long long B,
                         const int* d_stripe_ids, const unsigned char* d_named, int S_sel, void* d_work,
                         unsigned* d_report, void* stream) {
    if (!ec) return refuse("ec is NULL");
    if (const int rc = bad_common(B, S_sel, d_stripes, d_report); rc != ECG_OK) return rc;
    if (ec->impl->mem != ECG_MEM_DEVICE) return refuse("the handle is not an ECG_MEM_DEVICE handle");
    std::vector<int> H;
    int n, r;
    if (const int rc = ec_check(ec, too_large, H, n, r); rc != ECG_OK) return rc;
    const std::vector<int> ids = iota(n);
    return run_strided_restore(n, r, H.data(), ids.data(), d_stripes, sstride, bstride, B, d_stripe_ids, d_named, S_sel,
                               d_work, d_report, (hipStream_t)stream);
}

int ecg_restore_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size, const unsigned char* h_named,
                   unsigned* d_report) {
    if (!ec) return refuse("ec is NULL");
    if (block_size < 0) return refuse("negative size (block_size = " + std::to_string(block_size) + ")");
    if (!d_data_ptrs || !d_coding_ptrs) return refuse("a block pointer array is NULL");
    if (!h_named) return refuse("h_named is NULL");
    if (!d_report) return refuse("d_report is NULL");
    if (ec->impl->mem != ECG_MEM_DEVICE) return refuse("the handle is not an ECG_MEM_DEVICE handle");
    std::vector<int> H;
    int n, r;
    if (const int rc = ec_check(ec, too_large, H, n, r); rc != ECG_OK) return rc;
    const BlockPtrs src{ec->impl->k, n, d_data_ptrs, d_coding_ptrs};
    if (src.any_null()) return refuse("a block pointer is NULL");
    if (block_size == 0) return ECG_OK;
    const std::vector<int> ids = iota(n);
    const CandidatePlan cp = make_plan(n, r, H.data(), ids.data(), false);
    return run_restore(cp, GF_MODE_INLINE, block_size, 1, nullptr, d_report, src.vec_ok(), ec->impl->stream, src,
                       [&](RestoreLaunch& ra) {
                           solve_plan(n, r, H.data(), h_named, ra.inl);
                           return (int)ECG_OK;
                       });
}

long long ecg_restore_work_bytes(int S_sel) {
    if (S_sel < 0) return refuse("negative size (S_sel = " + std::to_string(S_sel) + ")");
    return (long long)S_sel * (long long)sizeof(RestorePlan);
}

int ecg_restore_names_from_sums(int n, int Q, const unsigned* d_sums, const unsigned* d_expected, int S_sel,
                                unsigned char* d_named, int* d_count, void* stream) {
    if (n < 1 || Q < 0 || S_sel < 0)
        return refuse("n = " + std::to_string(n) + ", Q = " + std::to_string(Q) + ", S_sel = " + std::to_string(S_sel) +
                      ": n must be >= 1, Q and S_sel >= 0");
    if (!d_sums || !d_expected) return refuse(!d_sums ? "d_sums is NULL" : "d_expected is NULL");
    if (!d_named || !d_count) return refuse(!d_named ? "d_named is NULL" : "d_count is NULL");
    if (Q == 0 || S_sel == 0) return ECG_OK;
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (const hipError_t e = launch_restore_names(n, Q, d_sums, d_expected, S_sel, d_named, d_count, st);
        e != hipSuccess)
        return hip_fail(e, "launch_restore_names");
    return ECG_OK;
}

int ecg_restore_counters(long long* launches, long long* bytes) {
    restore_traffic(launches, bytes);
    return ECG_OK;
}

int ecg_restore_last_launch(int* v, int cap) { return restore_last_launch(v, cap); }

}  // extern "C"
