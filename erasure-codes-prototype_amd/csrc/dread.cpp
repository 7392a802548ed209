// extern "C" entry points declared in include/ecg_dread.h (libecg_dread.so): the host side of the degraded range
// read.  A call checks its arguments, flushes the thread's batch scope, zeroes the report on the stream and hands H and
// src_ids to the two launches in their kernel arguments (dread_kernels.hpp): the plans are made on the device, from the
// device-resident lost flags, into the caller's scratch.  ecg_dread_plan is the same rule on the host, over gf256.hpp.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ecg_dread.h"
#include "capi_handle.hpp"
#include "check_common.hpp"
#include "dread_kernels.hpp"
#include "dread_records.hpp"
#include "engine.hpp"
#include "gf256.hpp"

using namespace ecg;

namespace {

int refuse(const std::string& why) {
    set_last_error("dread: " + why);
    return ECG_EINVAL;
}

std::string num(long long v) { return std::to_string(v); }

int too_large(long long n, int r) {
    if (r >= 1 && r <= kMaxMT && n >= 1 && n <= kInlineSrc) return ECG_OK;
    return refuse("r = " + num(r) + ", n = " + num(n) + " is outside 1 <= r <= " + num(kMaxMT) + ", 1 <= n <= " +
                  num(kInlineSrc) + " (the plan wave holds an r x r transform and two columns of H per lane); "
                  "ecg_ec_decode remains the path of such a code");
}

int bad_ids(int n, const int* src_ids) {
    std::vector<int> seen(src_ids, src_ids + n);
    std::sort(seen.begin(), seen.end());
    if (seen[0] < 0) return refuse("src_ids holds a negative id (" + num(seen[0]) + ")");
    for (int j = 1; j < n; j++)
        if (seen[j] == seen[j - 1]) return refuse("src_ids names block " + num(seen[j]) + " twice");
    return ECG_OK;
}

struct BatchArgs {
    const void* d_base;
    long long sstride, bstride, B;
    int S;
    const unsigned char* d_lost;
    const long long* d_records;
    int R;
    long long max_len;
    void* d_out;
    long long out_bytes;
    void* d_work;
    unsigned* d_report;
    hipStream_t st;
};

int bad_batch(const BatchArgs& b) {
    if (b.B < 0 || b.S < 0 || b.R < 0 || b.max_len < 0 || b.out_bytes < 0)
        return refuse("negative size (B = " + num(b.B) + ", S = " + num(b.S) + ", R = " + num(b.R) +
                      ", max_len = " + num(b.max_len) + ", out_bytes = " + num(b.out_bytes) + ")");
    if (b.B >= (1LL << 31)) return refuse("B = " + num(b.B) + " is not below 2^31");
    if (b.max_len > b.B) return refuse("max_len = " + num(b.max_len) + " exceeds B = " + num(b.B));
    if (!b.d_base) return refuse("the stripes' base is NULL");
    if (!b.d_lost) return refuse("d_lost is NULL");
    if (!b.d_records) return refuse("d_records is NULL");
    if (!b.d_out) return refuse("d_out is NULL");
    if (!b.d_report) return refuse("d_report is NULL");
    if (((uintptr_t)b.d_records & 7u) != 0) return refuse("d_records is not 8-byte aligned");
    if (b.R > 0 && !b.d_work) return refuse("d_work is NULL (ecg_dread_work_bytes(R, n) bytes of device scratch)");
    if (((uintptr_t)b.d_work & 31u) != 0) return refuse("d_work is not 32-byte aligned");
    int cpw, wpr;
    if (!dread_grid(b.max_len, b.R, cpw, wpr))
        return refuse("R = " + num(b.R) + " records of " + num(wpr) + " workgroups each need more than 2^31 - 1 "
                      "workgroups");
    return ECG_OK;
}

// After the shape checks of the entry point: the batch checks, the no-op, the flush, the zeroed report, the launches.
int run_batch(int n, int r, const int* H, const int* src_ids, const BatchArgs& b) {
    if (const int rc = bad_batch(b); rc != ECG_OK) return rc;
    if (b.R == 0) return ECG_OK;
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;
    if (const hipError_t e = hipMemsetAsync(b.d_report, 0, (size_t)b.R * 2 * sizeof(unsigned), b.st); e != hipSuccess)
        return hip_fail(e, "hipMemsetAsync(dread report)");
    DreadLaunch a;
    memset(&a, 0, sizeof(a));
    a.base = (const uint8_t*)b.d_base;
    a.sstride = b.sstride;
    a.bstride = b.bstride;
    a.lost = b.d_lost;
    a.records = b.d_records;
    a.out = (uint8_t*)b.d_out;
    a.work = (uint8_t*)b.d_work;
    a.report = b.d_report;
    a.B = b.B;
    a.max_len = b.max_len;
    a.out_bytes = b.out_bytes;
    a.S = b.S;
    a.n = n;
    a.r = r;
    a.R = b.R;
    int max_reads = 0;
    for (int j = 0; j < n; j++) {
        a.src_ids[j] = src_ids[j];
        bool any = false;
        for (int p = 0; p < r; p++) any |= (a.H[p * n + j] = (uint8_t)(H[(size_t)p * n + j] & 0xff)) != 0;
        max_reads += any ? 1 : 0;
    }
    const StridedSrc src{b.d_base, b.sstride, b.bstride};
    if (const hipError_t e = launch_dread(a, src.vec_ok(), max_reads, b.st); e != hipSuccess)
        return hip_fail(e, "launch_dread");
    return ECG_OK;
}

// The plan rule of include/ecg_dread.h, as the device runs it (dread_kernels.hip) but row by row over ints.
int host_plan(int n, int r, const int* H, const unsigned char* lost, int col, unsigned char* c_out, int* reads) {
    memset(c_out, 0, (size_t)n);
    *reads = 0;
    if (!lost[col]) {
        c_out[col] = 1;
        *reads = 1;
        return kDreadAnswered;
    }
    int nz[kMaxMT] = {}, T[kMaxMT][kMaxMT] = {};
    for (int q = 0; q < r; q++) {
        T[q][q] = 1;
        for (int j = 0; j < n; j++) nz[q] += !lost[j] && (H[(size_t)q * n + j] & 0xff) != 0;
    }
    bool used[kMaxMT] = {};
    int pcol = -1;
    for (int c = 0; c < n; c++) {
        if (!lost[c]) continue;
        int cur[kMaxMT] = {};  // T * H[:, c]
        for (int q = 0; q < r; q++)
            for (int p = 0; p < r; p++) cur[q] ^= gf::mul(T[q][p], H[(size_t)p * n + c] & 0xff);
        int best = -1;
        for (int q = 0; q < r; q++)
            if (!used[q] && cur[q] != 0 && (best < 0 || nz[q] < nz[best])) best = q;
        if (best < 0) continue;
        used[best] = true;
        if (c == col) pcol = best;
        const int iv = gf::inv(cur[best]);
        for (int p = 0; p < r; p++) T[best][p] = gf::mul(T[best][p], iv);
        for (int q = 0; q < r; q++)
            if (q != best && cur[q] != 0)
                for (int p = 0; p < r; p++) T[q][p] ^= gf::mul(T[best][p], cur[q]);
    }
    if (pcol < 0) return kDreadUnrecoverable;
    bool unit = true;
    for (int j = 0; j < n; j++) {
        int v = 0;
        for (int p = 0; p < r; p++) v ^= gf::mul(T[pcol][p], H[(size_t)p * n + j] & 0xff);
        if (lost[j]) unit &= v == (j == col ? 1 : 0);
        else c_out[j] = (unsigned char)v;
    }
    if (!unit) {
        memset(c_out, 0, (size_t)n);
        return kDreadUnrecoverable;
    }
    for (int j = 0; j < n; j++) *reads += c_out[j] != 0;
    return kDreadAnswered;
}

}  // namespace

extern "C" {

int ecg_dread_matrix_batch(int n, int r, const int* H, const int* src_ids, const void* d_base, long long sstride,
                           long long bstride, long long B, int S, const unsigned char* d_lost,
                           const long long* d_records, int R, long long max_len, void* d_out, long long out_bytes,
                           void* d_work, unsigned* d_report, void* stream) {
    if (const int rc = too_large(n, r); rc != ECG_OK) return rc;
    if (!H || !src_ids) return refuse(!H ? "H is NULL" : "src_ids is NULL");
    if (const int rc = bad_ids(n, src_ids); rc != ECG_OK) return rc;
    return run_batch(n, r, H, src_ids,
                     {d_base, sstride, bstride, B, S, d_lost, d_records, R, max_len, d_out, out_bytes, d_work,
                      d_report, (hipStream_t)stream});
}

int ecg_dread_encode_batch(int k, int m, const int* matrix, const void* d_stripes, long long sstride,
                           long long bstride, long long B, int S, const unsigned char* d_lost,
                           const long long* d_records, int R, long long max_len, void* d_out, long long out_bytes,
                           void* d_work, unsigned* d_report, void* stream) {
    if (k < 1 || m < 1) return refuse("k = " + num(k) + ", m = " + num(m) + ": both must be >= 1");
    if (const int rc = too_large((long long)k + m, m); rc != ECG_OK) return rc;
    if (!matrix) return refuse("matrix is NULL");
    const std::vector<int> H = encode_check(k, m, matrix), ids = iota(k + m);
    return run_batch(k + m, m, H.data(), ids.data(),
                     {d_stripes, sstride, bstride, B, S, d_lost, d_records, R, max_len, d_out, out_bytes, d_work,
                      d_report, (hipStream_t)stream});
}

int ecg_dread_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B, int S,
                       const unsigned char* d_lost, const long long* d_records, int R, long long max_len, void* d_out,
                       long long out_bytes, void* d_work, unsigned* d_report, void* stream) {
    if (!ec) return refuse("ec is NULL");
    if (ec->impl->mem != ECG_MEM_DEVICE) return refuse("the handle is not an ECG_MEM_DEVICE handle");
    std::vector<int> H;
    int n, r;
    if (const int rc = ec_check(ec, too_large, H, n, r); rc != ECG_OK) return rc;
    const std::vector<int> ids = iota(n);
    return run_batch(n, r, H.data(), ids.data(),
                     {d_stripes, sstride, bstride, B, S, d_lost, d_records, R, max_len, d_out, out_bytes, d_work,
                      d_report, (hipStream_t)stream});
}

long long ecg_dread_work_bytes(int R, int n) {
    if (R < 0 || n < 1 || n > kInlineSrc)
        return refuse("work_bytes: R = " + num(R) + ", n = " + num(n) + " (R >= 0, 1 <= n <= " + num(kInlineSrc) + ")");
    return (long long)R * dread_plan_bytes(n);
}

int ecg_dread_plan(int n, int r, const int* H, const unsigned char* h_lost, int col, unsigned char* c_out,
                   int* reads) {
    if (const int rc = too_large(n, r); rc != ECG_OK) return rc;
    if (!H || !h_lost || !c_out) return refuse(!H ? "H is NULL" : !h_lost ? "h_lost is NULL" : "c_out is NULL");
    if (col < 0 || col >= n) return refuse("col = " + num(col) + " is not in [0, " + num(n) + ")");
    int nreads = 0;
    const int state = host_plan(n, r, H, h_lost, col, c_out, &nreads);
    if (reads) *reads = nreads;
    return state;
}

int ecg_dread_check_records(const long long* h_records, int R, int n, long long B, int S, long long max_len,
                            long long out_bytes) {
    if (R < 0) return refuse("negative size (R = " + num(R) + ")");  // ECG_EINVAL is -2: no record index, not -1
    if (!h_records && R > 0) return refuse("h_records is NULL");
    std::string why;
    const int first = dread_check_records(h_records, R, n, B, S, max_len, out_bytes, why);
    if (first >= 0) set_last_error("dread: " + why);
    return first;
}

int ecg_dread_counters(long long* launches, long long* records) {
    dread_traffic(launches, records);
    return ECG_OK;
}

int ecg_dread_last_launch(int* v, int cap) { return dread_last_launch(v, cap); }

}  // extern "C"
