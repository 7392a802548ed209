// extern "C" entry points declared in include/ecg_vread.h (libecg_vread.so): the host side of the verified range read.
// A call checks its arguments, flushes the thread's batch scope, zeroes the sums and the report on the stream and hands
// H and src_ids to the launches in their kernel arguments (vread_kernels.hpp): plans, sums and verdicts are made on the
// device.  The checks are dread.cpp's plus those of the piece size and the two tables.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/ecg_vread.h"
#include "capi_handle.hpp"
#include "check_common.hpp"
#include "dread_records.hpp"
#include "engine.hpp"
#include "vread_kernels.hpp"

using namespace ecg;

namespace {

std::atomic<long long> g_span_bytes{0};  // ecg_vread_set_span_bytes; 0 = auto

int refuse(const std::string& why) {
    set_last_error("vread: " + why);
    return ECG_EINVAL;
}

std::string num(long long v) { return std::to_string(v); }

int too_large(long long n, int r) {
    if (r >= 1 && r <= kMaxMT && n >= 1 && n <= kInlineSrc) return ECG_OK;
    return refuse("r = " + num(r) + ", n = " + num(n) + " is outside 1 <= r <= " + num(kMaxMT) + ", 1 <= n <= " +
                  num(kInlineSrc) + " (the plan wave holds an r x r transform and two columns of H per lane)");
}

int bad_ids(int n, const int* src_ids) {
    std::vector<int> seen(src_ids, src_ids + n);
    std::sort(seen.begin(), seen.end());
    if (seen[0] < 0) return refuse("src_ids holds a negative id (" + num(seen[0]) + ")");
    for (int j = 1; j < n; j++)
        if (seen[j] == seen[j - 1]) return refuse("src_ids names block " + num(seen[j]) + " twice");
    return ECG_OK;
}

int bad_piece(long long piece_bytes) {
    if (piece_bytes == 0) return ECG_OK;
    if (piece_bytes >= kPsumMinPiece && piece_bytes <= kPsumMaxPiece && (piece_bytes & (piece_bytes - 1)) == 0)
        return ECG_OK;
    return refuse("piece_bytes = " + num(piece_bytes) + " is neither 0 (block sums) nor a power of two in [" +
                  num(kPsumMinPiece) + ", 2^30]");
}

struct BatchArgs {
    const void* d_base;
    long long sstride, bstride, B;
    int S;
    const unsigned char* d_lost;
    long long piece_bytes;
    const unsigned* d_expected;
    const long long* d_records;
    int R;
    long long max_len;
    void* d_out;
    long long out_bytes;
    void* d_work;
    unsigned* d_sums;
    unsigned* d_report;
    hipStream_t st;
};

int bad_batch(const BatchArgs& b, long long& NP) {
    if (b.B < 0 || b.S < 0 || b.R < 0 || b.max_len < 0 || b.out_bytes < 0)
        return refuse("negative size (B = " + num(b.B) + ", S = " + num(b.S) + ", R = " + num(b.R) +
                      ", max_len = " + num(b.max_len) + ", out_bytes = " + num(b.out_bytes) + ")");
    if (b.B >= (1LL << 31)) return refuse("B = " + num(b.B) + " is not below 2^31");
    if (b.max_len > b.B) return refuse("max_len = " + num(b.max_len) + " exceeds B = " + num(b.B));
    if (const int rc = bad_piece(b.piece_bytes); rc != ECG_OK) return rc;
    if (!b.d_base) return refuse("the stripes' base is NULL");
    if (!b.d_expected) return refuse("d_expected is NULL");
    if (!b.d_records) return refuse("d_records is NULL");
    if (!b.d_out) return refuse("d_out is NULL");
    if (!b.d_sums) return refuse("d_sums is NULL");
    if (!b.d_report) return refuse("d_report is NULL");
    if (((uintptr_t)b.d_records & 7u) != 0) return refuse("d_records is not 8-byte aligned");
    if (b.R > 0 && !b.d_work) return refuse("d_work is NULL (ecg_vread_work_bytes(R, n) bytes of device scratch)");
    if (((uintptr_t)b.d_work & 31u) != 0) return refuse("d_work is not 32-byte aligned");
    if ((((uintptr_t)b.d_expected | (uintptr_t)b.d_sums | (uintptr_t)b.d_report) & 3u) != 0)
        return refuse("d_expected, d_sums or d_report is not 4-byte aligned");
    long long span;
    int wpr;
    const bool fits = vread_grid(b.max_len, vread_piece(b.piece_bytes, b.B), b.B, b.R,
                                 g_span_bytes.load(std::memory_order_relaxed), NP, span, wpr);
    if ((long long)b.R * NP >= (1LL << 31))
        return refuse("R = " + num(b.R) + " records of " + num(NP) + " sums each: R * NP is not below 2^31");
    if (!fits)
        return refuse("R = " + num(b.R) + " records of " + num(wpr) + " workgroups each need more than 2^31 - 1 "
                      "workgroups");
    return ECG_OK;
}

// After the shape checks of the entry point: the batch checks, the no-op, the flush, the zeroed tables, the launches.
int run_batch(int n, int r, const int* H, const int* src_ids, const BatchArgs& b) {
    long long NP = 0;
    if (const int rc = bad_batch(b, NP); rc != ECG_OK) return rc;
    if (b.R == 0) return ECG_OK;
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;
    if (const hipError_t e =
            hipMemsetAsync(b.d_report, 0, (size_t)b.R * kVreadReportWords * sizeof(unsigned), b.st);
        e != hipSuccess)
        return hip_fail(e, "hipMemsetAsync(vread report)");
    if (NP > 0)
        if (const hipError_t e = hipMemsetAsync(b.d_sums, 0, (size_t)b.R * (size_t)NP * sizeof(unsigned), b.st);
            e != hipSuccess)
            return hip_fail(e, "hipMemsetAsync(vread sums)");
    VreadLaunch a;
    memset(&a, 0, sizeof(a));
    a.d.base = (const uint8_t*)b.d_base;
    a.d.sstride = b.sstride;
    a.d.bstride = b.bstride;
    a.d.lost = b.d_lost;
    a.d.records = b.d_records;
    a.d.out = (uint8_t*)b.d_out;
    a.d.work = (uint8_t*)b.d_work;
    a.d.report = b.d_report;
    a.d.B = b.B;
    a.d.max_len = b.max_len;
    a.d.out_bytes = b.out_bytes;
    a.d.S = b.S;
    a.d.n = n;
    a.d.r = r;
    a.d.R = b.R;
    a.expected = b.d_expected;
    a.sums = b.d_sums;
    a.P = vread_piece(b.piece_bytes, b.B);
    for (int j = 0; j < n; j++) {
        a.d.src_ids[j] = src_ids[j];
        for (int p = 0; p < r; p++) a.d.H[p * n + j] = (uint8_t)(H[(size_t)p * n + j] & 0xff);
    }
    const StridedSrc src{b.d_base, b.sstride, b.bstride};
    if (const hipError_t e = launch_vread(a, src.vec_ok(), g_span_bytes.load(std::memory_order_relaxed), b.st);
        e != hipSuccess)
        return hip_fail(e, "launch_vread");
    return ECG_OK;
}

}  // namespace

extern "C" {

int ecg_vread_matrix_batch(int n, int r, const int* H, const int* src_ids, const void* d_base, long long sstride,
                           long long bstride, long long B, int S, const unsigned char* d_lost, long long piece_bytes,
                           const unsigned* d_expected, const long long* d_records, int R, long long max_len,
                           void* d_out, long long out_bytes, void* d_work, unsigned* d_sums, unsigned* d_report,
                           void* stream) {
    if (const int rc = too_large(n, r); rc != ECG_OK) return rc;
    if (!H || !src_ids) return refuse(!H ? "H is NULL" : "src_ids is NULL");
    if (const int rc = bad_ids(n, src_ids); rc != ECG_OK) return rc;
    return run_batch(n, r, H, src_ids,
                     {d_base, sstride, bstride, B, S, d_lost, piece_bytes, d_expected, d_records, R, max_len, d_out,
                      out_bytes, d_work, d_sums, d_report, (hipStream_t)stream});
}

int ecg_vread_encode_batch(int k, int m, const int* matrix, const void* d_stripes, long long sstride,
                           long long bstride, long long B, int S, const unsigned char* d_lost, long long piece_bytes,
                           const unsigned* d_expected, const long long* d_records, int R, long long max_len,
                           void* d_out, long long out_bytes, void* d_work, unsigned* d_sums, unsigned* d_report,
                           void* stream) {
    if (k < 1 || m < 1) return refuse("k = " + num(k) + ", m = " + num(m) + ": both must be >= 1");
    if (const int rc = too_large((long long)k + m, m); rc != ECG_OK) return rc;
    if (!matrix) return refuse("matrix is NULL");
    const std::vector<int> H = encode_check(k, m, matrix), ids = iota(k + m);
    return run_batch(k + m, m, H.data(), ids.data(),
                     {d_stripes, sstride, bstride, B, S, d_lost, piece_bytes, d_expected, d_records, R, max_len, d_out,
                      out_bytes, d_work, d_sums, d_report, (hipStream_t)stream});
}

int ecg_vread_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B, int S,
                       const unsigned char* d_lost, long long piece_bytes, const unsigned* d_expected,
                       const long long* d_records, int R, long long max_len, void* d_out, long long out_bytes,
                       void* d_work, unsigned* d_sums, unsigned* d_report, void* stream) {
    if (!ec) return refuse("ec is NULL");
    if (ec->impl->mem != ECG_MEM_DEVICE) return refuse("the handle is not an ECG_MEM_DEVICE handle");
    std::vector<int> H;
    int n, r;
    if (const int rc = ec_check(ec, too_large, H, n, r); rc != ECG_OK) return rc;
    const std::vector<int> ids = iota(n);
    return run_batch(n, r, H.data(), ids.data(),
                     {d_stripes, sstride, bstride, B, S, d_lost, piece_bytes, d_expected, d_records, R, max_len, d_out,
                      out_bytes, d_work, d_sums, d_report, (hipStream_t)stream});
}

long long ecg_vread_work_bytes(int R, int n) {
    if (R < 0 || n < 1 || n > kInlineSrc)
        return refuse("work_bytes: R = " + num(R) + ", n = " + num(n) + " (R >= 0, 1 <= n <= " + num(kInlineSrc) + ")");
    return (long long)R * dread_plan_bytes(n);
}

int ecg_vread_cover(long long off, long long len, long long piece_bytes, long long B, long long* q0,
                    long long* npieces, long long* cover_bytes) {
    if (const int rc = bad_piece(piece_bytes); rc != ECG_OK) return rc;
    if (B < 0 || B >= (1LL << 31) || off < 0 || len < 0 || off > B || len > B - off)
        return refuse("cover: off = " + num(off) + ", len = " + num(len) + " is not a range of a block of B = " +
                      num(B) + " bytes (B < 2^31)");
    long long first = 0, count = 0, bytes = 0;
    if (len > 0) {
        const long long P = vread_piece(piece_bytes, B);
        first = off / P;
        const long long last = (off + len - 1) / P;
        count = last - first + 1;
        bytes = std::min((last + 1) * P, B) - first * P;
    }
    if (q0) *q0 = first;
    if (npieces) *npieces = count;
    if (cover_bytes) *cover_bytes = bytes;
    return ECG_OK;
}

long long ecg_vread_max_pieces(long long max_len, long long piece_bytes, long long B) {
    if (const int rc = bad_piece(piece_bytes); rc != ECG_OK) return rc;
    if (B < 0 || B >= (1LL << 31) || max_len < 0 || max_len > B)
        return refuse("max_pieces: max_len = " + num(max_len) + ", B = " + num(B) + " (0 <= max_len <= B < 2^31)");
    return vread_max_pieces(max_len, vread_piece(piece_bytes, B), B);
}

int ecg_vread_check_records(const long long* h_records, int R, int n, long long B, int S, long long max_len,
                            long long out_bytes) {
    if (R < 0) return refuse("negative size (R = " + num(R) + ")");  // ECG_EINVAL is -2: no record index, not -1
    if (!h_records && R > 0) return refuse("h_records is NULL");
    std::string why;
    const int first = dread_check_records(h_records, R, n, B, S, max_len, out_bytes, why);
    if (first >= 0) set_last_error("vread: " + why);
    return first;
}

int ecg_vread_set_span_bytes(long long bytes) {
    if (bytes < 0 || bytes % kPsumRowBytes != 0)
        return refuse("span_bytes = " + num(bytes) + " is neither 0 (auto) nor a positive multiple of " +
                      num(kPsumRowBytes));
    g_span_bytes.store(bytes, std::memory_order_relaxed);
    return ECG_OK;
}

int ecg_vread_counters(long long* launches, long long* records) {
    vread_traffic(launches, records);
    return ECG_OK;
}

int ecg_vread_last_launch(int* v, int cap) { return vread_last_launch(v, cap); }

}  // extern "C"
