// extern "C" entry points declared in include/ecg_update.h (libecg_update.so): the host side of the delta update.
// A call turns its coefficient matrix into one plan per column (update_kernels.hpp) -- k_in single-source programs of
// one program set, so the engine's program cache builds, uploads and keeps the tables --, zeroes the report on the
// stream and launches once.
#include <string.h>

#include <algorithm>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ecg_update.h"
#include "capi_handle.hpp"
#include "check_common.hpp"
#include "engine.hpp"
#include "update_kernels.hpp"

using namespace ecg;

namespace {

int refuse(const std::string& why) {
    set_last_error("update: " + why);
    return ECG_EINVAL;
}

std::string num(long long v) { return std::to_string(v); }

// The plans of G's columns as the programs of one set; ECG_EINVAL for a column with more than 8 nonzero coefficients.
struct ColumnPlans {
    std::vector<LinearOp> progs;  // [k_in]: one source, mt rows
    int max_nnz = 0, mt = 1;
};

int make_plans(int k_in, int m_out, const int* coef, const int* src_ids, const int* dst_ids, ColumnPlans& out) {
    out.max_nnz = 0;
    for (int j = 0; j < k_in; j++) {
        int nnz = 0;
        for (int i = 0; i < m_out; i++) nnz += (coef[(size_t)i * k_in + j] & 0xff) != 0;
        if (nnz > kUpdateMaxNnz)
            return refuse("column " + num(j) + " has " + num(nnz) + " nonzero coefficients, more than " +
                          num(kUpdateMaxNnz) + " (one lane holds the parity columns of a record)");
        out.max_nnz = std::max(out.max_nnz, nnz);
    }
    out.mt = std::max(out.max_nnz, 1);
    out.progs.assign((size_t)k_in, LinearOp());
    for (int j = 0; j < k_in; j++) {
        LinearOp& op = out.progs[j];
        op.src_ids.assign(1, src_ids[j]);
        op.dst_ids.assign((size_t)out.mt, -1);
        op.coef.assign((size_t)out.mt, 0);
        int p = 0;
        for (int i = 0; i < m_out; i++)
            if (const int c = coef[(size_t)i * k_in + j] & 0xff; c != 0) {
                op.dst_ids[p] = dst_ids[i];
                op.coef[p++] = (uint8_t)c;
            }
    }
    return ECG_OK;
}

int bad_shape(int k_in, int m_out, const int* coef, const int* src_ids, const int* dst_ids) {
    if (k_in < 1 || m_out < 1)
        return refuse("k_in = " + num(k_in) + ", m_out = " + num(m_out) + ": both must be >= 1");
    if ((long long)k_in + m_out > kInlineSrc)
        return refuse("k_in + m_out = " + num((long long)k_in + m_out) + " exceeds " + num(kInlineSrc));
    if (!coef) return refuse("coef is NULL");
    if (!src_ids || !dst_ids) return refuse(!src_ids ? "src_ids is NULL" : "dst_ids is NULL");
    std::vector<int> seen;
    for (int j = 0; j < k_in; j++) seen.push_back(src_ids[j]);
    std::sort(seen.begin(), seen.end());
    if (seen[0] < 0) return refuse("src_ids holds a negative id (" + num(seen[0]) + ")");
    for (int j = 1; j < k_in; j++)
        if (seen[j] == seen[j - 1]) return refuse("src_ids names block " + num(seen[j]) + " twice");
    std::vector<int> d(dst_ids, dst_ids + m_out);
    std::sort(d.begin(), d.end());
    if (d[0] < 0) return refuse("dst_ids holds a negative id (" + num(d[0]) + ")");
    for (int i = 1; i < m_out; i++)
        if (d[i] == d[i - 1]) return refuse("dst_ids names block " + num(d[i]) + " twice");
    for (int i = 0; i < m_out; i++)
        if (std::binary_search(seen.begin(), seen.end(), d[i]))
            return refuse("block " + num(d[i]) + " is both a source and a destination");
    return ECG_OK;
}

struct BatchArgs {
    void* d_base;
    long long sstride, bstride, B;
    int S, mode;
    const long long* d_records;
    int R;
    long long max_len;
    const void* d_in;
    long long in_bytes;
    void* d_delta_out;
    unsigned* d_report;
    hipStream_t st;
};

int bad_mode(int mode, const void* d_delta_out) {
    if (mode != ECG_UPDATE_WRITE && mode != ECG_UPDATE_DELTA)
        return refuse("mode = " + num(mode) + " is neither ECG_UPDATE_WRITE (0) nor ECG_UPDATE_DELTA (1)");
    if (mode == ECG_UPDATE_DELTA && d_delta_out)
        return refuse("d_delta_out is given in ECG_UPDATE_DELTA mode (the input is the delta)");
    return ECG_OK;
}

int bad_batch(const BatchArgs& b) {
    if (b.B < 0 || b.S < 0 || b.R < 0 || b.max_len < 0 || b.in_bytes < 0)
        return refuse("negative size (B = " + num(b.B) + ", S = " + num(b.S) + ", R = " + num(b.R) +
                      ", max_len = " + num(b.max_len) + ", in_bytes = " + num(b.in_bytes) + ")");
    if (b.B >= (1LL << 31)) return refuse("B = " + num(b.B) + " is not below 2^31");
    if (b.max_len > b.B) return refuse("max_len = " + num(b.max_len) + " exceeds B = " + num(b.B));
    if (!b.d_base) return refuse("the stripes' base is NULL");
    if (!b.d_records) return refuse("d_records is NULL");
    if (!b.d_in) return refuse("d_in is NULL");
    if (!b.d_report) return refuse("d_report is NULL");
    if (((uintptr_t)b.d_records & 7u) != 0) return refuse("d_records is not 8-byte aligned");
    if (const int rc = bad_mode(b.mode, b.d_delta_out); rc != ECG_OK) return rc;
    int cpw, wpr;
    if (!update_grid(b.max_len, b.R, cpw, wpr))
        return refuse("R = " + num(b.R) + " records of " + num(wpr) + " workgroups each need more than 2^31 - 1 "
                      "workgroups");
    return ECG_OK;
}

// After every argument check: flush, tables, the zeroed report, the launch.  `fill` completes the descriptor.
template <class Fill>
int run_update(const ColumnPlans& cp, int k_in, int R, unsigned* d_report, bool vec_ok, hipStream_t st, Fill fill) {
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;
    int status = ECG_OK;
    const std::shared_ptr<ProgramSet> ps = Engine::instance().program_set(cp.progs, &status, st);
    if (!ps) return status;
    if (const int rc = ps->ensure_ready(st); rc != ECG_OK) return rc;
    if (ps->nprog != k_in || ps->k != 1 || ps->MT != cp.mt || ps->rtiles != 1) return ECG_EINVAL;
    if (const hipError_t e = hipMemsetAsync(d_report, 0, (size_t)R * 2 * sizeof(unsigned), st); e != hipSuccess)
        return hip_fail(e, "hipMemsetAsync(update report)");
    UpdateLaunch a;
    memset(&a, 0, sizeof(a));
    a.tabs = ps->d_tabs;
    a.src_ids = ps->d_src;
    a.dst_ids = ps->d_dst;
    a.report = d_report;
    a.k_in = k_in;
    a.mt = cp.mt;
    a.R = R;
    fill(a);
    if (const hipError_t e = launch_update(a, vec_ok, cp.max_nnz, st); e != hipSuccess)
        return hip_fail(e, "launch_update");
    Engine::instance().note_launch(*ps, st);
    return ECG_OK;
}

int run_batch(int k_in, int m_out, const int* coef, const int* src_ids, const int* dst_ids, const BatchArgs& b) {
    if (const int rc = bad_batch(b); rc != ECG_OK) return rc;
    ColumnPlans cp;
    if (const int rc = make_plans(k_in, m_out, coef, src_ids, dst_ids, cp); rc != ECG_OK) return rc;
    if (b.R == 0) return ECG_OK;
    const StridedSrc src{b.d_base, b.sstride, b.bstride};
    return run_update(cp, k_in, b.R, b.d_report, src.vec_ok(), b.st, [&](UpdateLaunch& a) {
        a.base = (uint8_t*)b.d_base;
        a.sstride = b.sstride;
        a.bstride = b.bstride;
        a.records = b.d_records;
        a.in = (const uint8_t*)b.d_in;
        a.delta_out = (uint8_t*)b.d_delta_out;
        a.B = b.B;
        a.max_len = b.max_len;
        a.in_bytes = b.in_bytes;
        a.S = b.S;
        a.mode = b.mode;
    });
}

// The class's encoding matrix, m x k; a class that defines none (the product codes) leaves the buffer as it was.
int ec_matrix(ecg_ec* ec, std::vector<int>& M, int& k, int& m) {
    if (ec->impl->mem != ECG_MEM_DEVICE) return refuse("the handle is not an ECG_MEM_DEVICE handle");
    k = ec->impl->k;
    m = ec->impl->m;
    if (k < 1 || m < 1) return refuse("k = " + num(k) + ", m = " + num(m) + ": both must be >= 1");
    M.assign((size_t)k * m, -1);
    if (const int rc = ec->impl->make_encoding_matrix(M.data()); rc != ECG_OK) return rc;
    for (const int v : M)
        if (v < 0) return refuse("the class defines no encoding matrix (product codes update row by row and column "
                                 "by column through ecg_update_matrix_batch)");
    if ((long long)k + m > kInlineSrc)
        return refuse("k_in + m_out = " + num((long long)k + m) + " exceeds " + num(kInlineSrc));
    return ECG_OK;
}

std::vector<int> iota_from(int first, int n) {
    std::vector<int> v((size_t)n);
    for (int i = 0; i < n; i++) v[i] = first + i;
    return v;
}

// The state of a record on the host: the device's rule (update_kernels.hip).
int record_state(const long long* r, int k_in, long long B, int S, long long max_len, long long in_bytes) {
    const long long stripe = r[0], col = r[1], off = r[2], len = r[3], in_off = r[4];
    if (stripe < 0 || stripe >= S) return kUpdateBadStripe;
    if (col < 0 || col >= k_in) return kUpdateBadCol;
    if (off < 0 || len < 0 || off > B || len > B - off) return kUpdateBadRange;
    if (len > max_len) return kUpdateTooLong;
    if (in_off < 0 || in_off > in_bytes || len > in_bytes - in_off) return kUpdateBadStaging;
    return kUpdateApplied;
}

// [lo, hi) into a set of pairwise disjoint ranges keyed by (group, lo): false if it overlaps one of them.
typedef std::map<std::pair<long long, long long>, long long> RangeSet;
bool insert_disjoint(RangeSet& set, long long group, long long lo, long long hi) {
    if (hi <= lo) return true;  // an empty range overlaps nothing
    auto next = set.lower_bound({group, lo});
    if (next != set.end() && next->first.first == group && next->first.second < hi) return false;
    if (next != set.begin()) {
        auto prev = std::prev(next);
        if (prev->first.first == group && prev->second > lo) return false;
    }
    set[{group, lo}] = hi;
    return true;
}

}  // namespace

extern "C" {

int ecg_update_matrix_batch(int k_in, int m_out, const int* coef, const int* src_ids, const int* dst_ids, void* d_base,
                            long long sstride, long long bstride, long long B, int S, int mode,
                            const long long* d_records, int R, long long max_len, const void* d_in, long long in_bytes,
                            void* d_delta_out, unsigned* d_report, void* stream) {
    if (const int rc = bad_shape(k_in, m_out, coef, src_ids, dst_ids); rc != ECG_OK) return rc;
    return run_batch(k_in, m_out, coef, src_ids, dst_ids,
                     {d_base, sstride, bstride, B, S, mode, d_records, R, max_len, d_in, in_bytes, d_delta_out,
                      d_report, (hipStream_t)stream});
}

int ecg_update_encode_batch(int k, int m, const int* matrix, void* d_stripes, long long sstride, long long bstride,
                            long long B, int S, int mode, const long long* d_records, int R, long long max_len,
                            const void* d_in, long long in_bytes, void* d_delta_out, unsigned* d_report, void* stream) {
    if (k < 1 || m < 1) return refuse("k = " + num(k) + ", m = " + num(m) + ": both must be >= 1");
    if ((long long)k + m > kInlineSrc)
        return refuse("k_in + m_out = " + num((long long)k + m) + " exceeds " + num(kInlineSrc));
    if (!matrix) return refuse("matrix is NULL");
    const std::vector<int> src = iota_from(0, k), dst = iota_from(k, m);
    return run_batch(k, m, matrix, src.data(), dst.data(),
                     {d_stripes, sstride, bstride, B, S, mode, d_records, R, max_len, d_in, in_bytes, d_delta_out,
                      d_report, (hipStream_t)stream});
}

int ecg_update_ec_batch(ecg_ec* ec, void* d_stripes, long long sstride, long long bstride, long long B, int S, int mode,
                        const long long* d_records, int R, long long max_len, const void* d_in, long long in_bytes,
                        void* d_delta_out, unsigned* d_report, void* stream) {
    if (!ec) return refuse("ec is NULL");
    std::vector<int> M;
    int k, m;
    if (const int rc = ec_matrix(ec, M, k, m); rc != ECG_OK) return rc;
    const std::vector<int> src = iota_from(0, k), dst = iota_from(k, m);
    return run_batch(k, m, M.data(), src.data(), dst.data(),
                     {d_stripes, sstride, bstride, B, S, mode, d_records, R, max_len, d_in, in_bytes, d_delta_out,
                      d_report, (hipStream_t)stream});
}

int ecg_update_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size, int mode, int col,
                  long long off, long long len, const void* d_in, void* d_delta_out, unsigned* d_report) {
    if (!ec) return refuse("ec is NULL");
    if (block_size < 0) return refuse("negative size (block_size = " + num(block_size) + ")");
    if (!d_data_ptrs || !d_coding_ptrs) return refuse("a block pointer array is NULL");
    if (!d_in) return refuse("d_in is NULL");
    if (!d_report) return refuse("d_report is NULL");
    if (const int rc = bad_mode(mode, d_delta_out); rc != ECG_OK) return rc;
    std::vector<int> M;
    int k, m;
    if (const int rc = ec_matrix(ec, M, k, m); rc != ECG_OK) return rc;
    const BlockPtrs blocks{k, k + m, d_data_ptrs, d_coding_ptrs};
    if (blocks.any_null()) return refuse("a block pointer is NULL");
    const std::vector<int> src = iota_from(0, k), dst = iota_from(k, m);
    ColumnPlans cp;
    if (const int rc = make_plans(k, m, M.data(), src.data(), dst.data(), cp); rc != ECG_OK) return rc;
    const bool named = col >= 0 && col < k;
    return run_update(cp, k, 1, d_report, blocks.vec_ok(), ec->impl->stream, [&](UpdateLaunch& a) {
        a.records = nullptr;
        a.rec[0] = 0;
        a.rec[1] = col;
        a.rec[2] = off;
        a.rec[3] = len;
        a.rec[4] = 0;
        a.idata = (uint8_t*)d_data_ptrs[named ? col : 0];
        if (named)
            for (int p = 0; p < cp.mt; p++)
                if (const int id = cp.progs[col].dst_ids[p]; id >= 0) a.ipar[p] = (uint8_t*)d_coding_ptrs[id - k];
        a.in = (const uint8_t*)d_in;
        a.delta_out = (uint8_t*)d_delta_out;
        a.B = block_size;
        a.max_len = len < 0 ? 0 : std::min<long long>(len, block_size);
        a.in_bytes = len < 0 ? 0 : len;
        a.S = 1;
        a.mode = mode;
    });
}

int ecg_update_check_records(const long long* h_records, int R, int k_in, long long B, int S, long long max_len,
                             long long in_bytes, int with_delta_out) {
    if (R < 0) return refuse("negative size (R = " + num(R) + ")");  // ECG_EINVAL is -2: no record index, not -1
    if (!h_records && R > 0) return refuse("h_records is NULL");
    static const char* const rule[] = {"", "stripe is not in [0, S)", "col is not in [0, k_in)",
                                       "off < 0, len < 0 or off + len > B", "len > max_len",
                                       "in_off < 0 or in_off + len > in_bytes"};
    RangeSet ranges, staging;
    for (int i = 0; i < R; i++) {
        const long long* r = h_records + (size_t)i * kUpdateRecordWords;
        if (const int st = record_state(r, k_in, B, S, max_len, in_bytes); st != kUpdateApplied) {
            set_last_error("update: record " + num(i) + " is refused with state " + num(st) + ": " + rule[st]);
            return i;
        }
        if (!insert_disjoint(ranges, r[0], r[2], r[2] + r[3])) {
            set_last_error("update: record " + num(i) + " overlaps an earlier record's range in stripe " + num(r[0]));
            return i;
        }
        if (with_delta_out && !insert_disjoint(staging, 0, r[4], r[4] + r[3])) {
            set_last_error("update: record " + num(i) + " overlaps an earlier record's staging range (d_delta_out)");
            return i;
        }
    }
    return -1;
}

long long ecg_update_traffic_bytes(const unsigned char* nnz_per_col, const long long* h_records, int R, int mode,
                                   int with_delta_out) {
    if (!nnz_per_col || !h_records || R < 0) return refuse("traffic_bytes: a NULL array or a negative R");
    if (mode != ECG_UPDATE_WRITE && mode != ECG_UPDATE_DELTA) return refuse("traffic_bytes: mode = " + num(mode));
    long long total = 0;
    for (int i = 0; i < R; i++) {
        const long long* r = h_records + (size_t)i * kUpdateRecordWords;
        if (r[3] <= 0 || r[1] < 0) continue;
        total += r[3] * ((mode == ECG_UPDATE_WRITE ? 3 : 1) + (with_delta_out ? 1 : 0) + 2 * (long long)nnz_per_col[r[1]]);
    }
    return total;
}

int ecg_update_counters(long long* launches, long long* records) {
    update_traffic(launches, records);
    return ECG_OK;
}

int ecg_update_last_launch(int* v, int cap) { return update_last_launch(v, cap); }

}  // extern "C"
