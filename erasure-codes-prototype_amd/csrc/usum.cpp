// extern "C" entry points declared in include/ecg_usum.h (libecg_usum.so): the host side of the update sums.
// A call requests the program set update.cpp requests for the same G -- k_in single-source programs of mt rows, so the
// engine's program cache answers both libraries from one entry and one table upload --, zeroes the report on the
// stream and launches once.  ecg_usum_expected is the same definition on host arrays, one record after the other.
// make_plans and bad_shape restate update.cpp's (each library keeps its refusals under its own name).
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ecg_usum.h"
#include "capi_handle.hpp"
#include "check_common.hpp"
#include "engine.hpp"
#include "gf256.hpp"
#include "usum_kernels.hpp"

using namespace ecg;

namespace {

int refuse(const std::string& why) {
    set_last_error("usum: " + why);
    return ECG_EINVAL;
}

std::string num(long long v) { return std::to_string(v); }

// The plans of G's columns as the programs of one set (update.cpp make_plans: the same set, the same cache entry).
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
                          num(kUpdateMaxNnz) + " (one lane holds the streams of a record)");
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

// "" if ids[0..n) are non-negative and distinct, else what is wrong with them
std::string bad_ids(const char* name, const int* ids, int n) {
    std::vector<int> v(ids, ids + n);
    std::sort(v.begin(), v.end());
    if (v[0] < 0) return std::string(name) + " holds a negative id (" + num(v[0]) + ")";
    for (int j = 1; j < n; j++)
        if (v[j] == v[j - 1]) return std::string(name) + " names block " + num(v[j]) + " twice";
    return "";
}

int bad_shape(int k_in, int m_out, const int* coef, const int* src_ids, const int* dst_ids) {
    if (k_in < 1 || m_out < 1)
        return refuse("k_in = " + num(k_in) + ", m_out = " + num(m_out) + ": both must be >= 1");
    if ((long long)k_in + m_out > kInlineSrc)
        return refuse("k_in + m_out = " + num((long long)k_in + m_out) + " exceeds " + num(kInlineSrc));
    if (!coef) return refuse("coef is NULL");
    if (!src_ids || !dst_ids) return refuse(!src_ids ? "src_ids is NULL" : "dst_ids is NULL");
    if (const std::string why = bad_ids("src_ids", src_ids, k_in); !why.empty()) return refuse(why);
    if (const std::string why = bad_ids("dst_ids", dst_ids, m_out); !why.empty()) return refuse(why);
    for (int i = 0; i < m_out; i++)
        if (std::find(src_ids, src_ids + k_in, dst_ids[i]) != src_ids + k_in)
            return refuse("block " + num(dst_ids[i]) + " is both a source and a destination");
    return ECG_OK;
}

bool piece_ok(long long P) { return P == 0 || (P >= 512 && P <= (1LL << 30) && (P & (P - 1)) == 0); }

long long pieces_of(long long B, long long P) { return P == 0 ? 1 : (B + P - 1) / P; }

// What the device and the host form take after G: records, delta, the table, the reports.
struct Args {
    long long B;
    int S;
    const long long* records;
    int R;
    long long max_len;
    const void* delta;
    long long in_bytes;
    const int* sum_ids;
    int n_sums;
    long long piece_bytes;
    int which;
    unsigned* sums;
    const unsigned* update_report;
    unsigned* report;
};

// The rules both forms share; `rec`, `dl`, `sm`, `rp` name the arrays in the refusal (d_... or h_...).
int bad_args(const Args& b, const char* rec, const char* dl, const char* sm, const char* rp) {
    if (b.B < 0 || b.S < 0 || b.R < 0 || b.max_len < 0 || b.in_bytes < 0)
        return refuse("negative size (B = " + num(b.B) + ", S = " + num(b.S) + ", R = " + num(b.R) +
                      ", max_len = " + num(b.max_len) + ", in_bytes = " + num(b.in_bytes) + ")");
    if (b.B >= (1LL << 31)) return refuse("B = " + num(b.B) + " is not below 2^31");
    if (b.max_len > b.B) return refuse("max_len = " + num(b.max_len) + " exceeds B = " + num(b.B));
    if (!piece_ok(b.piece_bytes))
        return refuse("piece_bytes = " + num(b.piece_bytes) + " is neither 0 nor a power of two in [512, 2^30]");
    if (b.which < 1 || b.which > 3)
        return refuse("which = " + num(b.which) + " is not 1 (data), 2 (parity) or 3 (both)");
    if (!b.sum_ids) return refuse("sum_ids is NULL");
    if (b.n_sums < 1 || b.n_sums > kUsumIds)
        return refuse("n_sums = " + num(b.n_sums) + " is not in [1, " + num(kUsumIds) + "]");
    if (const std::string why = bad_ids("sum_ids", b.sum_ids, b.n_sums); !why.empty()) return refuse(why);
    const long long Q = pieces_of(b.B, b.piece_bytes);
    if ((long long)b.S * b.n_sums * Q >= (1LL << 31))  // at most 2^31 * 2^7 * 2^22: no overflow
        return refuse("S * n_sums * Q = " + num(b.S) + " * " + num(b.n_sums) + " * " + num(Q) +
                      " sum words is 2^31 or more");
    if (!b.records) return refuse(std::string(rec) + " is NULL");
    if (!b.delta) return refuse(std::string(dl) + " is NULL");
    if (!b.sums) return refuse(std::string(sm) + " is NULL");
    if (!b.report) return refuse(std::string(rp) + " is NULL");
    return ECG_OK;
}

int run_batch(int k_in, int m_out, const int* coef, const int* src_ids, const int* dst_ids, const Args& b,
              hipStream_t st) {
    if (const int rc = bad_args(b, "d_records", "d_delta", "d_sums", "d_report"); rc != ECG_OK) return rc;
    if (((uintptr_t)b.records & 7u) != 0) return refuse("d_records is not 8-byte aligned");
    if (((uintptr_t)b.sums & 3u) != 0) return refuse("d_sums is not 4-byte aligned");
    int cpw, wpr;
    if (!usum_grid(b.max_len, b.R, cpw, wpr))
        return refuse("R = " + num(b.R) + " records of " + num(wpr) + " workgroups each need more than 2^31 - 1 "
                      "workgroups");
    ColumnPlans cp;
    if (const int rc = make_plans(k_in, m_out, coef, src_ids, dst_ids, cp); rc != ECG_OK) return rc;
    if (b.R == 0) return ECG_OK;
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;
    int status = ECG_OK;
    const std::shared_ptr<ProgramSet> ps = Engine::instance().program_set(cp.progs, &status, st);
    if (!ps) return status;
    if (const int rc = ps->ensure_ready(st); rc != ECG_OK) return rc;
    if (ps->nprog != k_in || ps->k != 1 || ps->MT != cp.mt || ps->rtiles != 1) return ECG_EINVAL;
    if (const hipError_t e = hipMemsetAsync(b.report, 0, (size_t)b.R * 2 * sizeof(unsigned), st); e != hipSuccess)
        return hip_fail(e, "hipMemsetAsync(usum report)");
    UsumLaunch a;
    memset(&a, 0, sizeof(a));
    a.tabs = ps->d_tabs;
    a.src_ids = ps->d_src;
    a.dst_ids = ps->d_dst;
    a.records = b.records;
    a.delta = (const uint8_t*)b.delta;
    a.update_report = b.update_report;
    a.sums = b.sums;
    a.report = b.report;
    a.B = b.B;
    a.max_len = b.max_len;
    a.in_bytes = b.in_bytes;
    a.piece_bytes = b.piece_bytes;
    a.Q = pieces_of(b.B, b.piece_bytes);
    a.S = b.S;
    a.k_in = k_in;
    a.mt = cp.mt;
    a.R = b.R;
    a.which = b.which;
    a.n_sums = b.n_sums;
    for (int c = 0; c < b.n_sums; c++) a.sum_ids[c] = b.sum_ids[c];
    if (const hipError_t e = launch_usum(a, cp.max_nnz, st); e != hipSuccess) return hip_fail(e, "launch_usum");
    Engine::instance().note_launch(*ps, st);
    return ECG_OK;
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
        if (v < 0) return refuse("the class defines no encoding matrix (product codes carry their sums row by row and "
                                 "column by column through ecg_usum_matrix_batch)");
    if ((long long)k + m > kInlineSrc)
        return refuse("k_in + m_out = " + num((long long)k + m) + " exceeds " + num(kInlineSrc));
    return ECG_OK;
}

std::vector<int> iota_from(int first, int n) {
    std::vector<int> v((size_t)n);
    for (int i = 0; i < n; i++) v[i] = first + i;
    return v;
}

// The state of a record on the host: the device's rule (usum_kernels.hip).
unsigned record_state(const long long* r, int k_in, long long B, int S, long long max_len, long long in_bytes) {
    const long long stripe = r[0], col = r[1], off = r[2], len = r[3], in_off = r[4];
    if (stripe < 0 || stripe >= S) return kUpdateBadStripe;
    if (col < 0 || col >= k_in) return kUpdateBadCol;
    if (off < 0 || len < 0 || off > B || len > B - off) return kUpdateBadRange;
    if (len > max_len) return kUpdateTooLong;
    if (in_off < 0 || in_off > in_bytes || len > in_bytes - in_off) return kUpdateBadStaging;
    return kUpdateApplied;
}

// raw(c * d[0..n)): the bitwise definition, a byte at a time
uint32_t raw_of(const uint8_t* d, long long n, int c) {
    uint32_t v = 0u;
    for (long long i = 0; i < n; i++) {
        v ^= (uint32_t)gf::mul(c, d[i]);
        for (int b = 0; b < 8; b++) v = crc_mulx(v);
    }
    return v;
}

int column_of(const int* sum_ids, int n_sums, int id) {
    for (int c = 0; c < n_sums; c++)
        if (sum_ids[c] == id) return c;
    return -1;
}

}  // namespace

extern "C" {

int ecg_usum_matrix_batch(int k_in, int m_out, const int* coef, const int* src_ids, const int* dst_ids, long long B,
                          int S, const long long* d_records, int R, long long max_len, const void* d_delta,
                          long long in_bytes, const int* sum_ids, int n_sums, long long piece_bytes, int which,
                          unsigned* d_sums, const unsigned* d_update_report, unsigned* d_report, void* stream) {
    if (const int rc = bad_shape(k_in, m_out, coef, src_ids, dst_ids); rc != ECG_OK) return rc;
    return run_batch(k_in, m_out, coef, src_ids, dst_ids,
                     {B, S, d_records, R, max_len, d_delta, in_bytes, sum_ids, n_sums, piece_bytes, which, d_sums,
                      d_update_report, d_report},
                     (hipStream_t)stream);
}

int ecg_usum_encode_batch(int k, int m, const int* matrix, long long B, int S, const long long* d_records, int R,
                          long long max_len, const void* d_delta, long long in_bytes, long long piece_bytes, int which,
                          unsigned* d_sums, const unsigned* d_update_report, unsigned* d_report, void* stream) {
    if (k < 1 || m < 1) return refuse("k = " + num(k) + ", m = " + num(m) + ": both must be >= 1");
    if ((long long)k + m > kInlineSrc)
        return refuse("k_in + m_out = " + num((long long)k + m) + " exceeds " + num(kInlineSrc));
    if (!matrix) return refuse("matrix is NULL");
    const std::vector<int> src = iota_from(0, k), dst = iota_from(k, m), all = iota_from(0, k + m);
    return run_batch(k, m, matrix, src.data(), dst.data(),
                     {B, S, d_records, R, max_len, d_delta, in_bytes, all.data(), k + m, piece_bytes, which, d_sums,
                      d_update_report, d_report},
                     (hipStream_t)stream);
}

int ecg_usum_ec_batch(ecg_ec* ec, long long B, int S, const long long* d_records, int R, long long max_len,
                      const void* d_delta, long long in_bytes, long long piece_bytes, int which, unsigned* d_sums,
                      const unsigned* d_update_report, unsigned* d_report, void* stream) {
    if (!ec) return refuse("ec is NULL");
    std::vector<int> M;
    int k, m;
    if (const int rc = ec_matrix(ec, M, k, m); rc != ECG_OK) return rc;
    const std::vector<int> src = iota_from(0, k), dst = iota_from(k, m), all = iota_from(0, k + m);
    return run_batch(k, m, M.data(), src.data(), dst.data(),
                     {B, S, d_records, R, max_len, d_delta, in_bytes, all.data(), k + m, piece_bytes, which, d_sums,
                      d_update_report, d_report},
                     (hipStream_t)stream);
}

int ecg_usum_expected(int k_in, int m_out, const int* coef, const int* src_ids, const int* dst_ids, long long B, int S,
                      const long long* h_records, int R, long long max_len, const void* h_delta, long long in_bytes,
                      const int* sum_ids, int n_sums, long long piece_bytes, int which, unsigned* h_sums,
                      const unsigned* h_update_report, unsigned* h_report) {
    if (const int rc = bad_shape(k_in, m_out, coef, src_ids, dst_ids); rc != ECG_OK) return rc;
    const Args b{B, S, h_records, R, max_len, h_delta, in_bytes, sum_ids, n_sums, piece_bytes, which, h_sums,
                 h_update_report, h_report};
    if (const int rc = bad_args(b, "h_records", "h_delta", "h_sums", "h_report"); rc != ECG_OK) return rc;
    ColumnPlans cp;  // only for its refusal: the host form needs no plan
    if (const int rc = make_plans(k_in, m_out, coef, src_ids, dst_ids, cp); rc != ECG_OK) return rc;
    const long long P = piece_bytes, Q = pieces_of(B, P);
    const uint8_t* delta = (const uint8_t*)h_delta;
    for (int r = 0; r < R; r++) {
        const long long* rec = h_records + (size_t)r * kUpdateRecordWords;
        unsigned state = h_update_report ? h_update_report[2 * (size_t)r] : 0u;
        if (state == kUpdateApplied) state = record_state(rec, k_in, B, S, max_len, in_bytes);
        h_report[2 * (size_t)r] = state;
        h_report[2 * (size_t)r + 1] = 0u;
        if (state != kUpdateApplied) continue;
        const long long stripe = rec[0], col = rec[1], off = rec[2], len = rec[3], in_off = rec[4];
        unsigned nonzero = 0u;
        for (long long i = 0; i < len; i++) nonzero += delta[in_off + i] != 0;
        h_report[2 * (size_t)r + 1] = nonzero;
        for (int row = -1; row < m_out; row++) {  // -1: the data block
            const int c = row < 0 ? 1 : coef[(size_t)row * k_in + col] & 0xff;
            if (c == 0 || !(which & (row < 0 ? ECG_USUM_DATA : ECG_USUM_PARITY))) continue;
            const int sc = column_of(sum_ids, n_sums, row < 0 ? src_ids[col] : dst_ids[row]);
            if (sc < 0) continue;
            for (long long a = off; a < off + len;) {
                const long long q = P ? a / P : 0;
                const long long e = P ? std::min((q + 1) * P, B) : B;
                const long long b1 = std::min(off + len, e);
                const uint32_t v = raw_of(delta + in_off + (a - off), b1 - a, c);
                h_sums[((size_t)stripe * n_sums + sc) * Q + q] ^= crc_shift(v, (unsigned long long)(e - b1), kCrcPowers.p);
                a = b1;
            }
        }
    }
    return ECG_OK;
}

long long ecg_usum_traffic_bytes(const unsigned char* nnz_per_col, const long long* h_records, int R, long long B,
                                 long long piece_bytes, int which) {
    if (!nnz_per_col || !h_records || R < 0) return refuse("traffic_bytes: a NULL array or a negative R");
    if (which < 1 || which > 3) return refuse("traffic_bytes: which = " + num(which));
    if (!piece_ok(piece_bytes) || B < 0) return refuse("traffic_bytes: piece_bytes = " + num(piece_bytes) + ", B = " + num(B));
    long long total = 0;
    for (int i = 0; i < R; i++) {
        const long long* r = h_records + (size_t)i * kUpdateRecordWords;
        if (r[3] <= 0 || r[1] < 0 || r[2] < 0) continue;
        const long long met = piece_bytes ? (r[2] + r[3] - 1) / piece_bytes - r[2] / piece_bytes + 1 : 1;
        const long long blocks = ((which & ECG_USUM_DATA) ? 1 : 0) + ((which & ECG_USUM_PARITY) ? nnz_per_col[r[1]] : 0);
        total += r[3] + 8 * met * blocks;
    }
    return total;
}

int ecg_usum_counters(long long* launches, long long* records) {
    usum_traffic(launches, records);
    return ECG_OK;
}

int ecg_usum_last_launch(int* v, int cap) { return usum_last_launch(v, cap); }

}  // extern "C"
