// extern "C" entry points declared in include/ecg_sum.h (libecg_sum.so): the host side of the block checksums.
// No tables come from the engine's program cache: the kernels' constants are compile-time data of their code object
// (sum_kernels.hip), and the host functions below use the same arithmetic (sum_kernels.hpp).
#include <string.h>

#include <atomic>
#include <string>
#include <vector>

#include "../../include/ecg_sum.h"
#include "capi_handle.hpp"
#include "check_common.hpp"
#include "engine.hpp"
#include "sum_kernels.hpp"

using namespace ecg;

namespace {

std::atomic<long long> g_segment_bytes{0};  // ecg_sum_set_segment_bytes; 0 = auto
std::atomic<int> g_table_scheme{-1};        // ecg_sum_set_table_scheme; -1 = auto

int refuse(const std::string& why) {
    set_last_error("sum: " + why);
    return ECG_EINVAL;
}

// The checks every batch form shares.  ECG_OK, or the refusal.
int check_batch(long long B, int S_sel, const void* d_base, const unsigned* d_sums) {
    if (B < 0 || S_sel < 0) return refuse("negative size (B = " + std::to_string(B) + ", S_sel = " +
                                          std::to_string(S_sel) + ")");
    if (B >= (1LL << 31)) return refuse("B = " + std::to_string(B) + " is 2^31 or more");
    if (!d_base) return refuse("the stripes' base pointer is NULL");
    if (!d_sums) return refuse("d_sums is NULL");
    return ECG_OK;
}

int check_verify(const unsigned* d_expected, const int* d_targets, const unsigned* d_bad) {
    if (!d_expected) return refuse("d_expected is NULL");
    if (!d_targets) return refuse("d_targets is NULL");
    if (!d_bad) return refuse("d_bad is NULL");
    return ECG_OK;
}

int check_handle(const ecg_ec* ec) {
    if (!ec) return refuse("the handle is NULL");
    if (ec->impl->mem != ECG_MEM_DEVICE) return refuse("the handle is not an ECG_MEM_DEVICE handle");
    if (ec->impl->k < 1 || ec->impl->m < 0) return refuse("the handle has no blocks");
    return ECG_OK;
}

struct Verify {
    const unsigned* expected;
    int* targets;
    unsigned* bad;
};

// Flush the thread's batch scope, sum, and compare if asked.
int run_sum(int mode, int n, const int* src_ids, const uint8_t* const* ptrs, const void* d_base, long long sstride,
            long long bstride, long long B, const int* d_stripe_ids, int S, unsigned* d_sums, bool vec_ok,
            const Verify* vf, hipStream_t st) {
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;
    if (const hipError_t e = launch_sum(mode, n, src_ids, ptrs, d_base, sstride, bstride, B, d_stripe_ids, S, d_sums,
                                        vec_ok, g_segment_bytes.load(std::memory_order_relaxed),
                                        g_table_scheme.load(std::memory_order_relaxed), st);
        e != hipSuccess)
        return hip_fail(e, "launch_sum");
    if (vf) {
        const SumVerify v{d_sums, vf->expected, vf->targets, vf->bad, S, n};
        if (const hipError_t e = launch_sum_verify(v, st); e != hipSuccess) return hip_fail(e, "launch_sum_verify");
    }
    return ECG_OK;
}

int run_strided(int n, const int* src_ids, const void* d_base, long long sstride, long long bstride, long long B,
                const int* d_stripe_ids, int S_sel, unsigned* d_sums, const Verify* vf, void* stream) {
    if (S_sel == 0 || B == 0) return ECG_OK;
    const StridedSrc src{d_base, sstride, bstride};
    return run_sum(SUM_MODE_STRIDED, n, src_ids, nullptr, d_base, sstride, bstride, B, d_stripe_ids, S_sel, d_sums,
                   src.vec_ok(), vf, (hipStream_t)stream);
}

// Slicing-by-8 tables of the host sum: t[0] is the byte table of the definition, t[s][v] = t[s-1][v] * x^8.
struct HostTables {
    uint32_t t[8][256];
    HostTables() {
        for (uint32_t v = 0; v < 256; ++v) {
            uint32_t c = v;
            for (int b = 0; b < 8; ++b) c = crc_mulx(c);
            t[0][v] = c;
        }
        for (int s = 1; s < 8; ++s)
            for (int v = 0; v < 256; ++v) t[s][v] = (t[s - 1][v] >> 8) ^ t[0][t[s - 1][v] & 0xffu];
    }
};

}  // namespace

extern "C" {

int ecg_sum_blocks_batch(int n, const int* src_ids, const void* d_base, long long sstride, long long bstride,
                         long long B, const int* d_stripe_ids, int S_sel, unsigned* d_sums, void* stream) {
    if (n < 1) return refuse("n = " + std::to_string(n) + " is less than 1");
    if (!src_ids) return refuse("src_ids is NULL");
    if (const int rc = check_batch(B, S_sel, d_base, d_sums); rc != ECG_OK) return rc;
    return run_strided(n, src_ids, d_base, sstride, bstride, B, d_stripe_ids, S_sel, d_sums, nullptr, stream);
}

int ecg_sum_verify_batch(int n, const int* src_ids, const void* d_base, long long sstride, long long bstride,
                         long long B, const int* d_stripe_ids, int S_sel, const unsigned* d_expected, unsigned* d_sums,
                         int* d_targets, unsigned* d_bad, void* stream) {
    if (n < 1) return refuse("n = " + std::to_string(n) + " is less than 1");
    if (!src_ids) return refuse("src_ids is NULL");
    if (const int rc = check_batch(B, S_sel, d_base, d_sums); rc != ECG_OK) return rc;
    if (const int rc = check_verify(d_expected, d_targets, d_bad); rc != ECG_OK) return rc;
    const Verify vf{d_expected, d_targets, d_bad};
    return run_strided(n, src_ids, d_base, sstride, bstride, B, d_stripe_ids, S_sel, d_sums, &vf, stream);
}

int ecg_sum_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B,
                     const int* d_stripe_ids, int S_sel, unsigned* d_sums, void* stream) {
    if (const int rc = check_handle(ec); rc != ECG_OK) return rc;
    if (const int rc = check_batch(B, S_sel, d_stripes, d_sums); rc != ECG_OK) return rc;
    const std::vector<int> ids = iota(ec->impl->k + ec->impl->m);
    return run_strided((int)ids.size(), ids.data(), d_stripes, sstride, bstride, B, d_stripe_ids, S_sel, d_sums,
                       nullptr, stream);
}

int ecg_sum_verify_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B,
                            const int* d_stripe_ids, int S_sel, const unsigned* d_expected, unsigned* d_sums,
                            int* d_targets, unsigned* d_bad, void* stream) {
    if (const int rc = check_handle(ec); rc != ECG_OK) return rc;
    if (const int rc = check_batch(B, S_sel, d_stripes, d_sums); rc != ECG_OK) return rc;
    if (const int rc = check_verify(d_expected, d_targets, d_bad); rc != ECG_OK) return rc;
    const std::vector<int> ids = iota(ec->impl->k + ec->impl->m);
    const Verify vf{d_expected, d_targets, d_bad};
    return run_strided((int)ids.size(), ids.data(), d_stripes, sstride, bstride, B, d_stripe_ids, S_sel, d_sums, &vf,
                       stream);
}

int ecg_sum_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size, unsigned* d_sums) {
    if (const int rc = check_handle(ec); rc != ECG_OK) return rc;
    if (block_size < 0) return refuse("negative size (block_size = " + std::to_string(block_size) + ")");
    if (!d_data_ptrs || !d_coding_ptrs) return refuse("a block pointer array is NULL");
    if (!d_sums) return refuse("d_sums is NULL");
    const int n = ec->impl->k + ec->impl->m;
    if (n > kSumPtrs) return refuse("n = " + std::to_string(n) + " is more than " + std::to_string(kSumPtrs) +
                                    " block pointers");
    const BlockPtrs src{ec->impl->k, n, d_data_ptrs, d_coding_ptrs};
    if (src.any_null()) return refuse("a block pointer is NULL");
    if (block_size == 0) return ECG_OK;
    const uint8_t* ptrs[kSumPtrs];
    for (int b = 0; b < n; b++) ptrs[b] = (const uint8_t*)src.at(b);
    return run_sum(SUM_MODE_INLINE, n, nullptr, ptrs, nullptr, 0, 0, block_size, nullptr, 1, d_sums, src.vec_ok(),
                   nullptr, ec->impl->stream);
}

unsigned ecg_sum_crc32c(const void* host_bytes, long long len) {
    if (len < 0 || (!host_bytes && len > 0)) {
        refuse("crc32c of " + std::to_string(len) + " bytes at " + (host_bytes ? "a pointer" : "NULL"));
        return 0;
    }
    static const HostTables T;
    const uint8_t* p = (const uint8_t*)host_bytes;
    uint32_t c = 0xFFFFFFFFu;
    for (; len >= 8; len -= 8, p += 8) {
        uint32_t lo, hi;
        memcpy(&lo, p, 4);
        memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = T.t[7][lo & 0xffu] ^ T.t[6][(lo >> 8) & 0xffu] ^ T.t[5][(lo >> 16) & 0xffu] ^ T.t[4][lo >> 24] ^
            T.t[3][hi & 0xffu] ^ T.t[2][(hi >> 8) & 0xffu] ^ T.t[1][(hi >> 16) & 0xffu] ^ T.t[0][hi >> 24];
    }
    for (; len > 0; --len, ++p) c = (c >> 8) ^ T.t[0][(c ^ *p) & 0xffu];
    return c ^ 0xFFFFFFFFu;
}

unsigned ecg_sum_combine(unsigned crc_a, unsigned crc_b, long long len_b) {
    if (len_b < 0) {
        refuse("combine with len_b = " + std::to_string(len_b));
        return 0;
    }
    return crc_shift(crc_a, (unsigned long long)len_b, kCrcPowers.p) ^ crc_b;
}

int ecg_sum_counters(long long* launches, long long* bytes) {
    sum_traffic(launches, bytes);
    return ECG_OK;
}

int ecg_sum_last_launch(int* v, int cap) { return sum_last_launch(v, cap); }

int ecg_sum_set_segment_bytes(long long bytes) {
    if (bytes < 0 || bytes % kSumRowBytes != 0 || bytes >= (1LL << 31))
        return refuse("segment bytes " + std::to_string(bytes) + " is not 0 or a multiple of " +
                      std::to_string(kSumRowBytes) + " below 2^31");
    g_segment_bytes.store(bytes, std::memory_order_relaxed);
    return ECG_OK;
}

int ecg_sum_set_table_scheme(int scheme) {
    if (scheme < -1 || scheme > 1) return refuse("table scheme " + std::to_string(scheme) + " is not -1, 0 or 1");
    g_table_scheme.store(scheme, std::memory_order_relaxed);
    return ECG_OK;
}

}  // extern "C"
