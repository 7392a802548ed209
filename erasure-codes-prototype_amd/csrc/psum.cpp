// extern "C" entry points declared in include/ecg_psum.h (libecg_psum.so): the host side of the piece checksums.
// No tables come from the engine's program cache: the kernels' constants are compile-time data of their code object
// (psum_kernels.hip), and ecg_psum_fold uses the same arithmetic (sum_kernels.hpp).
#include <atomic>
#include <string>
#include <vector>

#include "../../include/ecg_psum.h"
#include "capi_handle.hpp"
#include "check_common.hpp"
#include "engine.hpp"
#include "psum_kernels.hpp"

using namespace ecg;

namespace {

std::atomic<long long> g_span_bytes{0};  // ecg_psum_set_span_bytes; 0 = auto

int refuse(const std::string& why) {
    set_last_error("psum: " + why);
    return ECG_EINVAL;
}

bool piece_ok(long long P) { return P >= kPsumMinPiece && P <= kPsumMaxPiece && (P & (P - 1)) == 0; }

// The checks every form shares, n known.  ECG_OK, or the refusal.
int check_batch(int n, long long B, long long P, int S_sel, const void* d_base, const unsigned* d_sums) {
    if (B < 0 || S_sel < 0) return refuse("negative size (B = " + std::to_string(B) + ", S_sel = " +
                                          std::to_string(S_sel) + ")");
    if (B >= (1LL << 31)) return refuse("B = " + std::to_string(B) + " is 2^31 or more");
    if (!piece_ok(P)) return refuse("piece_bytes = " + std::to_string(P) + " is not a power of two in [512, 2^30]");
    if (!d_base) return refuse("the stripes' base pointer is NULL");
    if (!d_sums) return refuse("d_sums is NULL");
    const long long Q = (B + P - 1) / P;
    if ((long long)S_sel * n >= (1LL << 31) || (long long)S_sel * n * Q >= (1LL << 31))
        return refuse("S_sel * n * Q = " + std::to_string(S_sel) + " * " + std::to_string(n) + " * " +
                      std::to_string(Q) + " output words is 2^31 or more");
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
int run_psum(int mode, int n, const int* src_ids, const uint8_t* const* ptrs, const void* d_base, long long sstride,
             long long bstride, long long B, long long P, const int* d_stripe_ids, int S, unsigned* d_sums,
             bool vec_ok, const Verify* vf, hipStream_t st) {
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;
    if (const hipError_t e = launch_psum(mode, n, src_ids, ptrs, d_base, sstride, bstride, B, P, d_stripe_ids, S,
                                         d_sums, vec_ok, g_span_bytes.load(std::memory_order_relaxed), st);
        e != hipSuccess)
        return hip_fail(e, "launch_psum");
    if (vf) {
        const PsumVerify v{d_sums, vf->expected, vf->targets, vf->bad, (B + P - 1) / P, S, n};
        if (const hipError_t e = launch_psum_verify(v, st); e != hipSuccess) return hip_fail(e, "launch_psum_verify");
    }
    return ECG_OK;
}

int run_strided(int n, const int* src_ids, const void* d_base, long long sstride, long long bstride, long long B,
                long long P, const int* d_stripe_ids, int S_sel, unsigned* d_sums, const Verify* vf, void* stream) {
    if (S_sel == 0 || B == 0) return ECG_OK;
    const StridedSrc src{d_base, sstride, bstride};
    return run_psum(SUM_MODE_STRIDED, n, src_ids, nullptr, d_base, sstride, bstride, B, P, d_stripe_ids, S_sel, d_sums,
                    src.vec_ok(), vf, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int ecg_psum_pieces_batch(int n, const int* src_ids, const void* d_base, long long sstride, long long bstride,
                          long long B, long long piece_bytes, const int* d_stripe_ids, int S_sel, unsigned* d_sums,
                          void* stream) {
    if (n < 1) return refuse("n = " + std::to_string(n) + " is less than 1");
    if (!src_ids) return refuse("src_ids is NULL");
    if (const int rc = check_batch(n, B, piece_bytes, S_sel, d_base, d_sums); rc != ECG_OK) return rc;
    return run_strided(n, src_ids, d_base, sstride, bstride, B, piece_bytes, d_stripe_ids, S_sel, d_sums, nullptr,
                       stream);
}

int ecg_psum_verify_batch(int n, const int* src_ids, const void* d_base, long long sstride, long long bstride,
                          long long B, long long piece_bytes, const int* d_stripe_ids, int S_sel,
                          const unsigned* d_expected, unsigned* d_sums, int* d_targets, unsigned* d_bad, void* stream) {
    if (n < 1) return refuse("n = " + std::to_string(n) + " is less than 1");
    if (!src_ids) return refuse("src_ids is NULL");
    if (const int rc = check_batch(n, B, piece_bytes, S_sel, d_base, d_sums); rc != ECG_OK) return rc;
    if (const int rc = check_verify(d_expected, d_targets, d_bad); rc != ECG_OK) return rc;
    const Verify vf{d_expected, d_targets, d_bad};
    return run_strided(n, src_ids, d_base, sstride, bstride, B, piece_bytes, d_stripe_ids, S_sel, d_sums, &vf, stream);
}

int ecg_psum_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B,
                      long long piece_bytes, const int* d_stripe_ids, int S_sel, unsigned* d_sums, void* stream) {
    if (const int rc = check_handle(ec); rc != ECG_OK) return rc;
    const std::vector<int> ids = iota(ec->impl->k + ec->impl->m);
    if (const int rc = check_batch((int)ids.size(), B, piece_bytes, S_sel, d_stripes, d_sums); rc != ECG_OK) return rc;
    return run_strided((int)ids.size(), ids.data(), d_stripes, sstride, bstride, B, piece_bytes, d_stripe_ids, S_sel,
                       d_sums, nullptr, stream);
}

int ecg_psum_verify_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B,
                             long long piece_bytes, const int* d_stripe_ids, int S_sel, const unsigned* d_expected,
                             unsigned* d_sums, int* d_targets, unsigned* d_bad, void* stream) {
    if (const int rc = check_handle(ec); rc != ECG_OK) return rc;
    const std::vector<int> ids = iota(ec->impl->k + ec->impl->m);
    if (const int rc = check_batch((int)ids.size(), B, piece_bytes, S_sel, d_stripes, d_sums); rc != ECG_OK) return rc;
    if (const int rc = check_verify(d_expected, d_targets, d_bad); rc != ECG_OK) return rc;
    const Verify vf{d_expected, d_targets, d_bad};
    return run_strided((int)ids.size(), ids.data(), d_stripes, sstride, bstride, B, piece_bytes, d_stripe_ids, S_sel,
                       d_sums, &vf, stream);
}

int ecg_psum_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size, long long piece_bytes,
                unsigned* d_sums) {
    if (const int rc = check_handle(ec); rc != ECG_OK) return rc;
    if (block_size < 0) return refuse("negative size (block_size = " + std::to_string(block_size) + ")");
    if (!piece_ok(piece_bytes))
        return refuse("piece_bytes = " + std::to_string(piece_bytes) + " is not a power of two in [512, 2^30]");
    if (!d_data_ptrs || !d_coding_ptrs) return refuse("a block pointer array is NULL");
    if (!d_sums) return refuse("d_sums is NULL");
    const int n = ec->impl->k + ec->impl->m;
    if (n > kPsumPtrs) return refuse("n = " + std::to_string(n) + " is more than " + std::to_string(kPsumPtrs) +
                                     " block pointers");
    const BlockPtrs src{ec->impl->k, n, d_data_ptrs, d_coding_ptrs};
    if (src.any_null()) return refuse("a block pointer is NULL");
    if (block_size == 0) return ECG_OK;
    const uint8_t* ptrs[kPsumPtrs];
    for (int b = 0; b < n; b++) ptrs[b] = (const uint8_t*)src.at(b);
    return run_psum(SUM_MODE_INLINE, n, nullptr, ptrs, nullptr, 0, 0, block_size, piece_bytes, nullptr, 1, d_sums,
                    src.vec_ok(), nullptr, ec->impl->stream);
}

unsigned ecg_psum_fold(const unsigned* h_sums, long long Q, long long piece_bytes, long long B) {
    if (B < 0 || Q < 0 || !piece_ok(piece_bytes) || Q != (B + piece_bytes - 1) / piece_bytes || (!h_sums && Q > 0)) {
        refuse("fold of Q = " + std::to_string(Q) + " sums of piece_bytes = " + std::to_string(piece_bytes) +
               " over B = " + std::to_string(B) + (h_sums ? "" : " at NULL"));
        return 0;
    }
    // crc32c(A || piece) = crc32c(A) * x^(8 |piece|) ^ crc32c(piece): one ladder walk per piece
    uint32_t c = 0;
    for (long long q = 0; q < Q; ++q) {
        const long long len = B - q * piece_bytes < piece_bytes ? B - q * piece_bytes : piece_bytes;
        c = crc_shift(c, (unsigned long long)len, kCrcPowers.p) ^ h_sums[q];
    }
    return c;
}

int ecg_psum_counters(long long* launches, long long* bytes) {
    psum_traffic(launches, bytes);
    return ECG_OK;
}

int ecg_psum_last_launch(int* v, int cap) { return psum_last_launch(v, cap); }

int ecg_psum_set_span_bytes(long long bytes) {
    if (bytes < 0 || bytes % kPsumRowBytes != 0 || bytes >= (1LL << 31))
        return refuse("span bytes " + std::to_string(bytes) + " is not 0 or a multiple of " +
                      std::to_string(kPsumRowBytes) + " below 2^31");
    g_span_bytes.store(bytes, std::memory_order_relaxed);
    return ECG_OK;
}

}  // extern "C"
