// extern "C" entry points declared in include/ecg_scrub.h (libecg_scrub.so): the host side of the read-only
// parity check.  A check is a LinearOp whose "destinations" are the row numbers: the engine's program cache
// (Engine::program_set) builds and keeps its coefficient tables exactly as for a region product.
#include <string.h>

#include <string>
#include <vector>

#include "../../include/ecg_scrub.h"
#include "capi_handle.hpp"
#include "check_common.hpp"
#include "engine.hpp"
#include "scrub_kernels.hpp"

using namespace ecg;

namespace {

// Flush the thread's batch scope, fetch the tables, zero the counters, launch.  `fill` sets the launch's sources.
template <class Fill>
int run_check(const Check& chk, int mode, long long B, int S, unsigned* d_counts, bool vec_ok, hipStream_t st,
              Fill fill) {
    const LinearOp& op = chk.op;
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;
    Engine& eng = Engine::instance();
    int status = ECG_OK;
    std::shared_ptr<ProgramSet> ps = eng.program_set(&op, 1, &status, st);
    if (!ps) return status;
    if (const int rc = ps->ensure_ready(st); rc != ECG_OK) return rc;
    ScrubLaunch a;
    memset(&a, 0, sizeof(a));
    a.g.tabs = ps->d_tabs;
    a.g.src_ids = ps->d_src;
    a.g.dst_ids = ps->d_dst;
    a.g.B = B;
    a.g.k = ps->k;
    a.g.m = ps->m;
    a.g.S = S;
    a.g.MT = ps->MT;
    a.g.rtiles = ps->rtiles;
    a.g.binary = ps->binary ? 1 : 0;
    a.counts = d_counts;
    a.ident = chk.ident;
    a.ident_base = chk.ident_base;
    fill(a.g);
    if (const hipError_t e = hipMemsetAsync(d_counts, 0, (size_t)S * (size_t)ps->m * sizeof(unsigned), st);
        e != hipSuccess)
        return hip_fail(e, "hipMemsetAsync(scrub counts)");
    if (const hipError_t e = launch_scrub(a, mode, vec_ok, st); e != hipSuccess) return hip_fail(e, "launch_scrub");
    eng.note_launch(*ps, st);
    return ECG_OK;
}

int run_strided_check(const Check& chk, const void* d_base, long long sstride, long long bstride, long long B, int S,
                      unsigned* d_counts, hipStream_t st) {
    const StridedSrc src{d_base, sstride, bstride};
    return run_check(chk, GF_MODE_STRIDED, B, S, d_counts, src.vec_ok(), st, src);
}

// The scrub has a kernel for every r (row tiles); only the inline form's descriptor bounds n.
int any_size(int, int) { return ECG_OK; }
int inline_size(int n, int) { return n > kInlineSrc ? ECG_EINVAL : ECG_OK; }

}  // namespace

extern "C" {

int ecg_scrub_matrix_batch(int k_in, int r, const int* H, const int* src_ids, const void* d_base, long long sstride,
                           long long bstride, long long B, int S, unsigned* d_counts, void* stream) {
    if (k_in < 1 || r < 1 || bad_sizes(B, S) || !H || !src_ids || !d_base || !d_counts) return ECG_EINVAL;
    if (S == 0 || B == 0) return ECG_OK;
    return run_strided_check(make_check(k_in, r, H, src_ids, true), d_base, sstride, bstride, B, S, d_counts,
                             (hipStream_t)stream);
}

int ecg_scrub_encode_batch(int k, int m, const int* matrix, const void* d_stripes, long long sstride,
                           long long bstride, long long B, int S, unsigned* d_counts, void* stream) {
    if (k < 1 || m < 1 || bad_sizes(B, S) || !matrix || !d_stripes || !d_counts) return ECG_EINVAL;
    if (S == 0 || B == 0) return ECG_OK;
    const std::vector<int> H = encode_check(k, m, matrix), ids = iota(k + m);
    return run_strided_check(make_check(k + m, m, H.data(), ids.data(), true), d_stripes, sstride, bstride, B, S,
                             d_counts, (hipStream_t)stream);
}

int ecg_scrub_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B, int S,
                       unsigned* d_counts, void* stream) {
    if (!ec || bad_sizes(B, S) || !d_stripes || !d_counts || ec->impl->mem != ECG_MEM_DEVICE) return ECG_EINVAL;
    std::vector<int> H;
    int n, r;
    if (const int rc = ec_check(ec, any_size, H, n, r); rc != ECG_OK) return rc;
    if (S == 0 || B == 0) return ECG_OK;
    const std::vector<int> ids = iota(n);
    return run_strided_check(make_check(n, r, H.data(), ids.data(), true), d_stripes, sstride, bstride, B, S, d_counts,
                             (hipStream_t)stream);
}

int ecg_scrub_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size, unsigned* d_counts) {
    if (!ec || block_size < 0 || !d_data_ptrs || !d_coding_ptrs || !d_counts || ec->impl->mem != ECG_MEM_DEVICE)
        return ECG_EINVAL;
    std::vector<int> H;
    int n, r;
    if (const int rc = ec_check(ec, inline_size, H, n, r); rc != ECG_OK) return rc;
    const BlockPtrs src{ec->impl->k, n, d_data_ptrs, d_coding_ptrs};
    if (src.any_null()) return ECG_EINVAL;
    if (block_size == 0) return ECG_OK;
    const std::vector<int> ids = iota(n);
    return run_check(make_check(n, r, H.data(), ids.data(), false), GF_MODE_INLINE, block_size, 1, d_counts,
                     src.vec_ok(), ec->impl->stream, src);
}

int ecg_scrub_suspects(int r, int n, const int* H, const unsigned* h_counts, int* ids, int cap) {
    if (r < 1 || n < 1 || !H || !h_counts || cap < 0) return ECG_EINVAL;
    bool any = false;
    for (int p = 0; p < r; p++) any |= h_counts[p] != 0;
    if (!any) return 0;
    std::vector<int> found;
    for (int b = 0; b < n; b++) {
        bool same = true;
        for (int p = 0; p < r && same; p++) same = (H[(size_t)p * n + b] != 0) == (h_counts[p] != 0);
        if (same) found.push_back(b);
    }
    if (ids && cap >= (int)found.size() && !found.empty()) memcpy(ids, found.data(), found.size() * sizeof(int));
    return (int)found.size();
}

int ecg_scrub_counters(long long* launches, long long* bytes) {
    scrub_traffic(launches, bytes);
    return ECG_OK;
}

int ecg_scrub_last_launch(int* v, int cap) { return scrub_last_launch(v, cap); }

}  // extern "C"
