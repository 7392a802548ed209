// Host-side pieces shared by the entry points over a check matrix H: scrub.cpp (libecg_scrub.so), locate.cpp
// (libecg_locate.so), heal.cpp (libecg_heal.so) and heal2.cpp (libecg_heal2.so).  Header-only; no HIP launch and no
// state.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "capi_handle.hpp"
#include "engine.hpp"
#include "gf_kernels.hpp"

namespace ecg {

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

inline int hip_fail(hipError_t e, const char* what) {
    set_last_error(std::string(what) + ": " + hipGetErrorString(e));
    return ECG_EHIP;
}

// A check as the kernels take it: the columns that go through the coefficient tables, as a LinearOp whose
// "destinations" are the row numbers, and whether H = [C | I] (scrub_kernels.hpp ScrubLaunch::ident).
struct Check {
    LinearOp op;
    int ident = 0, ident_base = 0;
};

// H = [C | I] when the last r of its columns are unit columns -- column kg + q a single 1 in row q -- over
// consecutive blocks (`consecutive`: the strided form addresses them as ident_base + q), with C not empty.
inline Check make_check(int k_in, int r, const int* H, const int* src_ids, bool consecutive) {
    Check c;
    const int kg = k_in - r;
    bool ident = kg >= 1;
    for (int q = 0; ident && q < r; q++) {
        for (int p = 0; p < r; p++) ident &= (H[(size_t)p * k_in + kg + q] & 0xff) == (p == q ? 1 : 0);
        ident &= !consecutive || src_ids[kg + q] == src_ids[kg] + q;
    }
    const int cols = ident ? kg : k_in;
    c.ident = ident ? 1 : 0;
    c.ident_base = ident ? src_ids[kg] : 0;
    c.op.src_ids.assign(src_ids, src_ids + cols);
    c.op.dst_ids.resize((size_t)r);
    for (int p = 0; p < r; p++) c.op.dst_ids[p] = p;
    c.op.coef.resize((size_t)cols * r);
    for (int p = 0; p < r; p++)
        for (int j = 0; j < cols; j++) c.op.coef[(size_t)p * cols + j] = (uint8_t)(H[(size_t)p * k_in + j] & 0xff);
    return c;
}

// Sizes every entry point checks before anything else (and before any device is touched).
inline bool bad_sizes(long long B, long long S) { return B < 0 || S < 0 || B >= (1LL << 31); }

// [matrix | I] over k + m blocks; the row of an all-zero matrix row stays all zero (not checked)
inline std::vector<int> encode_check(int k, int m, const int* matrix) {
    const size_t n = (size_t)k + m;
    std::vector<int> H((size_t)m * n, 0);
    for (int p = 0; p < m; p++) {
        bool any = false;
        for (int j = 0; j < k; j++) any |= (H[p * n + j] = matrix[(size_t)p * k + j] & 0xff) != 0;
        if (any) H[p * n + k + p] = 1;
    }
    return H;
}

inline std::vector<int> iota(int n) {
    std::vector<int> v((size_t)n);
    for (int i = 0; i < n; i++) v[i] = i;
    return v;
}

// The check matrix of an ErasureCode handle, r x n: ECG_OK, the code's own error, or what `refuse(n, r)` makes of its
// size (ECG_OK, or the library's refusal).
template <class Refuse>
int ec_check(ecg_ec* ec, Refuse refuse, std::vector<int>& H, int& n, int& r) {
    r = ec->impl->check_matrix(H);
    if (r < 0) return r;
    if (r < 1) return ECG_EINVAL;
    n = (int)(H.size() / (size_t)r);
    return refuse(n, r);
}

// The sources of a strided form, S stripes of blocks at d_base + s * sstride + b * bstride: whether the vector path
// may read them, and (called with the launch's GfLaunch) their place in the descriptor.
struct StridedSrc {
    const void* d_base;
    long long sstride, bstride;
    bool vec_ok() const { return aligned16(d_base) && sstride % 16 == 0 && bstride % 16 == 0; }
    void operator()(GfLaunch& g) const {
        g.in_base = (const uint8_t*)d_base;
        g.in_sstride = sstride;
        g.in_bstride = bstride;
    }
};

// The sources of a single-stripe `_ec` form: block b < k is d_data_ptrs[b], block b >= k is d_coding_ptrs[b - k].
struct BlockPtrs {
    int k, n;
    char **d_data_ptrs, **d_coding_ptrs;
    const void* at(int b) const { return b < k ? d_data_ptrs[b] : d_coding_ptrs[b - k]; }
    bool any_null() const {
        for (int b = 0; b < n; b++)
            if (!at(b)) return true;
        return false;
    }
    bool vec_ok() const {
        bool ok = true;
        for (int b = 0; b < n; b++) ok &= aligned16(at(b));
        return ok;
    }
    void operator()(GfLaunch& g) const {
        for (int b = 0; b < n; b++) g.isrc[b] = (const uint8_t*)at(b);
    }
};

}  // namespace ecg
