// The plan wave of the verified range read, device side: what gf_vread_plan_kernel (vread_kernels.hip) runs, one wave
// per record.  It RESTATES gf_dread_plan_kernel (dread_kernels.hip) line by line, plus a null `lost`: calling that
// kernel's body through an inlined function made the compiler allocate it 151 VGPRs instead of 67, so dread's kernel
// keeps its own text and the two must be changed together (tests/test_gpu_vread.py compares their answers).
// Everything here is inlined into the kernel that uses it; the header defines no kernel and no host state.
//
// The wave validates the record (states 1-5) and, for a lost column, runs the plan rule of dread_kernels.hpp over the
// stripe's lost columns, however many: the only state is the r x r row transform, one packed 64-bit word per COLUMN of
// the transform (byte q = row q), the same in every lane, every index static.  The current value of a lost column is
// transform * H[:, c], r shift-and-add products.  H and src_ids sit in the kernel arguments, a DreadLaunch at their
// start; lane L holds columns L and L + 64 of H as packed words and ends with c_L and c_{L+64} = (w * H)[.], which it
// writes, compacted by a ballot, as block id and CoefTab of the record's plan.  No LDS, no private segment, vector
// stores only.
#pragma once
#include <stddef.h>

#include "dread_kernels.hpp"
#include "gf_device.hpp"

namespace ecg {

static_assert(kMaxMT == 8, "a column of the row transform is eight bytes in one 64-bit word");
static_assert(kInlineSrc == 128, "a lane of the plan wave holds two columns of H");

typedef unsigned long long u64;

// x * 2 in every byte of the word (GF(2^8) / 0x11d)
__device__ __forceinline__ u64 xtime8(u64 x) {
    return ((x & 0x7f7f7f7f7f7f7f7fULL) << 1) ^ (((x >> 7) & 0x0101010101010101ULL) * 0x1dULL);
}

// c * x in every byte of the word, by shift and add
__device__ __forceinline__ u64 mul8(u64 x, unsigned c) {
    u64 r = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        r ^= ((c >> b) & 1u) ? x : 0ULL;
        x = xtime8(x);
    }
    return r;
}

// x * y byte by byte
__device__ __forceinline__ u64 mulv(u64 x, u64 y) {
    u64 r = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        r ^= x & (((y >> b) & 0x0101010101010101ULL) * 0xffULL);
        x = xtime8(x);
    }
    return r;
}

// the sum of the eight products: the dot product of two packed vectors
__device__ __forceinline__ unsigned dot8(u64 x, u64 y) {
    u64 p = mulv(x, y);
    p ^= p >> 32;
    p ^= p >> 16;
    p ^= p >> 8;
    return (unsigned)p & 0xffu;
}

// 1 / a = a^254 = a^2 a^4 .. a^128
__device__ __forceinline__ unsigned inv8(unsigned a) {
    unsigned x = a, r = 1u;
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        x = (unsigned)mul8(x, x) & 0xffu;
        r = (unsigned)mul8(r, x) & 0xffu;
    }
    return r;
}

__device__ __forceinline__ unsigned byte_of(u64 w, int c) { return (unsigned)(w >> (8 * c)) & 0xffu; }

__device__ __forceinline__ u64 lane_word(u64 v, int src) {
    const unsigned lo = __shfl((unsigned)v, src), hi = __shfl((unsigned)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}

// bytes [0, a, b, a ^ b]: c * e for e = 0..3 from c * 1 and c * 2
__device__ __forceinline__ uint32_t quad(unsigned a, unsigned b) { return (a << 8) | (b << 16) | ((a ^ b) << 24); }

// The CoefTab of coefficient c1 (gf_kernels.hpp), in two 16-byte stores.
__device__ __forceinline__ void store_tab(CoefTab* t, unsigned c1) {
    unsigned x[8];  // c * 2^j
    x[0] = c1;
#pragma unroll
    for (int j = 1; j < 8; ++j) x[j] = (unsigned)xtime8(x[j - 1]) & 0xffu;
    u32x4 lo, hi;
    lo.x = quad(x[0], x[1]);
    lo.y = lo.x ^ (x[2] * 0x01010101u);
    lo.z = quad(x[3], x[4]);
    lo.w = lo.z ^ (x[5] * 0x01010101u);
    hi.x = quad(x[6], x[7]);
    hi.y = c1 == 1u ? 0xffffffffu : 0u;
    hi.z = 0u;
    hi.w = 0u;
    u32x4* tab = reinterpret_cast<u32x4*>(t);
    tab[0] = lo;
    tab[1] = hi;
}

__device__ __forceinline__ unsigned record_state(const DreadLaunch& a, long long stripe, long long col, long long off,
                                                 long long len, long long out_off) {
    if (stripe < 0 || stripe >= a.S) return kDreadBadStripe;
    if (col < 0 || col >= a.n) return kDreadBadCol;
    if (off < 0 || len < 0 || off > a.B || len > a.B - off) return kDreadBadRange;
    if (len > a.max_len) return kDreadTooLong;
    if (out_off < 0 || out_off > a.out_bytes || len > a.out_bytes - out_off) return kDreadBadOut;
    return kDreadAnswered;
}

// The plan of record blockIdx.x into a.work, by the 64 lanes of one wave.  `a` is the DreadLaunch at the START of the
// kernel's arguments.  A null a.lost stands for no lost column in any stripe.
__device__ __forceinline__ void dread_plan_wave(const DreadLaunch& a) {
    const long long rix = blockIdx.x;
    const int lane = threadIdx.x;
    const ECG_CONST long long* rec = cst(a.records) + rix * kDreadRecordWords;
    const long long stripe = rec[0], col = rec[1];
    int* head = reinterpret_cast<int*>(a.work + rix * a.plan_bytes);
    unsigned state = record_state(a, stripe, col, rec[2], rec[3], rec[4]);
    if (state != kDreadAnswered) {  // uniform
        if (lane < 2) head[lane] = lane == 0 ? (int)state : 0;
        return;
    }
    // H and src_ids where the kernel arguments lie: a lane reads its own columns, which a by-value copy would take
    // through the private segment
    const ECG_CONST char* args = (const ECG_CONST char*)__builtin_amdgcn_kernarg_segment_ptr();
    const ECG_CONST uint8_t* H = (const ECG_CONST uint8_t*)(args + offsetof(DreadLaunch, H));
    const ECG_CONST int* src_ids = (const ECG_CONST int*)(args + offsetof(DreadLaunch, src_ids));
    const int n = a.n, r = a.r;
    const bool have = a.lost != nullptr;  // uniform
    const uint8_t* f = have ? a.lost + stripe * n : nullptr;
    const bool in0 = lane < n, in1 = lane + 64 < n;
    const bool l0 = have && in0 && f[lane] != 0, l1 = have && in1 && f[lane + 64] != 0;
    const u64 m0 = __ballot(l0), m1 = __ballot(l1);
    u64 h0 = 0, h1 = 0;  // columns lane and lane + 64 of H: byte p = H[p][.]
#pragma unroll
    for (int p = 0; p < kMaxMT; ++p) {
        if (p < r && in0) h0 |= (u64)H[p * n + lane] << (8 * p);
        if (p < r && in1) h1 |= (u64)H[p * n + lane + 64] << (8 * p);
    }
    const bool col_lost = ((col < 64 ? m0 >> col : m1 >> (col - 64)) & 1ULL) != 0;
    unsigned c0 = lane == col ? 1u : 0u, c1 = lane + 64 == col ? 1u : 0u;  // the copy: one source with c = 1
    if (col_lost) {  // uniform
        int nz[kMaxMT];  // nonzeros of row q in the columns outside E
#pragma unroll
        for (int q = 0; q < kMaxMT; ++q)
            nz[q] = __popcll(__ballot(in0 && !l0 && byte_of(h0, q) != 0u)) +
                    __popcll(__ballot(in1 && !l1 && byte_of(h1, q) != 0u));
        u64 Tc[kMaxMT];  // column p of the row transform: byte q = T[q][p]; the identity to begin with
#pragma unroll
        for (int p = 0; p < kMaxMT; ++p) Tc[p] = 1ULL << (8 * p);
        unsigned used = 0u;
        int pcol = -1;
        u64 w0 = m0, w1 = m1;
        while (w0 | w1) {  // the lost columns in ascending order, uniform
            int c;
            if (w0) {
                c = __ffsll(w0) - 1;
                w0 &= w0 - 1;
            } else {
                c = 64 + __ffsll(w1) - 1;
                w1 &= w1 - 1;
            }
            const u64 hc = c < 64 ? lane_word(h0, c) : lane_word(h1, c - 64);
            u64 cur = 0;  // the column as it stands: byte q = (T * H[:, c])[q]
#pragma unroll
            for (int p = 0; p < kMaxMT; ++p) cur ^= mul8(Tc[p], byte_of(hc, p));
            int best = -1, key = 1 << 30;
#pragma unroll
            for (int q = 0; q < kMaxMT; ++q) {
                const bool can = q < r && !((used >> q) & 1u) && byte_of(cur, q) != 0u;
                const int kq = nz[q] * kMaxMT + q;
                if (can && kq < key) {
                    key = kq;
                    best = q;
                }
            }
            if (best < 0) continue;  // no pivot: the column is skipped
            used |= 1u << best;
            if (c == col) pcol = best;
            const unsigned iv = inv8(byte_of(cur, best));
            const u64 keep = ~(0xffULL << (8 * best));
            const u64 fvec = cur & keep;  // what every other row holds in column c
#pragma unroll
            for (int p = 0; p < kMaxMT; ++p) {
                const unsigned s = (unsigned)mul8(byte_of(Tc[p], best), iv) & 0xffu;  // the pivot row, scaled
                Tc[p] = ((Tc[p] & keep) | ((u64)s << (8 * best))) ^ mul8(fvec, s);
            }
        }
        if (pcol < 0) {
            state = kDreadUnrecoverable;
        } else {
            u64 w = 0;  // the pivot row of col
#pragma unroll
            for (int p = 0; p < kMaxMT; ++p) w |= (u64)byte_of(Tc[p], pcol) << (8 * p);
            c0 = dot8(w, h0);
            c1 = dot8(w, h1);
            // on E, w * H is the unit vector of col, or the block is not recoverable
            const bool bad0 = l0 && c0 != (lane == col ? 1u : 0u), bad1 = l1 && c1 != (lane + 64 == col ? 1u : 0u);
            if ((__ballot(bad0) | __ballot(bad1)) != 0ULL) state = kDreadUnrecoverable;
            c0 = l0 ? 0u : c0;
            c1 = l1 ? 0u : c1;
        }
    }
    if (state != kDreadAnswered) {  // uniform
        if (lane < 2) head[lane] = lane == 0 ? (int)state : 0;
        return;
    }
    const u64 z0 = __ballot(c0 != 0u), z1 = __ballot(c1 != 0u);
    const u64 below = (1ULL << lane) - 1ULL;
    const int n0 = __popcll(z0);
    if (lane < 2) head[lane] = lane == 0 ? (int)kDreadAnswered : n0 + __popcll(z1);
    int* ids = head + kDreadHeadWords;
    CoefTab* tabs = reinterpret_cast<CoefTab*>(ids + dread_ids_words(n));
    if (c0 != 0u) {
        const int i = __popcll(z0 & below);
        ids[i] = src_ids[lane];
        store_tab(tabs + i, c0);
    }
    if (c1 != 0u) {
        const int i = n0 + __popcll(z1 & below);
        ids[i] = src_ids[lane + 64];
        store_tab(tabs + i, c1);
    }
}

}  // namespace ecg
