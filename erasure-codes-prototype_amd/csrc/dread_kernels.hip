// Degraded range read for MI355X (gfx950, CDNA4): byte ranges of stored blocks answered into a caller buffer, lost
// blocks rebuilt from the survivors their reconstruction really needs.  Nothing of the stripes is written.
//
//   gf_dread_plan_kernel   one wave per record, before the main launch on the same stream.  It validates the record
//       (states 1-5) and, for a lost column, runs the plan rule of dread_kernels.hpp over the stripe's lost columns,
//       however many: the only state is the r x r row transform, one packed 64-bit word per COLUMN of the transform
//       (byte q = row q), the same in every lane, every index static.  The current value of a lost column is
//       transform * H[:, c], r shift-and-add products.  H and src_ids sit in the kernel arguments; lane L holds
//       columns L and L + 64 of H as packed words and ends with c_L and c_{L+64} = (w * H)[.], which it writes,
//       compacted by a ballot, as block id and CoefTab of the record's plan.  No LDS, no private segment, vector
//       stores only.
//   gf_dread_kernel<VEC>   grid.x = R * wg_per_record, linear: workgroup b takes chunk b % wg_per_record of record
//       b / wg_per_record.  The record and its plan are uniform per workgroup and read through the constant address
//       space, so they sit in SGPRs.  A refused record has its state written by lane 0 of its first workgroup and
//       nothing else is read or written; a workgroup whose chunk lies past the record's end exits after those loads.
//       Chunks are cut on the SOURCE blocks' 16-byte grid: column c of a record is bytes [c0 + 16 c, c0 + 16 c + 16) of
//       the blocks, c0 = off & ~15, one lane per column.  Only a record's first and last column can be partial.
//         full column, VEC     the loop over the record's `reads` sources is uniform: aligned 16-byte loads in batches
//                              of four (check_device.hpp fold_inputs), gmul through the source's CoefTab, folded with
//                              xor3; one 16-byte store that has no alignment relative to out_off.
//         partial column, or   the in-range bytes only, one at a time with byte loads and byte stores: the bytes of a
//         any column, !VEC     neighbouring record's answer are never stored to.
// No atomics, no scalar stores; the answer buffer and the report see plain vector stores only.
#include <stddef.h>

#include "check_device.hpp"
#include "dread_kernels.hpp"
#include "launch_rule.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "dread_kernels.hip is gfx950 (CDNA4) code"
#endif

namespace ecg {

namespace {

static_assert(kMaxMT == 8, "a column of the row transform is eight bytes in one 64-bit word");
static_assert(kInlineSrc == 128, "a lane of the plan wave holds two columns of H");

typedef unsigned long long u64;
typedef u32x4 u32x4_unaligned __attribute__((aligned(1)));

// ---------------------------------------------------------------------------------------------
// The plan kernel

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

__global__ void __launch_bounds__(64) gf_dread_plan_kernel(const DreadLaunch a) {
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
    const uint8_t* f = a.lost + stripe * n;
    const bool in0 = lane < n, in1 = lane + 64 < n;
    const bool l0 = in0 && f[in0 ? lane : 0] != 0, l1 = in1 && f[in1 ? lane + 64 : 0] != 0;
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

// ---------------------------------------------------------------------------------------------
// The main kernel

template <bool VEC>
__global__ void __launch_bounds__(kThreads) gf_dread_kernel(const DreadLaunch a) {
    const long long wg = blockIdx.x;
    const long long r = wg / a.wg_per_record;
    const long long w = wg - r * a.wg_per_record;
    const ECG_CONST int* head = (const ECG_CONST int*)cst((const uint8_t*)a.work + r * a.plan_bytes);
    const unsigned state = (unsigned)head[0];
    const int reads = head[1];
    if (w == 0 && threadIdx.x == 0) {  // the call zeroed the report
        if (state != kDreadAnswered) a.report[2 * r] = state;
        else a.report[2 * r + 1] = (unsigned)reads;
    }
    if (state != kDreadAnswered) return;  // uniform: nothing of a refused record is read or written
    const ECG_CONST long long* rec = cst(a.records) + r * kDreadRecordWords;
    const long long stripe = rec[0], off = rec[2], len = rec[3], out_off = rec[4];
    const long long c0 = off & ~15LL, end = off + len;
    const long long ncols = len == 0 ? 0 : ((end + 15) >> 4) - (off >> 4);
    const long long w0 = w * a.cols_per_wg;
    if (w0 >= ncols) return;  // the chunk lies past the record's end
    const long long w1 = min(w0 + (long long)a.cols_per_wg, ncols);

    const ECG_CONST int* ids = head + kDreadHeadWords;
    const ECG_CONST CoefTab* T = (const ECG_CONST CoefTab*)(ids + dread_ids_words(a.n));
    const uint8_t* sbase = a.base + stripe * a.sstride;
    const long long bstride = a.bstride;
    auto src = [&](int j) { return sbase + (long long)ids[j] * bstride; };
    const long long shift = out_off - off;  // answer index of block byte x: shift + x
    for (long long c = w0 + threadIdx.x; c < w1; c += kThreads) {
        const long long x0 = c0 + (c << 4);
        const long long lo = max(x0, off), hi = min(x0 + 16, end);
        if (VEC && hi - lo == 16) {
            uint32_t acc[1][4] = {{0u, 0u, 0u, 0u}};
            fold_inputs<1, false>(reads, T, x0, acc, src);
            u32x4 o;
            o.x = acc[0][0], o.y = acc[0][1], o.z = acc[0][2], o.w = acc[0][3];
            *reinterpret_cast<u32x4_unaligned*>(a.out + (shift + x0)) = o;
        } else {
            for (long long x = lo; x < hi; ++x) {
                uint32_t v = 0u;
                for (int j = 0; j < reads; ++j) v ^= gmul(T[j], split((uint32_t)src(j)[x]));
                a.out[shift + x] = (uint8_t)(v & 0xffu);
            }
        }
    }
}

LaunchLog<kDreadLaunchFields> g_dread_log;

}  // namespace

void dread_traffic(long long* launches, long long* records) { g_dread_log.traffic(launches, records); }

int dread_last_launch(int* v, int cap) { return g_dread_log.last_launch(v, cap); }

bool dread_grid(long long max_len, long long R, int& cols_per_wg, int& wg_per_record) {
    const long long ncols = (max_len + 30) >> 4;  // a record of max_len bytes that starts at byte 15 of a column
    long long cpw = get_option(ECG_OPT_COLS_PER_WG);
    if (cpw <= 0) cpw = kThreads;
    if (ncols < cpw) cpw = ((ncols + kThreads - 1) / kThreads) * kThreads;
    if (cpw < kThreads) cpw = kThreads;
    cols_per_wg = (int)cpw;
    const long long wpr = (ncols + cpw - 1) / cpw;
    wg_per_record = (int)(wpr < 1 ? 1 : wpr);
    return R * (long long)wg_per_record <= 0x7fffffffLL;
}

hipError_t launch_dread(const DreadLaunch& base, bool vec_ok, int max_reads, hipStream_t st) {
    if (base.R < 1 || base.n < 1 || base.n > kInlineSrc || base.r < 1 || base.r > kMaxMT || base.S < 0 || base.B < 0 ||
        base.max_len < 0 || base.out_bytes < 0 || !base.base || !base.lost || !base.records || !base.out ||
        !base.work || !base.report)
        return hipErrorInvalidValue;
    DreadLaunch a = base;
    a.plan_bytes = dread_plan_bytes(a.n);
    if (!dread_grid(a.max_len, a.R, a.cols_per_wg, a.wg_per_record)) return hipErrorInvalidConfiguration;
    void* argv[] = {(void*)&a};
    if (const hipError_t e = hipLaunchKernel((const void*)gf_dread_plan_kernel, dim3((unsigned)a.R), dim3(64), argv, 0, st);
        e != hipSuccess)
        return e;
    g_dread_log.count(1, a.R);
    if (vec_ok && a.max_len > 0) g_dread_log.record({a.cols_per_wg, a.wg_per_record, a.R, max_reads});
    const void* kernel = vec_ok ? (const void*)gf_dread_kernel<true> : (const void*)gf_dread_kernel<false>;
    return launch_kernel(kernel, a, dim3((unsigned)((long long)a.R * a.wg_per_record)), st);
}

}  // namespace ecg
