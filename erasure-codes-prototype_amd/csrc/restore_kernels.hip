// Named-block restoration for MI355X (gfx950, CDNA4): rebuild up to r flagged blocks of a stripe in place, from the
// syndromes.
//
// The heal (heal_kernels.hip) takes one named block per stripe: e = s_p0 / H[p0][b].  Here a stripe names a set E of
// t <= r blocks, and a bad position is the linear system H_E * e = s.  Three kernels:
//
//   gf_restore_plan_kernel   one wave per selected stripe, before the main launch on the same stream.  It gathers the
//       flagged columns, runs Gauss-Jordan on H_E with row pivoting -- the r x 8 matrix and the r x r row transform as
//       one packed 64-bit word per row, every index static, all of it in registers and the same in every lane -- and
//       then lane L < r r writes coefficient A[L] of the plan (restore_kernels.hpp) as a CoefTab, lanes 0..23 the
//       header.  H sits in the kernel arguments.  No LDS, no private segment, vector stores only.
//   gf_restore_kernel, gf_restore_byte_kernel   the heal's two kernels with another dirty path.  The syndrome phase is
//       the locate's (check_device.hpp syndromes16, syndrome_byte), and one ballot sends a wave with all-zero
//       syndromes on to its next column: clean data costs what the locate costs.  A dirty wave column reads its
//       stripe's plan through uniform loads (STRIDED: the constant address space; INLINE: the kernel arguments) and
//       folds its r syndromes through the r x r set A, as the syndrome phase folds r inputs: outputs i < t are e of
//       flagged block ids[i], outputs i >= t the residual, whose nonzero bytes are the positions the flagged blocks
//       cannot explain.  Then a loop of t <= 8 trips, uniform per workgroup: the bytes of e_i that are nonzero and
//       consistent are counted for block ids[i], and a lane that holds one reloads its 16 bytes of the block, XORs
//       and stores them.  Lanes with an empty mask store nothing.  The n + 3 counters are the locate's three
//       statically indexed registers; wave 0 of a stripe's first workgroup adds the state.
//   gf_restore_names_kernel  sums != expected -> flags, one lane per piece row.
//
// Workgroups own disjoint chunks of a stripe, lanes disjoint columns: as long as the launch's stripe ids are distinct
// no two lanes read-modify-write the same bytes.
#include <stddef.h>

#include "check_device.hpp"
#include "launch_rule.hpp"
#include "restore_kernels.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "restore_kernels.hip is gfx950 (CDNA4) code"
#endif

namespace ecg {

namespace {

static_assert(kInlineSrc + 3 <= kSlots * 64, "three counter registers per lane hold n + 3 counters");
static_assert(kMaxMT == 8, "a row of the elimination is eight bytes in one 64-bit word");

// ---------------------------------------------------------------------------------------------
// The plan kernel

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

// bytes [0, a, b, a ^ b]: c * e for e = 0..3 from c * 1 and c * 2
__device__ __forceinline__ uint32_t quad(unsigned a, unsigned b) { return (a << 8) | (b << 16) | ((a ^ b) << 24); }

__global__ void __launch_bounds__(64) gf_restore_plan_kernel(const RestorePlanLaunch pa) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int n = pa.n, r = pa.r;
    const uint8_t* f = pa.named + (size_t)s * (size_t)n;
    u64 m0 = __ballot(lane < n && f[lane] != 0);
    u64 m1 = __ballot(lane + 64 < n && f[lane + 64] != 0);
    const int t = __popcll(m0) + __popcll(m1);
    int ids[kMaxMT];
#pragma unroll
    for (int c = 0; c < kMaxMT; ++c) {
        int id = -1;
        if (m0) {
            id = __ffsll(m0) - 1;
            m0 &= m0 - 1;
        } else if (m1) {
            id = 64 + __ffsll(m1) - 1;
            m1 &= m1 - 1;
        }
        ids[c] = id;
    }
    int state = t == 0 ? kRestoreNone : t > r ? kRestoreTooMany : kRestoreUsable;
    // a[q]: row q of H_E, byte c = H[q][ids[c]]; T[q]: row q of the row transform, the identity to begin with
    u64 a[kMaxMT], T[kMaxMT];
#pragma unroll
    for (int q = 0; q < kMaxMT; ++q) {
        a[q] = 0;
        T[q] = 1ULL << (8 * q);
#pragma unroll
        for (int c = 0; c < kMaxMT; ++c)
            if (state == kRestoreUsable && q < r && c < t) a[q] |= (u64)pa.H[q * n + ids[c]] << (8 * c);
    }
    unsigned used = 0u;
    int rows[kMaxMT];
#pragma unroll
    for (int c = 0; c < kMaxMT; ++c) rows[c] = -1;
#pragma unroll
    for (int c = 0; c < kMaxMT; ++c) {
        if (state != kRestoreUsable || c >= t) continue;
        int p = -1;  // the first row that was no pivot yet and is nonzero in column c (rows >= r are zero)
#pragma unroll
        for (int q = 0; q < kMaxMT; ++q)
            if (p < 0 && !((used >> q) & 1u) && byte_of(a[q], c) != 0u) p = q;
        if (p < 0) {
            state = kRestoreDependent;
            continue;
        }
        used |= 1u << p;
        rows[c] = p;
        u64 ar = 0, tr = 0;
#pragma unroll
        for (int q = 0; q < kMaxMT; ++q) {
            ar = q == p ? a[q] : ar;
            tr = q == p ? T[q] : tr;
        }
        const unsigned iv = inv8(byte_of(ar, c));
        ar = mul8(ar, iv);
        tr = mul8(tr, iv);
#pragma unroll
        for (int q = 0; q < kMaxMT; ++q) {
            const unsigned fq = byte_of(a[q], c);
            a[q] = q == p ? ar : a[q] ^ mul8(ar, fq);
            T[q] = q == p ? tr : T[q] ^ mul8(tr, fq);
        }
    }
    if (state == kRestoreUsable) {  // the residual rows after the pivot rows, in ascending order
        int w = t;
#pragma unroll
        for (int q = 0; q < kMaxMT; ++q) {
            if (q >= r || ((used >> q) & 1u)) continue;
#pragma unroll
            for (int i = 0; i < kMaxMT; ++i) rows[i] = i == w ? q : rows[i];
            ++w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < kMaxMT; ++c) rows[c] = -1;
    }
    RestorePlan* out = pa.plans + s;
    if (lane < kRestorePlanWords) {  // the header: state, t, ids, rows, padding
        int v = lane == 0 ? state : lane == 1 ? t : 0;
#pragma unroll
        for (int c = 0; c < kMaxMT; ++c) {
            v = lane == 2 + c ? ids[c] : v;
            v = lane == 2 + kMaxMT + c ? rows[c] : v;
        }
        reinterpret_cast<int*>(out)[lane] = v;
    }
    if (lane < r * r) {  // A[p * r + i] = T[rows[i]][p]
        const int p = lane / r, i = lane - p * r;
        int ri = -1;
#pragma unroll
        for (int c = 0; c < kMaxMT; ++c) ri = c == i ? rows[c] : ri;
        u64 tr = 0;
#pragma unroll
        for (int q = 0; q < kMaxMT; ++q) tr = q == ri ? T[q] : tr;
        const unsigned c1 = state == kRestoreUsable ? byte_of(tr, p) : 0u;
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
        u32x4* tab = reinterpret_cast<u32x4*>(&out->A[lane]);
        tab[0] = lo;
        tab[1] = hi;
    }
}

// ---------------------------------------------------------------------------------------------
// The main kernels

// The stripe's plan, a uniform pointer into the constant address space.  STRIDED: the plan kernel's record.  INLINE:
// the descriptor is the kernel's only argument, so its `inl` lies at a fixed offset of the kernel-argument segment;
// read there, not through the by-value copy, every table load is a scalar load whatever the size of the kernel.
template <int MODE>
__device__ __forceinline__ const ECG_CONST RestorePlan* plan_of(const RestoreLaunch& ra, int s) {
    if constexpr (MODE == GF_MODE_INLINE) {
        const ECG_CONST char* args = (const ECG_CONST char*)__builtin_amdgcn_kernarg_segment_ptr();
        return (const ECG_CONST RestorePlan*)(args + offsetof(RestoreLaunch, inl));
    } else {
        return cst(ra.plans) + s;
    }
}

// The dirty path at byte `off` of every block (W = 4: the 16-byte column there; W = 1: the byte).  Every lane of the
// wave is here (a lane past its chunk comes with zero syndromes, solves to zero and stores nothing): the wave sums
// read every lane.
template <int R, int W, int MODE>
__device__ __forceinline__ void mend(const RestoreLaunch& ra, const uint8_t* sbase, const uint32_t (&syn)[R][W],
                                     long long off, const ECG_CONST RestorePlan* pl, int lane,
                                     unsigned (&mine)[kSlots]) {
    const LocateLaunch& sa = ra.l;
    uint32_t bad[W], ok[W];
    unsigned nb = 0u;
#pragma unroll
    for (int d = 0; d < W; ++d) {
        uint32_t any = syn[0][d];
#pragma unroll
        for (int p = 1; p < R; ++p) any |= syn[p][d];
        bad[d] = nonzero_mask(any);
        nb += (unsigned)__popc(bad[d]);
    }
    const unsigned bad_total = wave_sum(nb);
    credit(mine, sa.n, bad_total, lane);
    if (pl->state != kRestoreUsable) {  // uniform: read and counted, never written
        credit(mine, sa.n + 1, bad_total, lane);
        return;
    }
    const int t = pl->t;
    uint32_t out[R][W];  // A * s: e of the flagged blocks, then the residual
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int d = 0; d < W; ++d) out[i][d] = 0u;
#pragma unroll
    for (int p = 0; p < R; ++p)
#pragma unroll
        for (int d = 0; d < W; ++d) {
            const Split sp = split(syn[p][d]);
#pragma unroll
            for (int i = 0; i < R; ++i) out[i][d] ^= gmul(pl->A[p * R + i], sp);
        }
    unsigned nu = 0u;
#pragma unroll
    for (int d = 0; d < W; ++d) {
        uint32_t res = 0u;
#pragma unroll
        for (int i = 0; i < R; ++i) res |= i >= t ? out[i][d] : 0u;
        ok[d] = bad[d] & ~nonzero_mask(res);
        nu += (unsigned)__popc(bad[d] & ~ok[d]);
    }
    if (__ballot(nu != 0u) != 0ull) credit(mine, sa.n + 1, wave_sum(nu), lane);
#pragma unroll
    for (int i = 0; i < R; ++i) {
        if (i >= t) continue;  // uniform
        uint32_t vm[W];
        unsigned v = 0u;
#pragma unroll
        for (int d = 0; d < W; ++d) {
            vm[d] = nonzero_mask(out[i][d]) & ok[d];
            v += (unsigned)__popc(vm[d]);
        }
        if (__ballot(v != 0u) == 0ull) continue;  // a flagged block that is not damaged here
        const int b = pl->ids[i];
        credit(mine, b, wave_sum(v), lane);
        if (v == 0u) continue;
        uint8_t* q = block_ptr<MODE>(sa, sbase, b) + off;
        if constexpr (W == 4) {
            u32x4 e;
            e.x = out[i][0] & byte_mask(vm[0]);
            e.y = out[i][1] & byte_mask(vm[1]);
            e.z = out[i][2] & byte_mask(vm[2]);
            e.w = out[i][3] & byte_mask(vm[3]);
            u32x4* qq = reinterpret_cast<u32x4*>(q);
            *qq = *qq ^ e;
        } else {
            *q = (uint8_t)(*q ^ (out[i][0] & byte_mask(vm[0])));
        }
    }
}

// The state of the stripe, once: wave 0 of the stripe's first workgroup in the call's first launch.
__device__ __forceinline__ void post_state(const RestoreLaunch& ra, int w, const ECG_CONST RestorePlan* pl, int lane,
                                           unsigned (&mine)[kSlots]) {
    if (ra.post_state && w == 0 && threadIdx.x < 64) credit(mine, ra.l.n + 2, (unsigned)pl->state, lane);
}

// Vector path: bytes [0, 16 * floor(B / 16)) of every block; all pointers 16-byte aligned.
// grid.x = S * wg_per_stripe (stripe-major).  The column loop is per wave, so that every lane reaches the wave sums.
template <int R, int MODE>
__global__ void __launch_bounds__(kThreads, occupancy_for(R)) gf_restore_kernel(const RestoreLaunch ra) {
    const LocateLaunch& sa = ra.l;
    const GfLaunch& a = sa.g;
    int s, w;
    wg_coords(a, s, w);
    const uint8_t* sbase = stripe_base<MODE>(a, s);
    const ECG_CONST RestorePlan* pl = plan_of<MODE>(ra, s);
    const long long ncols = a.B >> 4;  // < 2^27: B < 2^31
    const long long w0 = (long long)w * a.cols_per_wg;
    const int c0 = (int)w0, c1 = (int)min(w0 + (long long)a.cols_per_wg, ncols);
    const int lane = threadIdx.x & 63;
    unsigned mine[kSlots] = {0u, 0u, 0u};
    post_state(ra, w, pl, lane, mine);
    for (int cw = c0 + (int)(threadIdx.x & ~63u); cw < c1; cw += kThreads) {
        const int c = cw + lane;
        const long long off = (long long)c << 4;
        uint32_t acc[R][4];  // zeroed in place, as the locate's
#pragma unroll
        for (int p = 0; p < R; ++p)
#pragma unroll
            for (int d = 0; d < 4; ++d) acc[p][d] = 0u;
        if (c < c1) syndromes16<R, MODE>(sa, sbase, off, acc);
        if (clean_wave(acc)) continue;  // a clean wave column: the locate's cost, nothing more
        mend<R, 4, MODE>(ra, sbase, acc, off, pl, lane, mine);
    }
    post_counters(mine, sa.votes + (size_t)s * (size_t)(sa.n + 3), sa.n + 3, lane);
}

// Byte path: bytes [off0, B) (tails, unaligned blocks).  cols_per_wg = bytes per workgroup.
template <int R, int MODE>
__global__ void __launch_bounds__(kThreads) gf_restore_byte_kernel(const RestoreLaunch ra) {
    const LocateLaunch& sa = ra.l;
    const GfLaunch& a = sa.g;
    int s, w;
    wg_coords(a, s, w);
    const long long by0 = a.off0 + (long long)w * a.cols_per_wg;
    const long long by1 = min(by0 + (long long)a.cols_per_wg, a.B);
    const uint8_t* sbase = stripe_base<MODE>(a, s);
    const ECG_CONST RestorePlan* pl = plan_of<MODE>(ra, s);
    const int lane = threadIdx.x & 63;
    unsigned mine[kSlots] = {0u, 0u, 0u};
    post_state(ra, w, pl, lane, mine);
    for (long long ow = by0 + (threadIdx.x & ~63); ow < by1; ow += kThreads) {
        const long long o = ow + lane;
        uint32_t acc[R][1] = {};
        if (o < by1) syndrome_byte<R, MODE>(sa, sbase, o, acc);
        if (clean_wave(acc)) continue;
        mend<R, 1, MODE>(ra, sbase, acc, o, pl, lane, mine);
    }
    post_counters(mine, sa.votes + (size_t)s * (size_t)(sa.n + 3), sa.n + 3, lane);
}

// ---------------------------------------------------------------------------------------------
// The bridge from a verify: one lane per piece row (i, q).

__global__ void __launch_bounds__(256) gf_restore_names_kernel(int n, int Q, long long rows, const unsigned* sums,
                                                               const unsigned* expected, uint8_t* named, int* count) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const long long i = row / Q, q = row - i * Q;
    const size_t in = (size_t)i * (size_t)n * (size_t)Q + (size_t)q;
    uint8_t* f = named + (size_t)row * (size_t)n;
    int c = 0;
    for (int j = 0; j < n; ++j) {
        const bool differs = sums[in + (size_t)j * (size_t)Q] != expected[in + (size_t)j * (size_t)Q];
        f[j] = differs ? 1 : 0;
        c += differs ? 1 : 0;
    }
    count[row] = c;
}

// ---------------------------------------------------------------------------------------------
// Dispatch

struct RestoreKernels {  // launch_rule.hpp candidate_kernel
    template <int R, int MODE, bool BYTE>
    static const void* kernel() {
        if constexpr (BYTE) return (const void*)gf_restore_byte_kernel<R, MODE>;
        else return (const void*)gf_restore_kernel<R, MODE>;
    }
};

CheckLaunchLog g_restore_log;

}  // namespace

void restore_traffic(long long* launches, long long* bytes) { g_restore_log.traffic(launches, bytes); }

int restore_last_launch(int* v, int cap) { return g_restore_log.last_launch(v, cap); }

hipError_t launch_restore_plan(const RestorePlanLaunch& p, hipStream_t st) {
    if (p.n < 1 || p.n > kInlineSrc || p.r < 1 || p.r > kMaxMT || p.S < 0 || !p.named || !p.plans)
        return hipErrorInvalidValue;
    if (p.S == 0) return hipSuccess;
    void* argv[] = {(void*)&p};
    return hipLaunchKernel((const void*)gf_restore_plan_kernel, dim3((unsigned)p.S), dim3(64), argv, 0, st);
}

hipError_t launch_restore_names(int n, int Q, const unsigned* sums, const unsigned* expected, int S, uint8_t* named,
                                int* count, hipStream_t st) {
    if (n < 1 || Q < 0 || S < 0 || !sums || !expected || !named || !count) return hipErrorInvalidValue;
    long long rows = (long long)S * Q;
    if (rows == 0) return hipSuccess;
    const long long gx = (rows + 255) / 256;
    if (gx > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    void* argv[] = {(void*)&n, (void*)&Q, (void*)&rows, (void*)&sums, (void*)&expected, (void*)&named, (void*)&count};
    return hipLaunchKernel((const void*)gf_restore_names_kernel, dim3((unsigned)gx), dim3(256), argv, 0, st);
}

hipError_t launch_restore(const RestoreLaunch& base, int mode, bool vec_ok, hipStream_t st) {
    const LocateLaunch& bl = base.l;
    const GfLaunch& b = bl.g;
    if (b.k < 1 || b.m < 1 || b.m > kMaxMT || b.MT != b.m || b.rtiles != 1 || b.S < 1 || b.B < 0 || bl.n < 1 ||
        bl.n > kInlineSrc || bl.n != b.k + (bl.ident ? b.m : 0) || !bl.votes || !b.tabs)
        return hipErrorInvalidValue;
    if (mode != GF_MODE_INLINE && mode != GF_MODE_STRIDED) return hipErrorInvalidValue;
    if (mode == GF_MODE_INLINE && b.S != 1) return hipErrorInvalidValue;
    if (mode == GF_MODE_STRIDED && !base.plans) return hipErrorInvalidValue;
    if (b.B == 0) return hipSuccess;
    RestoreLaunch ra = base;
    GfLaunch& a = ra.l.g;
    a.row_split = 0;
    a.prog_of_stripe = nullptr;
    ra.post_state = 1;
    auto launch = [&](const void* kernel, dim3 g) {
        const hipError_t e = launch_kernel(kernel, ra, g, st);
        ra.post_state = 0;  // the call's first launch has taken the state
        return e;
    };
    return launch_paths(
        a, vec_ok, g_restore_log, (long long)a.S * a.B * bl.n, 1,
        [&](dim3 g) { return launch(candidate_kernel<RestoreKernels, 1, false>(a.m, mode), g); },
        [&](dim3 g) { return launch(candidate_kernel<RestoreKernels, 1, true>(a.m, mode), g); });
}

}  // namespace ecg
