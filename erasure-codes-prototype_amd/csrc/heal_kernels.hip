// In-place correction for MI355X (gfx950, CDNA4): XOR the error value back into the block that explains a bad
// position.
//
// If only block b is damaged at byte position x, by the error value e, every check row p sees s_p[x] = H[p][b] * e.
// The locate (locate_kernels.hip) stops at "block b explains x"; here the lane that holds x goes one step on:
//   e = s_p0[x] / H[p0][b]      (p0 = p0(b) the first row where column b is nonzero; one multiply by a 1 / H[p0][b] table)
// and byte x of block b becomes v_b[x] ^ e.  Per selected stripe (heal_kernels.hpp HealLaunch)
//   report[b] = #{ x corrected in block b },  report[n] = #{ x : s[x] != 0 },  report[n + 1] = #{ bad x left alone }.
//
// The syndrome phase is the locate's, line by line (shared pieces in gf_device.hpp): one lane per 16-byte column holds
// all R <= 8 syndromes, non-temporal dwordx4 loads, CoefTab tables in SGPRs, the same folds and load batches, the
// same workgroup -> chunk maps, for H = [C | I] only C through the tables with the stored blocks XORed in, and one
// ballot that sends a wave with all-zero syndromes on to its next column: clean data costs what the locate costs.
// A dirty wave column runs the candidate loop over [b0, b1): the one named block (TARGET) or every block (ANY), a
// bound that is uniform per workgroup.  The vote mask is the locate's; a lane whose mask is not empty computes e,
// masks it byte-wise (a 0x80 vote bit -> a 0xff byte: bytes of the column that block b does not explain stay), reloads
// its own 16 bytes of block b, XORs and stores them.  Lanes with an empty mask store nothing, so a byte is written
// only where it is corrected.  The n + 2 counters are the locate's three statically indexed registers, at most three
// atomic instructions per wave.  No LDS, no barrier; vector stores only.
//
// Workgroups own disjoint chunks of a stripe, lanes disjoint columns: as long as the launch's stripe ids are distinct
// no two lanes read-modify-write the same bytes.
#include <atomic>

#include "gf_device.hpp"
#include "heal_kernels.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "heal_kernels.hip is gfx950 (CDNA4) code"
#endif

namespace ecg {

namespace {

static_assert(kThreads % 64 == 0, "whole waves");
static_assert(kInlineSrc + 2 <= 3 * 64, "three counter registers per lane hold n + 2 counters");
constexpr int kSlots = 3;

// One bit (bit 7) per nonzero byte of a dword (locate_kernels.hip nonzero_mask).
__device__ __forceinline__ uint32_t nonzero_mask(uint32_t x) {
    const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
    return (t | x) & 0x80808080u;
}

// 0x80 bits -> 0xff bytes
__device__ __forceinline__ uint32_t byte_mask(uint32_t m) { return (m >> 7) * 0xffu; }

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// counter idx += tot, in the lane that owns it (idx and tot are uniform)
__device__ __forceinline__ void credit(unsigned (&mine)[kSlots], int idx, unsigned tot, int lane) {
    const unsigned add = lane == (idx & 63) ? tot : 0u;
    const int slot = idx >> 6;
#pragma unroll
    for (int j = 0; j < kSlots; ++j) mine[j] += slot == j ? add : 0u;
}

template <int MODE>
__device__ __forceinline__ const uint8_t* stripe_base(const GfLaunch& a, int s) {
    if constexpr (MODE == GF_MODE_INLINE) {
        return nullptr;
    } else {
        const long long st = a.stripe_of ? (long long)cst(a.stripe_of)[s] : (long long)s;
        return a.in_base + st * a.in_sstride;
    }
}

// column j of the table part
template <int MODE>
__device__ __forceinline__ const uint8_t* col_ptr(const GfLaunch& a, const uint8_t* sbase, int j) {
    if constexpr (MODE == GF_MODE_INLINE) return a.isrc[j];
    else return sbase + (long long)cst(a.src_ids)[j] * a.in_bstride;
}

// the stored block of check row q of H = [C | I] (LocateLaunch::ident)
template <int MODE>
__device__ __forceinline__ const uint8_t* ident_ptr(const LocateLaunch& sa, const uint8_t* sbase, int q) {
    if constexpr (MODE == GF_MODE_INLINE) return sa.g.isrc[sa.g.k + q];
    else return sbase + (long long)(sa.ident_base + q) * sa.g.in_bstride;
}

// Candidate b's block, to be written: a table column, or -- the last R candidates of an [C | I] check, which the
// tables do not hold -- the stored block of check row b - k.  b is uniform.
template <int MODE>
__device__ __forceinline__ uint8_t* block_ptr(const LocateLaunch& sa, const uint8_t* sbase, int b) {
    const uint8_t* p = b < sa.g.k ? col_ptr<MODE>(sa.g, sbase, b) : ident_ptr<MODE>(sa, sbase, b - sa.g.k);
    return const_cast<uint8_t*>(p);
}

// The stripe's candidate range [b0, b1): uniform per workgroup.
__device__ __forceinline__ void candidates(const HealLaunch& ha, int s, int& b0, int& b1) {
    b0 = 0;
    b1 = ha.l.n;
    if (ha.any) return;
    const int t = ha.targets ? cst(ha.targets)[s] : ha.target;
    const bool named = t >= 0 && t < ha.l.n;
    b0 = named ? t : 0;
    b1 = named ? t + 1 : 0;
}

// The candidate test over the R syndromes of W dwords (W = 4: the 16-byte column at byte `off` of every block;
// W = 1: the byte at `off`), and the correction.  Every lane of the wave is here (a lane past its chunk comes with
// zero syndromes, votes for nothing and stores nothing): the wave sums read every lane.
template <int R, int W, int MODE>
__device__ __forceinline__ void mend(const HealLaunch& ha, const uint8_t* sbase, const uint32_t (&syn)[R][W],
                                     long long off, int b0, int b1, int lane, unsigned (&mine)[kSlots]) {
    const LocateLaunch& sa = ha.l;
    const ECG_CONST CoefTab* Q = cst(sa.ratios);
    const ECG_CONST CoefTab* I = cst(ha.invlead);
    uint32_t bad[W], expl[W];
#pragma unroll
    for (int d = 0; d < W; ++d) {
        uint32_t any = syn[0][d];
#pragma unroll
        for (int p = 1; p < R; ++p) any |= syn[p][d];
        bad[d] = nonzero_mask(any);
        expl[d] = 0u;
    }
    for (int b = b0; b < b1; ++b) {  // uniform
        const unsigned p0 = (sa.p0[b >> 3] >> ((b & 7) * 4)) & 15u;
        if (p0 == kNoPivot) continue;  // a zero column explains nothing and is never corrected
        const ECG_CONST CoefTab* t = Q + (size_t)b * R;
        uint32_t vm[W], lead[W];
        unsigned v = 0u;
#pragma unroll
        for (int d = 0; d < W; ++d) {
            lead[d] = syn[0][d];
#pragma unroll
            for (int p = 1; p < R; ++p) lead[d] = p0 == (unsigned)p ? syn[p][d] : lead[d];
            const Split sp = split(lead[d]);
            uint32_t res = 0u;
#pragma unroll
            for (int q = 0; q < R; ++q) res |= syn[q][d] ^ gmul(t[q], sp);
            vm[d] = nonzero_mask(lead[d]) & ~nonzero_mask(res);
            v += (unsigned)__popc(vm[d]);
        }
        if (__ballot(v != 0u) == 0ull) continue;
#pragma unroll
        for (int d = 0; d < W; ++d) expl[d] |= vm[d];
        credit(mine, b, wave_sum(v), lane);
        if (v != 0u) {  // this lane holds a correction: e = s_p0 / H[p0][b] in the bytes that voted
            uint8_t* p = block_ptr<MODE>(sa, sbase, b) + off;
            if constexpr (W == 4) {
                u32x4 e;
                e.x = gmul(I[b], split(lead[0])) & byte_mask(vm[0]);
                e.y = gmul(I[b], split(lead[1])) & byte_mask(vm[1]);
                e.z = gmul(I[b], split(lead[2])) & byte_mask(vm[2]);
                e.w = gmul(I[b], split(lead[3])) & byte_mask(vm[3]);
                u32x4* q = reinterpret_cast<u32x4*>(p);
                *q = *q ^ e;
            } else {
                *p = (uint8_t)(*p ^ (gmul(I[b], split(lead[0])) & byte_mask(vm[0])));
            }
        }
    }
    unsigned nb = 0u, nu = 0u;
#pragma unroll
    for (int d = 0; d < W; ++d) {
        nb += (unsigned)__popc(bad[d]);
        nu += (unsigned)__popc(bad[d] & ~expl[d]);
    }
    credit(mine, sa.n, wave_sum(nb), lane);
    if (__ballot(nu != 0u) != 0ull) credit(mine, sa.n + 1, wave_sum(nu), lane);
}

// A wave's counters -> report[0, n + 2): one atomic instruction per register that holds a nonzero counter.
__device__ __forceinline__ void post_report(const unsigned (&mine)[kSlots], unsigned* out, int ncount, int lane) {
    if (__ballot((mine[0] | mine[1] | mine[2]) != 0u) == 0ull) return;
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
        const int idx = j * 64 + lane;
        if (idx < ncount && mine[j] != 0u) atomicAdd(out + idx, mine[j]);
    }
}

// Vector path: bytes [0, 16 * floor(B / 16)) of every block; all pointers 16-byte aligned.
// grid.x = S * wg_per_stripe (stripe-major).  The column loop is per wave, so that every lane reaches the wave sums.
template <int R, int MODE>
__global__ void __launch_bounds__(kThreads, occupancy_for(R)) gf_heal_kernel(const HealLaunch ha) {
    const LocateLaunch& sa = ha.l;
    const GfLaunch& a = sa.g;
    int s, w;
    wg_coords(a, s, w);
    const int k = a.k;
    const ECG_CONST CoefTab* T = cst(a.tabs);
    const uint8_t* sbase = stripe_base<MODE>(a, s);
    int b0, b1;
    candidates(ha, s, b0, b1);
    const long long ncols = a.B >> 4;  // < 2^27: B < 2^31
    const long long w0 = (long long)w * a.cols_per_wg;
    const int c0 = (int)w0, c1 = (int)min(w0 + (long long)a.cols_per_wg, ncols);
    const int lane = threadIdx.x & 63;

    unsigned mine[kSlots] = {0u, 0u, 0u};

    for (int cw = c0 + (int)(threadIdx.x & ~63u); cw < c1; cw += kThreads) {
        const int c = cw + lane;
        const long long off = (long long)c << 4;
        uint32_t acc[R][4];
#pragma unroll
        for (int p = 0; p < R; ++p)
#pragma unroll
            for (int d = 0; d < 4; ++d) acc[p][d] = 0u;

        if (c < c1) {
            int j = 0;
            constexpr int LB = R >= 5 ? kGenWideLB : kGenLB;
            for (; j + LB <= k; j += LB) {
                uint32_t x[LB][4];
#pragma unroll
                for (int u = 0; u < LB; ++u) load16<1>(col_ptr<MODE>(a, sbase, j + u) + off, x[u]);
                fold<R, LB, false>(x, T + (size_t)j * R, acc);
            }
            if constexpr (LB > 4) {  // the rest of k: four, two, one
                if (j + 4 <= k) {
                    uint32_t x[4][4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) load16<1>(col_ptr<MODE>(a, sbase, j + u) + off, x[u]);
                    fold<R, 4, false>(x, T + (size_t)j * R, acc);
                    j += 4;
                }
            }
            if constexpr (LB > 2) {
                if (j + 2 <= k) {
                    uint32_t x[2][4];
#pragma unroll
                    for (int u = 0; u < 2; ++u) load16<1>(col_ptr<MODE>(a, sbase, j + u) + off, x[u]);
                    fold<R, 2, false>(x, T + (size_t)j * R, acc);
                    j += 2;
                }
            }
            if (j < k) {
                uint32_t x[1][4];
                load16<1>(col_ptr<MODE>(a, sbase, j) + off, x[0]);
                fold<R, 1, false>(x, T + (size_t)j * R, acc);
            }
            if (sa.ident) {  // uniform.  acc[p] ^= the block row p checks
                constexpr int IB = R < 4 ? R : 4;  // loads in flight, as a load batch
#pragma unroll
                for (int q0 = 0; q0 < R; q0 += IB) {
                    uint32_t x[IB][4];
#pragma unroll
                    for (int u = 0; u < IB; ++u)
                        if (q0 + u < R) load16<1>(ident_ptr<MODE>(sa, sbase, q0 + u) + off, x[u]);
#pragma unroll
                    for (int u = 0; u < IB; ++u)
                        if (q0 + u < R) {
#pragma unroll
                            for (int d = 0; d < 4; ++d) acc[q0 + u][d] ^= x[u][d];
                        }
                }
            }
        }
        uint32_t any = 0u;
#pragma unroll
        for (int p = 0; p < R; ++p)
#pragma unroll
            for (int d = 0; d < 4; ++d) any |= acc[p][d];
        if (__ballot(any != 0u) == 0ull) continue;  // a clean wave column: the locate's cost, nothing more
        mend<R, 4, MODE>(ha, sbase, acc, off, b0, b1, lane, mine);
    }
    post_report(mine, sa.votes + (size_t)s * (size_t)(sa.n + 2), sa.n + 2, lane);
}

// Byte path: bytes [off0, B) (tails, unaligned blocks).  cols_per_wg = bytes per workgroup.
template <int R, int MODE>
__global__ void __launch_bounds__(kThreads) gf_heal_byte_kernel(const HealLaunch ha) {
    const LocateLaunch& sa = ha.l;
    const GfLaunch& a = sa.g;
    int s, w;
    wg_coords(a, s, w);
    const int k = a.k;
    const ECG_CONST CoefTab* T = cst(a.tabs);
    const long long by0 = a.off0 + (long long)w * a.cols_per_wg;
    const long long by1 = min(by0 + (long long)a.cols_per_wg, a.B);
    const uint8_t* sbase = stripe_base<MODE>(a, s);
    int b0, b1;
    candidates(ha, s, b0, b1);
    const int lane = threadIdx.x & 63;
    unsigned mine[kSlots] = {0u, 0u, 0u};
    for (long long ow = by0 + (threadIdx.x & ~63); ow < by1; ow += kThreads) {
        const long long o = ow + lane;
        uint32_t acc[R][1];
#pragma unroll
        for (int p = 0; p < R; ++p) acc[p][0] = 0u;
        if (o < by1) {
            for (int j = 0; j < k; ++j) {
                const Split sp = split((uint32_t)col_ptr<MODE>(a, sbase, j)[o]);
                const ECG_CONST CoefTab* t = T + (size_t)j * R;
#pragma unroll
                for (int p = 0; p < R; ++p) acc[p][0] ^= gmul(t[p], sp);
            }
            if (sa.ident) {
#pragma unroll
                for (int p = 0; p < R; ++p) acc[p][0] ^= ident_ptr<MODE>(sa, sbase, p)[o];
            }
        }
        uint32_t any = 0u;
#pragma unroll
        for (int p = 0; p < R; ++p) any |= acc[p][0];
        if (__ballot(any != 0u) == 0ull) continue;
        mend<R, 1, MODE>(ha, sbase, acc, o, b0, b1, lane, mine);
    }
    post_report(mine, sa.votes + (size_t)s * (size_t)(sa.n + 2), sa.n + 2, lane);
}

// ---------------------------------------------------------------------------------------------
// Dispatch

using Launcher = hipError_t (*)(const HealLaunch&, dim3, hipStream_t);

template <int R, int MODE, bool BYTE>
hipError_t launch_one(const HealLaunch& a, dim3 g, hipStream_t st) {
    void* argv[] = {(void*)&a};
    if constexpr (BYTE)
        return hipLaunchKernel((const void*)gf_heal_byte_kernel<R, MODE>, g, dim3(kThreads), argv, 0, st);
    else
        return hipLaunchKernel((const void*)gf_heal_kernel<R, MODE>, g, dim3(kThreads), argv, 0, st);
}

template <int MODE, bool BYTE>
Launcher pick_r(int R) {
    switch (R) {
        case 1: return launch_one<1, MODE, BYTE>;
        case 2: return launch_one<2, MODE, BYTE>;
        case 3: return launch_one<3, MODE, BYTE>;
        case 4: return launch_one<4, MODE, BYTE>;
        case 5: return launch_one<5, MODE, BYTE>;
        case 6: return launch_one<6, MODE, BYTE>;
        case 7: return launch_one<7, MODE, BYTE>;
        case 8: return launch_one<8, MODE, BYTE>;
        default: return nullptr;
    }
}

template <bool BYTE>
Launcher pick(int R, int mode) {
    if (mode == GF_MODE_INLINE) return pick_r<GF_MODE_INLINE, BYTE>(R);
    if (mode == GF_MODE_STRIDED) return pick_r<GF_MODE_STRIDED, BYTE>(R);
    return nullptr;
}

std::atomic<long long> g_heal_launched{0}, g_heal_read{0};
// geometry of the most recent vector-path launch (heal_kernels.hpp kHealLaunchFields), all zero before the first
std::atomic<int> g_heal_last[kHealLaunchFields];

}  // namespace

void heal_traffic(long long* launches, long long* bytes) {
    if (launches) *launches = g_heal_launched.load(std::memory_order_relaxed);
    if (bytes) *bytes = g_heal_read.load(std::memory_order_relaxed);
}

int heal_last_launch(int* v, int cap) {
    if (v && cap >= kHealLaunchFields)
        for (int i = 0; i < kHealLaunchFields; ++i) v[i] = g_heal_last[i].load(std::memory_order_relaxed);
    return kHealLaunchFields;
}

hipError_t launch_heal(const HealLaunch& base, int mode, bool vec_ok, hipStream_t st) {
    const LocateLaunch& bl = base.l;
    const GfLaunch& b = bl.g;
    if (b.k < 1 || b.m < 1 || b.m > kMaxMT || b.MT != b.m || b.rtiles != 1 || b.S < 1 || b.B < 0 || bl.n < 1 ||
        bl.n > kInlineSrc || bl.n != b.k + (bl.ident ? b.m : 0) || !bl.votes || !bl.ratios || !base.invlead || !b.tabs)
        return hipErrorInvalidValue;
    if (mode != GF_MODE_INLINE && mode != GF_MODE_STRIDED) return hipErrorInvalidValue;
    if (mode == GF_MODE_INLINE && (b.S != 1 || base.targets)) return hipErrorInvalidValue;
    if (mode == GF_MODE_STRIDED && !base.any && !base.targets) return hipErrorInvalidValue;
    if (b.B == 0) return hipSuccess;
    HealLaunch ha = base;
    GfLaunch& a = ha.l.g;
    a.row_split = 0;
    a.prog_of_stripe = nullptr;
    const long long vec_bytes = vec_ok ? (a.B & ~15LL) : 0;
    g_heal_launched.fetch_add((vec_bytes > 0) + (vec_bytes < a.B), std::memory_order_relaxed);
    g_heal_read.fetch_add((long long)a.S * a.B * bl.n, std::memory_order_relaxed);
    if (vec_bytes > 0) {
        const long long ncols = vec_bytes >> 4;
        long long cpw = get_option(ECG_OPT_COLS_PER_WG);
        if (cpw <= 0) cpw = kThreads;  // 2 KiB of every block per workgroup, as the product, the scrub and the locate
        if (ncols < cpw) cpw = ((ncols + kThreads - 1) / kThreads) * kThreads;
        a.cols_per_wg = (int)cpw;
        a.wg_per_stripe = (int)((ncols + cpw - 1) / cpw);
        a.off0 = 0;
        const long long gx = (long long)a.S * a.wg_per_stripe;
        if (gx > 0x7fffffffLL) return hipErrorInvalidConfiguration;
        // The scrub's rule (scrub_kernels.hip launch_scrub): XCD-contiguous chunks, ECG_OPT_GRID_MAP 0 / 2 honoured.
        long long gm = get_option(ECG_OPT_GRID_MAP);
        if (gm == 3) gm = 1;
        long long G = get_option(ECG_OPT_MAP_GROUP);
        while (G > 1 && a.S % (8 * G) != 0) G >>= 1;
        if (gm == 2 && a.S % (8 * G) != 0) gm = 1;
        a.grid_map = (gm == 1 && gx % 8 == 0) ? 1 : (gm == 2) ? 2 : 0;
        a.map_group = (int)G;
        const int geo[kHealLaunchFields] = {a.grid_map, a.map_group, a.cols_per_wg, a.wg_per_stripe, a.S, a.rtiles};
        for (int i = 0; i < kHealLaunchFields; ++i) g_heal_last[i].store(geo[i], std::memory_order_relaxed);
        Launcher l = pick<false>(a.m, mode);
        if (!l) return hipErrorInvalidValue;
        const hipError_t e = l(ha, dim3((unsigned)gx), st);
        if (e != hipSuccess) return e;
    }
    if (vec_bytes < a.B) {
        const long long nbytes = a.B - vec_bytes;
        long long bpw = 16LL * kThreads;
        if (nbytes < bpw) bpw = ((nbytes + kThreads - 1) / kThreads) * kThreads;
        a.cols_per_wg = (int)bpw;
        a.wg_per_stripe = (int)((nbytes + bpw - 1) / bpw);
        a.off0 = vec_bytes;
        a.grid_map = 0;
        const long long gx = (long long)a.S * a.wg_per_stripe;
        if (gx > 0x7fffffffLL) return hipErrorInvalidConfiguration;
        Launcher l = pick<true>(a.m, mode);
        if (!l) return hipErrorInvalidValue;
        const hipError_t e = l(ha, dim3((unsigned)gx), st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace ecg
