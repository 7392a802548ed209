// In-place correction for MI355X (gfx950, CDNA4): XOR the error value back into the block that explains a bad
// position.
//
// If only block b is damaged at byte position x, by the error value e, every check row p sees s_p[x] = H[p][b] * e.
// The locate (locate_kernels.hip) stops at "block b explains x"; here the lane that holds x goes one step on:
//   e = s_p0[x] / H[p0][b]      (p0 = p0(b) the first row where column b is nonzero; one multiply by a 1 / H[p0][b] table)
// and byte x of block b becomes v_b[x] ^ e.  Per selected stripe (heal_kernels.hpp HealLaunch)
//   report[b] = #{ x corrected in block b },  report[n] = #{ x : s[x] != 0 },  report[n + 1] = #{ bad x left alone }.
//
// The syndrome phase is the locate's, the same code (check_device.hpp syndromes16, syndrome_byte): one lane per
// 16-byte column holds all R <= 8 syndromes, non-temporal dwordx4 loads, CoefTab tables in SGPRs, the same folds and
// load batches, the same workgroup -> chunk maps, for H = [C | I] only C through the tables with the stored blocks
// XORed in, and one ballot that sends a wave with all-zero syndromes on to its next column: clean data costs what the
// locate costs.  A dirty wave column runs the locate's candidate loop (check_device.hpp candidate_loop) over [b0, b1):
// the one named block (TARGET) or every block (ANY), a bound that is uniform per workgroup.  A lane whose vote mask is
// not empty computes e, masks it byte-wise (a 0x80 vote bit -> a 0xff byte: bytes of the column that block b does not
// explain stay), reloads its own 16 bytes of block b, XORs and stores them.  Lanes with an empty mask store nothing, so
// a byte is written only where it is corrected.  The n + 2 counters are the locate's three statically indexed
// registers, at most three atomic instructions per wave.  No LDS, no barrier; vector stores only.
//
// Workgroups own disjoint chunks of a stripe, lanes disjoint columns: as long as the launch's stripe ids are distinct
// no two lanes read-modify-write the same bytes.
#include "check_device.hpp"
#include "launch_rule.hpp"
#include "heal_kernels.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "heal_kernels.hip is gfx950 (CDNA4) code"
#endif

namespace ecg {

namespace {

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

// The candidate test over [b0, b1) and the correction of what it finds, at byte `off` of every block (W = 4: the
// 16-byte column there; W = 1: the byte).  A lane that votes for block b holds a correction: e = s_p0 / H[p0][b] in the
// bytes that voted.  A lane past its chunk comes with zero syndromes, votes for nothing and stores nothing.
template <int R, int W, int MODE>
__device__ __forceinline__ void mend(const HealLaunch& ha, const uint8_t* sbase, const uint32_t (&syn)[R][W],
                                     long long off, int b0, int b1, int lane, unsigned (&mine)[kSlots]) {
    const ECG_CONST CoefTab* I = cst(ha.invlead);
    candidate_loop<R, W>(ha.l, syn, b0, b1, lane, mine, [&](int b, const uint32_t (&lead)[W], const uint32_t (&vm)[W]) {
        uint8_t* p = block_ptr<MODE>(ha.l, sbase, b) + off;
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
    });
}

// Vector path: bytes [0, 16 * floor(B / 16)) of every block; all pointers 16-byte aligned.
// grid.x = S * wg_per_stripe (stripe-major).  The column loop is per wave, so that every lane reaches the wave sums.
template <int R, int MODE>
__global__ void __launch_bounds__(kThreads, occupancy_for(R)) gf_heal_kernel(const HealLaunch ha) {
    const LocateLaunch& sa = ha.l;
    const GfLaunch& a = sa.g;
    int s, w;
    wg_coords(a, s, w);
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
        uint32_t acc[R][4];  // zeroed in place, as the locate's
#pragma unroll
        for (int p = 0; p < R; ++p)
#pragma unroll
            for (int d = 0; d < 4; ++d) acc[p][d] = 0u;
        if (c < c1) syndromes16<R, MODE>(sa, sbase, off, acc);
        if (clean_wave(acc)) continue;  // a clean wave column: the locate's cost, nothing more
        mend<R, 4, MODE>(ha, sbase, acc, off, b0, b1, lane, mine);
    }
    post_counters(mine, sa.votes + (size_t)s * (size_t)(sa.n + 2), sa.n + 2, lane);
}

// Byte path: bytes [off0, B) (tails, unaligned blocks).  cols_per_wg = bytes per workgroup.
template <int R, int MODE>
__global__ void __launch_bounds__(kThreads) gf_heal_byte_kernel(const HealLaunch ha) {
    const LocateLaunch& sa = ha.l;
    const GfLaunch& a = sa.g;
    int s, w;
    wg_coords(a, s, w);
    const long long by0 = a.off0 + (long long)w * a.cols_per_wg;
    const long long by1 = min(by0 + (long long)a.cols_per_wg, a.B);
    const uint8_t* sbase = stripe_base<MODE>(a, s);
    int b0, b1;
    candidates(ha, s, b0, b1);
    const int lane = threadIdx.x & 63;
    unsigned mine[kSlots] = {0u, 0u, 0u};
    for (long long ow = by0 + (threadIdx.x & ~63); ow < by1; ow += kThreads) {
        const long long o = ow + lane;
        uint32_t acc[R][1] = {};
        if (o < by1) syndrome_byte<R, MODE>(sa, sbase, o, acc);
        if (clean_wave(acc)) continue;
        mend<R, 1, MODE>(ha, sbase, acc, o, b0, b1, lane, mine);
    }
    post_counters(mine, sa.votes + (size_t)s * (size_t)(sa.n + 2), sa.n + 2, lane);
}

// ---------------------------------------------------------------------------------------------
// Dispatch

struct HealKernels {  // launch_rule.hpp candidate_kernel
    template <int R, int MODE, bool BYTE>
    static const void* kernel() {
        if constexpr (BYTE) return (const void*)gf_heal_byte_kernel<R, MODE>;
        else return (const void*)gf_heal_kernel<R, MODE>;
    }
};

CheckLaunchLog g_heal_log;

}  // namespace

void heal_traffic(long long* launches, long long* bytes) { g_heal_log.traffic(launches, bytes); }

int heal_last_launch(int* v, int cap) { return g_heal_log.last_launch(v, cap); }

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
    return launch_paths(
        a, vec_ok, g_heal_log, (long long)a.S * a.B * bl.n, 1,
        [&](dim3 g) { return launch_kernel(candidate_kernel<HealKernels, 1, false>(a.m, mode), ha, g, st); },
        [&](dim3 g) { return launch_kernel(candidate_kernel<HealKernels, 1, true>(a.m, mode), ha, g, st); });
}

}  // namespace ecg
