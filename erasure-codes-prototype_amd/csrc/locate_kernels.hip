// Corruption localisation for MI355X (gfx950, CDNA4): which block of a stripe that fails its check is damaged?
//
// If only block b is damaged at byte position x, by the error value e, every check row p sees s_p[x] = H[p][b] * e:
// the syndrome vector is proportional to column b of H.  Per selected stripe (locate_kernels.hpp LocateLaunch)
//   votes[b] = #{ x : s[x] = e * H[:, b], e != 0 },  votes[n] = #{ x : s[x] != 0 },  votes[n + 1] = #{ bad x that no
//   single block explains }.
//
// The data path is the scrub's (scrub_kernels.hip; shared pieces in gf_device.hpp and check_device.hpp): one lane per
// 16-byte column, non-temporal dwordx4 loads, CoefTab tables in SGPRs, the same folds and load batches, the same
// workgroup -> chunk maps, and for H = [C | I] only C through the tables with the stored blocks XORed in.  The
// difference: ONE lane holds all R <= 8 syndromes of its column (one row tile, GENERAL flavour; c = 0 and c = 1 tables
// are exact, so a 0/1 H runs through it too).  A wave whose syndromes are all zero goes on to its next column after one
// OR-reduce per lane and one ballot: clean data costs what the scrub costs.  Any other wave runs the candidate test
// (check_device.hpp candidate_loop, which the heal shares): a uniform loop over the blocks b, with p0 = p0(b) the
// first row where column b is nonzero,
//   residual = OR_q  s_q ^ (H[q][b] / H[p0][b]) * s_p0          (ratio tables; the term q = p0 is s_p0 ^ 1 * s_p0 = 0:
//                                                                 kept, so the loop needs no row index in a register)
//   votes    = bytes where s_p0 != 0 and residual == 0
// by the 0x7f / 0x80 byte masks of the scrub.  s_p0 is picked by R - 1 selects on the uniform p0, never by indexing
// the accumulators (that would put them in scratch).  A candidate no lane votes for costs one ballot; the others are
// summed over the wave at once and added to the lane that owns the counter (lane i of register j owns counter
// 64 j + i), so the n + 2 counters of a wave live in three VGPRs, statically indexed, and leave it in at most three
// atomic instructions -- none when they are all zero: a clean stripe writes nothing.  No LDS, no barrier.
// Integer adds commute: the counts are exact and reproducible.
#include "check_device.hpp"
#include "launch_rule.hpp"
#include "locate_kernels.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "locate_kernels.hip is gfx950 (CDNA4) code"
#endif

namespace ecg {

namespace {

// The candidate test over every block: the votes are all a locate wants of it.
template <int R, int W>
__device__ __forceinline__ void tally(const LocateLaunch& sa, const uint32_t (&syn)[R][W], int lane,
                                      unsigned (&mine)[kSlots]) {
    candidate_loop<R, W>(sa, syn, 0, sa.n, lane, mine, [](int, const uint32_t (&)[W], const uint32_t (&)[W]) {});
}

// Vector path: bytes [0, 16 * floor(B / 16)) of every block; all pointers 16-byte aligned.
// grid.x = S * wg_per_stripe (stripe-major).  The column loop is per wave, so that every lane reaches the wave sums.
// Occupancy hints as the scrub's tiles of as many rows.
template <int R, int MODE>
__global__ void __launch_bounds__(kThreads, occupancy_for(R)) gf_locate_kernel(const LocateLaunch sa) {
    const GfLaunch& a = sa.g;
    int s, w;
    wg_coords(a, s, w);
    const uint8_t* sbase = stripe_base<MODE>(a, s);
    const long long ncols = a.B >> 4;  // < 2^27: B < 2^31
    const long long w0 = (long long)w * a.cols_per_wg;
    const int c0 = (int)w0, c1 = (int)min(w0 + (long long)a.cols_per_wg, ncols);
    const int lane = threadIdx.x & 63;
    unsigned mine[kSlots] = {0u, 0u, 0u};
    for (int cw = c0 + (int)(threadIdx.x & ~63u); cw < c1; cw += kThreads) {
        const int c = cw + lane;
        // zeroed in place: through `= {}` or a helper R = 3, 4 take one VGPR more, and R = 4 INLINE loses a wave per SIMD
        uint32_t acc[R][4];
#pragma unroll
        for (int p = 0; p < R; ++p)
#pragma unroll
            for (int d = 0; d < 4; ++d) acc[p][d] = 0u;
        if (c < c1) syndromes16<R, MODE>(sa, sbase, (long long)c << 4, acc);
        if (clean_wave(acc)) continue;  // a clean wave column: the scrub's cost, nothing more
        tally<R, 4>(sa, acc, lane, mine);
    }
    post_counters(mine, sa.votes + (size_t)s * (size_t)(sa.n + 2), sa.n + 2, lane);
}

// Byte path: bytes [off0, B) (tails, unaligned blocks).  cols_per_wg = bytes per workgroup.
template <int R, int MODE>
__global__ void __launch_bounds__(kThreads) gf_locate_byte_kernel(const LocateLaunch sa) {
    const GfLaunch& a = sa.g;
    int s, w;
    wg_coords(a, s, w);
    const long long b0 = a.off0 + (long long)w * a.cols_per_wg;
    const long long b1 = min(b0 + (long long)a.cols_per_wg, a.B);
    const uint8_t* sbase = stripe_base<MODE>(a, s);
    const int lane = threadIdx.x & 63;
    unsigned mine[kSlots] = {0u, 0u, 0u};
    for (long long ow = b0 + (threadIdx.x & ~63); ow < b1; ow += kThreads) {
        const long long o = ow + lane;
        uint32_t acc[R][1] = {};
        if (o < b1) syndrome_byte<R, MODE>(sa, sbase, o, acc);
        if (clean_wave(acc)) continue;
        tally<R, 1>(sa, acc, lane, mine);
    }
    post_counters(mine, sa.votes + (size_t)s * (size_t)(sa.n + 2), sa.n + 2, lane);
}

// ---------------------------------------------------------------------------------------------
// Dispatch

struct LocateKernels {  // launch_rule.hpp candidate_kernel
    template <int R, int MODE, bool BYTE>
    static const void* kernel() {
        if constexpr (BYTE) return (const void*)gf_locate_byte_kernel<R, MODE>;
        else return (const void*)gf_locate_kernel<R, MODE>;
    }
};

CheckLaunchLog g_locate_log;

}  // namespace

void locate_traffic(long long* launches, long long* bytes) { g_locate_log.traffic(launches, bytes); }

int locate_last_launch(int* v, int cap) { return g_locate_log.last_launch(v, cap); }

hipError_t launch_locate(const LocateLaunch& base, int mode, bool vec_ok, hipStream_t st) {
    const GfLaunch& b = base.g;
    if (b.k < 1 || b.m < 1 || b.m > kMaxMT || b.MT != b.m || b.rtiles != 1 || b.S < 1 || b.B < 0 || base.n < 1 ||
        base.n > kInlineSrc || base.n != b.k + (base.ident ? b.m : 0) || !base.votes || !base.ratios || !b.tabs)
        return hipErrorInvalidValue;
    if (mode != GF_MODE_INLINE && mode != GF_MODE_STRIDED) return hipErrorInvalidValue;
    if (mode == GF_MODE_INLINE && b.S != 1) return hipErrorInvalidValue;
    if (b.B == 0) return hipSuccess;
    LocateLaunch sa = base;
    GfLaunch& a = sa.g;
    a.row_split = 0;
    a.prog_of_stripe = nullptr;
    return launch_paths(
        a, vec_ok, g_locate_log, (long long)a.S * a.B * sa.n, 1,
        [&](dim3 g) { return launch_kernel(candidate_kernel<LocateKernels, 1, false>(a.m, mode), sa, g, st); },
        [&](dim3 g) { return launch_kernel(candidate_kernel<LocateKernels, 1, true>(a.m, mode), sa, g, st); });
}

}  // namespace ecg
