// Read-only GF(2^8) parity check for MI355X (gfx950, CDNA4): does a set of stored blocks still satisfy its code?
//
//   counts[s * r + p] = #{ x in [0, B) : XOR_j H[p][j] * in_j[x] != 0 }      (H: r x k check matrix)
//
// The data path is the region product's (gf_kernels.hip; shared pieces in gf_device.hpp, and check_device.hpp for what
// the locate and the heal share with this file): one lane per 16-byte column, non-temporal dwordx4 loads, CoefTab
// tables in SGPRs, the same folds into MT accumulators, the same load batches (check_device.hpp fold_inputs),
// workgroup -> chunk maps (launch_rule.hpp) and occupancy hints.  Where the product stores its accumulators, the
// check counts their nonzero bytes into MT per-lane counters (4 VALU ops per dword against ~18 per coefficient
// for the fold); a wave whose counters are all zero is done, any other reduces them with shuffles and issues at
// most one device-scope atomic add per row -- none where the sum is zero, so a clean stripe reads every byte
// once and writes nothing.  Integer adds commute: the counts are exact and reproducible.
// An encode-shaped check, H = [C | I], folds only C through the tables; row q's stored block is XORed in by one
// v_bitop3 per dword (ScrubLaunch::ident): the check then costs the encode's arithmetic, not (k + m) / k of it.
#include "check_device.hpp"
#include "launch_rule.hpp"
#include "scrub_kernels.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "scrub_kernels.hip is gfx950 (CDNA4) code"
#endif

namespace ecg {

namespace {

static_assert(kMaxMTBin <= 64, "one lane per row of a tile");

// Nonzero bytes of a dword: one bit per nonzero byte is left to count.
__device__ __forceinline__ unsigned nonzero_bytes(uint32_t x) { return (unsigned)__popc(nonzero_mask(x)); }

// Encode-shaped checks, H = [C | I] (ScrubLaunch::ident): the stored block of check row q, folded in after the C part.
template <int MODE>
__device__ __forceinline__ const uint8_t* ident_ptr(const ScrubLaunch& sa, int s, int q) {
    const GfLaunch& a = sa.g;
    if constexpr (MODE == GF_MODE_INLINE) return a.isrc[a.k + q];
    else return a.in_base + (long long)s * a.in_sstride + (long long)(sa.ident_base + q) * a.in_bstride;
}

// Per-lane counters -> counts[0, nrows), per wave.  A wave whose counters are all zero ends here (one ballot): no
// shuffle, no atomic, nothing written.  Otherwise the butterfly leaves every row's wave sum in every lane, lane p
// keeps row p's, and ONE atomic instruction adds the nonzero sums (lanes 0..nrows-1, adjacent counters).  No LDS and
// no barrier: a wave never waits for the other waves of its workgroup.
template <int MT>
__device__ __forceinline__ void post_counts(unsigned (&cnt)[MT], unsigned* out, int nrows) {
    unsigned any = 0u;
#pragma unroll
    for (int p = 0; p < MT; ++p) any |= cnt[p];
    if (__ballot(any != 0u) == 0ull) return;
    const int lane = threadIdx.x & 63;
    unsigned mine = 0u;
#pragma unroll
    for (int p = 0; p < MT; ++p) {
        const unsigned tot = wave_sum(cnt[p]);
        if (lane == p) mine = tot;
    }
    if (lane < nrows && mine != 0u) atomicAdd(out + lane, mine);
}

// Vector path: bytes [0, 16 * floor(B / 16)) of every block; all pointers 16-byte aligned.
// grid.x = S * wg_per_stripe (stripe-major), grid.y = row tiles of MT check rows, each reading all k inputs.
template <int MT, int MODE, bool BIN>
__global__ void __launch_bounds__(kThreads, occupancy_for(MT)) gf_scrub_kernel(const ScrubLaunch sa) {
    const GfLaunch& a = sa.g;
    int s, w;
    wg_coords(a, s, w);
    const int rt = blockIdx.y;
    const int prog = launch_prog<MODE>(a, s);
    const int k = a.k;
    const int row0 = rt * MT;
    const int nrows = min(MT, a.m - row0);
    const ECG_CONST CoefTab* T = cst(a.tabs) + (size_t)(prog * a.rtiles + rt) * (size_t)k * MT;
    const long long ncols = a.B >> 4;
    const long long c0 = (long long)w * a.cols_per_wg;
    const long long c1 = min(c0 + (long long)a.cols_per_wg, ncols);

    unsigned cnt[MT];
#pragma unroll
    for (int p = 0; p < MT; ++p) cnt[p] = 0u;

    for (long long c = c0 + threadIdx.x; c < c1; c += kThreads) {
        const long long off = c << 4;
        uint32_t acc[MT][4];
#pragma unroll
        for (int p = 0; p < MT; ++p)
#pragma unroll
            for (int d = 0; d < 4; ++d) acc[p][d] = 0u;

        fold_inputs<MT, BIN>(k, T, off, acc, [&](int j) { return src_ptr<MODE>(a, s, prog, j); });
        if (sa.ident) {  // uniform.  acc[p] ^= the block row p checks: one XOR per dword where a table fold takes ~18
            constexpr int IB = MT < 4 ? MT : 4;  // loads in flight, as a load batch
#pragma unroll
            for (int p0 = 0; p0 < MT; p0 += IB) {
                uint32_t x[IB][4];
                // straight-line loads: a row past the tile's last re-reads the tile's first block, masked out below
#pragma unroll
                for (int u = 0; u < IB; ++u) {
                    const int p = p0 + u;
                    if (p < MT) load16<1>(ident_ptr<MODE>(sa, s, row0 + (p < nrows ? p : 0)) + off, x[u]);
                }
#pragma unroll
                for (int u = 0; u < IB; ++u)
                    if (p0 + u < MT) {
                        const uint32_t keep = p0 + u < nrows ? ~0u : 0u;
#pragma unroll
                        for (int d = 0; d < 4; ++d)
                            acc[p0 + u][d] = __builtin_amdgcn_bitop3_b32(acc[p0 + u][d], x[u][d], keep, 0x78);
                    }
            }
        }
        // rows past nrows have all-zero tables (Engine::program_set pads the last tile): they count nothing
#pragma unroll
        for (int p = 0; p < MT; ++p)
#pragma unroll
            for (int d = 0; d < 4; ++d) cnt[p] += nonzero_bytes(acc[p][d]);
    }
    post_counts<MT>(cnt, sa.counts + (size_t)s * a.m + row0, nrows);
}

// Byte path: bytes [off0, B) (tails, unaligned blocks).  cols_per_wg = bytes per workgroup.
template <int MT, int MODE, bool BIN>
__global__ void __launch_bounds__(kThreads) gf_scrub_byte_kernel(const ScrubLaunch sa) {
    const GfLaunch& a = sa.g;
    int s, w;
    wg_coords(a, s, w);
    const int rt = blockIdx.y;
    const int prog = launch_prog<MODE>(a, s);
    const int k = a.k;
    const int row0 = rt * MT;
    const int nrows = min(MT, a.m - row0);
    const ECG_CONST CoefTab* T = cst(a.tabs) + (size_t)(prog * a.rtiles + rt) * (size_t)k * MT;
    const long long b0 = a.off0 + (long long)w * a.cols_per_wg;
    const long long b1 = min(b0 + (long long)a.cols_per_wg, a.B);
    unsigned cnt[MT];
#pragma unroll
    for (int p = 0; p < MT; ++p) cnt[p] = 0u;
    for (long long o = b0 + threadIdx.x; o < b1; o += kThreads) {
        uint32_t acc[MT];
#pragma unroll
        for (int p = 0; p < MT; ++p) acc[p] = 0u;
        for (int j = 0; j < k; ++j) {
            const uint32_t x = src_ptr<MODE>(a, s, prog, j)[o];
            const ECG_CONST CoefTab* t = T + (size_t)j * MT;
            if constexpr (BIN) {
#pragma unroll
                for (int p = 0; p < MT; ++p) acc[p] ^= x & t[p].mask;
            } else {
                const Split sp = split(x);
#pragma unroll
                for (int p = 0; p < MT; ++p) acc[p] ^= gmul(t[p], sp);
            }
        }
        if (sa.ident) {
#pragma unroll
            for (int p = 0; p < MT; ++p)
                if (p < nrows) acc[p] ^= ident_ptr<MODE>(sa, s, row0 + p)[o];
        }
#pragma unroll
        for (int p = 0; p < MT; ++p) cnt[p] += (acc[p] & 0xffu) != 0u ? 1u : 0u;
    }
    post_counts<MT>(cnt, sa.counts + (size_t)s * a.m + row0, nrows);
}

// ---------------------------------------------------------------------------------------------
// Dispatch

template <int MODE, bool BIN, bool BYTE>
const void* pick_mt(int MT) {
    const auto one = [](auto mt) -> const void* {
        if constexpr (BYTE) return (const void*)gf_scrub_byte_kernel<decltype(mt)::value, MODE, BIN>;
        else return (const void*)gf_scrub_kernel<decltype(mt)::value, MODE, BIN>;
    };
    if constexpr (BIN)  // wide BINARY tiles (kMaxMTBin)
        if (MT > 8) return pick_of8<9, const void*>(MT, nullptr, one);
    return pick_of8<1, const void*>(MT, nullptr, one);
}

template <bool BYTE>
const void* pick(const GfLaunch& a, int mode) {
    if (mode == GF_MODE_INLINE)
        return a.binary ? pick_mt<GF_MODE_INLINE, true, BYTE>(a.MT) : pick_mt<GF_MODE_INLINE, false, BYTE>(a.MT);
    if (mode == GF_MODE_STRIDED)
        return a.binary ? pick_mt<GF_MODE_STRIDED, true, BYTE>(a.MT) : pick_mt<GF_MODE_STRIDED, false, BYTE>(a.MT);
    return nullptr;
}

CheckLaunchLog g_scrub_log;

}  // namespace

void scrub_traffic(long long* launches, long long* bytes) { g_scrub_log.traffic(launches, bytes); }

int scrub_last_launch(int* v, int cap) { return g_scrub_log.last_launch(v, cap); }

hipError_t launch_scrub(const ScrubLaunch& base, int mode, bool vec_ok, hipStream_t st) {
    const GfLaunch& b = base.g;
    if (b.k < 1 || b.m < 1 || b.S < 1 || b.B < 0 || b.MT < 1 || b.MT > (b.binary ? kMaxMTBin : kMaxMT) ||
        b.rtiles < 1 || (long long)b.rtiles * b.MT < b.m || !base.counts)
        return hipErrorInvalidValue;
    if (mode != GF_MODE_INLINE && mode != GF_MODE_STRIDED) return hipErrorInvalidValue;
    if (mode == GF_MODE_INLINE && (b.S != 1 || b.k + (base.ident ? b.m : 0) > kInlineSrc)) return hipErrorInvalidValue;
    if (b.B == 0) return hipSuccess;
    ScrubLaunch sa = base;
    GfLaunch& a = sa.g;
    a.row_split = 0;
    return launch_paths(
        a, vec_ok, g_scrub_log, (long long)a.S * a.B * ((long long)a.rtiles * a.k + (sa.ident ? a.m : 0)), a.rtiles,
        [&](dim3 g) { return launch_kernel(pick<false>(a, mode), sa, g, st); },
        [&](dim3 g) { return launch_kernel(pick<true>(a, mode), sa, g, st); });
}

}  // namespace ecg
