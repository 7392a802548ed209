// The host-side launch rule of every kernel family -- launch_gf (gf_kernels.hip) and launch_scrub, launch_locate,
// launch_heal and launch_heal2 (scrub_kernels.hip, locate_kernels.hip, heal_kernels.hip, heal2_kernels.hip): how bytes
// [0, B) of S launch stripes are dealt to workgroups (plan_vector_path, plan_byte_path), the run-time choice of a
// kernel instantiation (pick_of8), what each library records about its launches (LaunchLog, one per library; the sums
// keep one too), and the check libraries' vector-then-byte launch sequence (launch_paths).  Host-only and header-only.
#pragma once
#include <atomic>
#include <type_traits>

#include "gf_kernels.hpp"

namespace ecg {

// Kernels a library launched in this process, the bytes they move as planned, and the N fields of its most recent
// launch (all zero before the first).  Relaxed atomics, diagnostics only: a reader racing a launch may see fields of
// two launches.
template <int N>
struct LaunchLog {
    std::atomic<long long> launched{0}, moved{0};
    std::atomic<int> last[N]{};

    void count(int launches, long long bytes) {
        launched.fetch_add(launches, std::memory_order_relaxed);
        moved.fetch_add(bytes, std::memory_order_relaxed);
    }
    void traffic(long long* launches, long long* bytes) const {
        if (launches) *launches = launched.load(std::memory_order_relaxed);
        if (bytes) *bytes = moved.load(std::memory_order_relaxed);
    }
    void record(const int (&v)[N]) {
        for (int i = 0; i < N; ++i) last[i].store(v[i], std::memory_order_relaxed);
    }
    // Returns the field count; v is written when cap suffices.
    int last_launch(int* v, int cap) const {
        if (v && cap >= N)
            for (int i = 0; i < N; ++i) v[i] = last[i].load(std::memory_order_relaxed);
        return N;
    }
};

// The check libraries' record: grid_map, map_group, cols_per_wg, wg_per_stripe, S, rtiles of the most recent
// vector-path launch as placed in the descriptor after the fallbacks.
constexpr int kCheckLaunchFields = 6;
using CheckLaunchLog = LaunchLog<kCheckLaunchFields>;

// Vector path over bytes [0, vec_bytes), vec_bytes > 0 a multiple of 16: one lane per 16-byte column, grid.x = gx =
// S * wg_per_stripe.  auto_map is the workgroup -> chunk map ECG_OPT_GRID_MAP 3 stands for in this launch: the product
// resolves its auto rule (gf_kernels.hip outputs_in_stripe); a check reads what an encode into the stripe reads and
// passes 1 (XCD-contiguous chunks).  ECG_OPT_GRID_MAP 0 / 2 are honoured, with the fallbacks gf_device.hpp wg_coords
// relies on (gx % 8 == 0; S % (8 G) == 0).  Fills the descriptor and gx; records nothing.
inline hipError_t plan_vector_path(GfLaunch& a, long long vec_bytes, int auto_map, long long& gx) {
    const long long ncols = vec_bytes >> 4;
    long long cpw = get_option(ECG_OPT_COLS_PER_WG);
    if (cpw <= 0) cpw = kThreads;  // 2 KiB of every block per workgroup (measured best, r01 microbench)
    if (ncols < cpw) cpw = ((ncols + kThreads - 1) / kThreads) * kThreads;
    a.cols_per_wg = (int)cpw;
    a.wg_per_stripe = (int)((ncols + cpw - 1) / cpw);
    a.off0 = 0;
    gx = (long long)a.S * a.wg_per_stripe;
    if (gx > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    long long gm = get_option(ECG_OPT_GRID_MAP);
    if (gm == 3) gm = auto_map;
    long long G = get_option(ECG_OPT_MAP_GROUP);
    while (G > 1 && a.S % (8 * G) != 0) G >>= 1;  // the largest power-of-two divisor run that tiles S
    if (gm == 2 && a.S % (8 * G) != 0) gm = 1;
    a.grid_map = (gm == 1 && gx % 8 == 0) ? 1 : (gm == 2) ? 2 : 0;
    a.map_group = (int)G;
    return hipSuccess;
}

// Byte path over bytes [vec_bytes, B) (tails, unaligned blocks): one lane per byte, cols_per_wg = bytes per
// workgroup, linear map.
inline hipError_t plan_byte_path(GfLaunch& a, long long vec_bytes, long long& gx) {
    const long long nbytes = a.B - vec_bytes;
    long long bpw = 16LL * kThreads;
    if (nbytes < bpw) bpw = ((nbytes + kThreads - 1) / kThreads) * kThreads;
    a.cols_per_wg = (int)bpw;
    a.wg_per_stripe = (int)((nbytes + bpw - 1) / bpw);
    a.off0 = vec_bytes;
    a.grid_map = 0;
    gx = (long long)a.S * a.wg_per_stripe;
    return gx > 0x7fffffffLL ? hipErrorInvalidConfiguration : hipSuccess;
}

// f(std::integral_constant<int, N>()) for N = n in [LO, LO + 8), else `none`: the R / MT switch of the dispatchers,
// which turns a run-time row count into a template argument (decltype(N)::value).
template <int LO, class T, class F>
T pick_of8(int n, T none, F f) {
    switch (n - LO) {
        case 0: return f(std::integral_constant<int, LO>());
        case 1: return f(std::integral_constant<int, LO + 1>());
        case 2: return f(std::integral_constant<int, LO + 2>());
        case 3: return f(std::integral_constant<int, LO + 3>());
        case 4: return f(std::integral_constant<int, LO + 4>());
        case 5: return f(std::integral_constant<int, LO + 5>());
        case 6: return f(std::integral_constant<int, LO + 6>());
        case 7: return f(std::integral_constant<int, LO + 7>());
        default: return none;
    }
}

// What every check library's launch_* does once its descriptor copy `a` has passed the library's own checks: count the
// launches and the `planned` bytes they read in `log`, then the vector path over the 16-byte columns (if vec_ok),
// recorded in `log`, and the byte path over what is left, which is not.  vec(grid) and byte(grid) launch the library's
// kernel for `a` as it then stands; gy is the grid's y dimension (the scrub's row tiles, else 1).
template <class Vec, class Byte>
hipError_t launch_paths(GfLaunch& a, bool vec_ok, CheckLaunchLog& log, long long planned, int gy, Vec vec, Byte byte) {
    const long long vec_bytes = vec_ok ? (a.B & ~15LL) : 0;
    log.count((vec_bytes > 0) + (vec_bytes < a.B), planned);
    long long gx = 0;
    if (vec_bytes > 0) {
        if (const hipError_t e = plan_vector_path(a, vec_bytes, 1, gx); e != hipSuccess) return e;
        log.record({a.grid_map, a.map_group, a.cols_per_wg, a.wg_per_stripe, a.S, a.rtiles});
        if (const hipError_t e = vec(dim3((unsigned)gx, (unsigned)gy)); e != hipSuccess) return e;
    }
    if (vec_bytes < a.B) {
        if (const hipError_t e = plan_byte_path(a, vec_bytes, gx); e != hipSuccess) return e;
        if (const hipError_t e = byte(dim3((unsigned)gx, (unsigned)gy)); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// One workgroup shape for every check kernel; a null kernel (no instantiation for the descriptor) is an error.
template <class Launch>
hipError_t launch_kernel(const void* kernel, const Launch& a, dim3 grid, hipStream_t st) {
    if (!kernel) return hipErrorInvalidValue;
    void* argv[] = {(void*)&a};
    return hipLaunchKernel(kernel, grid, dim3(kThreads), argv, 0, st);
}

// The kernel of a candidate-test library for R check rows, LO <= R <= kMaxMT, or null.  K::kernel<R, MODE, BYTE>() names
// the library's instantiations (locate, heal and heal2 each define such a K).
template <class K, int LO, int MODE, bool BYTE>
const void* candidate_kernel_of(int R) {
    return pick_of8<LO, const void*>(R, nullptr, [](auto r) -> const void* {
        constexpr int RR = decltype(r)::value;
        if constexpr (RR <= kMaxMT) return K::template kernel<RR, MODE, BYTE>();
        else return nullptr;
    });
}

template <class K, int LO, bool BYTE>
const void* candidate_kernel(int R, int mode) {
    if (mode == GF_MODE_INLINE) return candidate_kernel_of<K, LO, GF_MODE_INLINE, BYTE>(R);
    if (mode == GF_MODE_STRIDED) return candidate_kernel_of<K, LO, GF_MODE_STRIDED, BYTE>(R);
    return nullptr;
}

}  // namespace ecg
