// The host-side launch rule shared by launch_scrub, launch_locate and launch_heal (scrub_kernels.hip,
// locate_kernels.hip, heal_kernels.hip): how bytes [0, B) of S launch stripes are dealt to workgroups, and what each
// library records about its launches.  Host-only and header-only; every library owns one CheckLaunchLog.
#pragma once
#include <atomic>
#include <type_traits>

#include "gf_kernels.hpp"

namespace ecg {

// The fields of a last-launch record: grid_map, map_group, cols_per_wg, wg_per_stripe, S, rtiles.
constexpr int kCheckLaunchFields = 6;

// Kernels a library launched in this process, the bytes they read as planned, and the geometry of its most recent
// vector-path launch as placed in the descriptor after the fallbacks (all zero before the first).
struct CheckLaunchLog {
    std::atomic<long long> launched{0}, read{0};
    std::atomic<int> last[kCheckLaunchFields]{};

    void count(int launches, long long bytes) {
        launched.fetch_add(launches, std::memory_order_relaxed);
        read.fetch_add(bytes, std::memory_order_relaxed);
    }
    void traffic(long long* launches, long long* bytes) const {
        if (launches) *launches = launched.load(std::memory_order_relaxed);
        if (bytes) *bytes = read.load(std::memory_order_relaxed);
    }
    // Returns the field count; v is written when cap suffices.
    int last_launch(int* v, int cap) const {
        if (v && cap >= kCheckLaunchFields)
            for (int i = 0; i < kCheckLaunchFields; ++i) v[i] = last[i].load(std::memory_order_relaxed);
        return kCheckLaunchFields;
    }
};

// Vector path over bytes [0, vec_bytes), vec_bytes > 0 a multiple of 16: one lane per 16-byte column, grid.x = gx =
// S * wg_per_stripe.  The workgroup -> chunk map is the product's auto rule for outputs inside the input stripes
// (XCD-contiguous chunks): a check reads what an encode into the stripe reads.  ECG_OPT_GRID_MAP 0 / 2 are honoured as
// there, with the fallbacks gf_device.hpp wg_coords relies on (gx % 8 == 0; S % (8 G) == 0).  Recorded in `log`.
inline hipError_t plan_vector_path(GfLaunch& a, long long vec_bytes, CheckLaunchLog& log, long long& gx) {
    const long long ncols = vec_bytes >> 4;
    long long cpw = get_option(ECG_OPT_COLS_PER_WG);
    if (cpw <= 0) cpw = kThreads;  // 2 KiB of every block per workgroup, as the product
    if (ncols < cpw) cpw = ((ncols + kThreads - 1) / kThreads) * kThreads;
    a.cols_per_wg = (int)cpw;
    a.wg_per_stripe = (int)((ncols + cpw - 1) / cpw);
    a.off0 = 0;
    gx = (long long)a.S * a.wg_per_stripe;
    if (gx > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    long long gm = get_option(ECG_OPT_GRID_MAP);
    if (gm == 3) gm = 1;
    long long G = get_option(ECG_OPT_MAP_GROUP);
    while (G > 1 && a.S % (8 * G) != 0) G >>= 1;
    if (gm == 2 && a.S % (8 * G) != 0) gm = 1;
    a.grid_map = (gm == 1 && gx % 8 == 0) ? 1 : (gm == 2) ? 2 : 0;
    a.map_group = (int)G;
    const int geo[kCheckLaunchFields] = {a.grid_map, a.map_group, a.cols_per_wg, a.wg_per_stripe, a.S, a.rtiles};
    for (int i = 0; i < kCheckLaunchFields; ++i) log.last[i].store(geo[i], std::memory_order_relaxed);
    return hipSuccess;
}

// Byte path over bytes [vec_bytes, B) (tails, unaligned blocks): one lane per byte, cols_per_wg = bytes per
// workgroup, linear map.  Not recorded.
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

}  // namespace ecg
