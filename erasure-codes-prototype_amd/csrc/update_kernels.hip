// Delta update for MI355X (gfx950, CDNA4): scattered small overwrites applied to data and parity in place.
//
// One kernel, gf_update_kernel<NR, INL, VEC>.  grid.x = R * wg_per_record, linear: workgroup b takes chunk
// b % wg_per_record of record b / wg_per_record.  The record, its column's plan (update_kernels.hpp: up to NR
// destination ids and CoefTabs) and the block bases are uniform per workgroup and read through the constant address
// space (INL: the kernel arguments), so they sit in SGPRs.  The workgroup validates the record as a whole, uniformly:
// a refused record has its state written by lane 0 of its first workgroup and nothing else is read or written; a
// workgroup whose chunk lies past the record's end exits after those loads.
//
// Chunks are cut on the DESTINATION's 16-byte grid: column c of a record is bytes [c0 + 16 c, c0 + 16 c + 16) of the
// blocks, c0 = off & ~15, one lane per column.  Only a record's first and last column can be partial.
//   full column, VEC     16 bytes of input through an unaligned 16-byte global load (the staging range has no alignment
//                        relative to off), 16 of old data, delta split once per dword; then the loads of all nnz parity
//                        columns go out together, nnz gmul per dword, XOR, 16-byte stores.  A column whose delta is
//                        all zero stops after delta_out.
//   partial column, or   the in-range bytes only, one at a time with byte loads and byte stores: two records that cut
//   any column, !VEC     one 16-byte column between them never store to each other's bytes.
// `changed` is counted per lane, summed per wave and added with one vector atomic per wave.  No scalar stores and no
// scalar atomics; data, parity and delta_out see plain vector stores only.
#include "check_device.hpp"
#include "launch_rule.hpp"
#include "update_kernels.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "update_kernels.hip is gfx950 (CDNA4) code"
#endif

namespace ecg {

namespace {

static_assert(kUpdateMaxNnz <= kMaxMT, "a column's plan is one row tile of a program");

typedef u32x4 u32x4_unaligned __attribute__((aligned(1)));

template <int NR, bool INL, bool VEC>
__global__ void __launch_bounds__(kThreads, NR <= 4 ? 6 : 4) gf_update_kernel(const UpdateLaunch a) {
    const long long wg = blockIdx.x;
    const long long r = wg / a.wg_per_record;
    const long long w = wg - r * a.wg_per_record;
    long long stripe, col, off, len, in_off;
    if constexpr (INL) {
        stripe = a.rec[0], col = a.rec[1], off = a.rec[2], len = a.rec[3], in_off = a.rec[4];
    } else {
        const ECG_CONST long long* rec = cst(a.records) + r * kUpdateRecordWords;
        stripe = rec[0], col = rec[1], off = rec[2], len = rec[3], in_off = rec[4];
    }
    unsigned state = kUpdateApplied;
    if (stripe < 0 || stripe >= a.S) state = kUpdateBadStripe;
    else if (col < 0 || col >= a.k_in) state = kUpdateBadCol;
    else if (off < 0 || len < 0 || off > a.B || len > a.B - off) state = kUpdateBadRange;
    else if (len > a.max_len) state = kUpdateTooLong;
    else if (in_off < 0 || in_off > a.in_bytes || len > a.in_bytes - in_off) state = kUpdateBadStaging;
    if (state != kUpdateApplied) {  // uniform
        if (w == 0 && threadIdx.x == 0) a.report[2 * r] = state;
        return;
    }
    const long long c0 = off & ~15LL, end = off + len;
    const long long ncols = len == 0 ? 0 : ((end + 15) >> 4) - (off >> 4);
    const long long w0 = w * a.cols_per_wg;
    if (w0 >= ncols) return;  // the chunk lies past the record's end
    const long long w1 = min(w0 + (long long)a.cols_per_wg, ncols);

    const ECG_CONST int* ids = cst(a.dst_ids) + col * NR;
    const ECG_CONST CoefTab* T = cst(a.tabs) + col * NR;
    int nnz = 0;
#pragma unroll
    for (int p = 0; p < NR; ++p) nnz += ids[p] >= 0 ? 1 : 0;
    uint8_t* dp;
    uint8_t* pp[NR];
    if constexpr (INL) {
        dp = a.idata;
#pragma unroll
        for (int p = 0; p < NR; ++p) pp[p] = a.ipar[p];
    } else {
        uint8_t* sbase = a.base + stripe * a.sstride;
        dp = sbase + (long long)cst(a.src_ids)[col] * a.bstride;
#pragma unroll
        for (int p = 0; p < NR; ++p) pp[p] = sbase + (long long)(p < nnz ? ids[p] : 0) * a.bstride;
    }
    const bool write = a.mode == kUpdateWrite;
    const long long stage = in_off - off;  // staging index of block byte x: stage + x
    unsigned changed = 0u;
    for (long long c = w0 + threadIdx.x; c < w1; c += kThreads) {
        const long long x0 = c0 + (c << 4);
        const long long lo = max(x0, off), hi = min(x0 + 16, end);
        if (VEC && hi - lo == 16) {
            const u32x4 nv = *reinterpret_cast<const u32x4_unaligned*>(a.in + (stage + x0));
            u32x4 dl = nv;
            if (write) dl = nv ^ *reinterpret_cast<const u32x4*>(dp + x0);
            if (a.delta_out) *reinterpret_cast<u32x4_unaligned*>(a.delta_out + (stage + x0)) = dl;
            if ((dl.x | dl.y | dl.z | dl.w) == 0u) continue;
            const uint32_t d[4] = {dl.x, dl.y, dl.z, dl.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) changed += (unsigned)__popc(nonzero_mask(d[q]));
            if (write) *reinterpret_cast<u32x4*>(dp + x0) = nv;
            uint32_t par[NR][4];
#pragma unroll
            for (int p = 0; p < NR; ++p)
                if (p < nnz) load16<0>(pp[p] + x0, par[p]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const Split sp = split(d[q]);
#pragma unroll
                for (int p = 0; p < NR; ++p)
                    if (p < nnz) par[p][q] ^= gmul(T[p], sp);
            }
#pragma unroll
            for (int p = 0; p < NR; ++p)
                if (p < nnz) {
                    u32x4 o;
                    o.x = par[p][0], o.y = par[p][1], o.z = par[p][2], o.w = par[p][3];
                    *reinterpret_cast<u32x4*>(pp[p] + x0) = o;
                }
        } else {
            for (long long x = lo; x < hi; ++x) {
                const uint32_t nb = a.in[stage + x];
                const uint32_t dl = write ? nb ^ (uint32_t)dp[x] : nb;
                if (a.delta_out) a.delta_out[stage + x] = (uint8_t)dl;
                if (dl == 0u) continue;
                ++changed;
                if (write) dp[x] = (uint8_t)nb;
                const Split sp = split(dl);
#pragma unroll
                for (int p = 0; p < NR; ++p)
                    if (p < nnz) pp[p][x] = (uint8_t)(pp[p][x] ^ (gmul(T[p], sp) & 0xffu));
            }
        }
    }
    const unsigned total = wave_sum(changed);  // every lane of the wave is here: the exits above are uniform
    if ((threadIdx.x & 63) == 0 && total != 0u) atomicAdd(a.report + 2 * r + 1, total);
}

template <int NR>
const void* kernel_of(bool inl, bool vec) {
    if (inl) return vec ? (const void*)gf_update_kernel<NR, true, true> : (const void*)gf_update_kernel<NR, true, false>;
    return vec ? (const void*)gf_update_kernel<NR, false, true> : (const void*)gf_update_kernel<NR, false, false>;
}

LaunchLog<kUpdateLaunchFields> g_update_log;

}  // namespace

void update_traffic(long long* launches, long long* records) { g_update_log.traffic(launches, records); }

int update_last_launch(int* v, int cap) { return g_update_log.last_launch(v, cap); }

bool update_grid(long long max_len, long long R, int& cols_per_wg, int& wg_per_record) {
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

hipError_t launch_update(const UpdateLaunch& base, bool vec_ok, int max_nnz, hipStream_t st) {
    const bool inl = base.records == nullptr;
    if (base.R < 1 || base.k_in < 1 || base.mt < 1 || base.mt > kUpdateMaxNnz || max_nnz > base.mt || base.B < 0 ||
        base.max_len < 0 || base.in_bytes < 0 || !base.tabs || !base.src_ids || !base.dst_ids || !base.in ||
        !base.report || (inl ? base.R != 1 || !base.idata : !base.base) ||
        (base.mode != kUpdateWrite && base.mode != kUpdateDelta) || (base.mode == kUpdateDelta && base.delta_out))
        return hipErrorInvalidValue;
    UpdateLaunch a = base;
    if (!update_grid(a.max_len, a.R, a.cols_per_wg, a.wg_per_record)) return hipErrorInvalidConfiguration;
    const void* kernel = pick_of8<1, const void*>(a.mt, nullptr, [&](auto n) -> const void* {
        return kernel_of<decltype(n)::value>(inl, vec_ok);
    });
    g_update_log.count(1, a.R);
    if (vec_ok && a.max_len > 0) g_update_log.record({a.cols_per_wg, a.wg_per_record, a.R, max_nnz});
    return launch_kernel(kernel, a, dim3((unsigned)((long long)a.R * a.wg_per_record)), st);
}

}  // namespace ecg
