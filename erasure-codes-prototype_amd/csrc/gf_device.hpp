// Device-side building blocks shared by the GF(2^8) kernel families: the region product (gf_kernels.hip, in
// libecg.so) and, through check_device.hpp, the kernels over a check matrix -- the scrub (scrub_kernels.hip, in
// libecg_scrub.so), the locate (locate_kernels.hip, in libecg_locate.so) and the heal (heal_kernels.hip, in
// libecg_heal.so).  Everything here is inlined into the kernels that use it; the header defines no kernel and no
// host state.
#pragma once
#include "gf_kernels.hpp"

namespace ecg {

// Uniform metadata (coefficient tables, block ids, pointer tables) is read through the constant
// address space so the backend selects scalar (SMEM) loads into SGPRs; through a plain global
// pointer it cannot prove the output stores never clobber it and falls back to per-lane loads.
#define ECG_CONST __attribute__((address_space(4)))
template <typename T>
__device__ __forceinline__ const ECG_CONST T* cst(const T* p) {
    return (const ECG_CONST T*)p;
}

template <int MODE>
__device__ __forceinline__ const uint8_t* src_ptr(const GfLaunch& a, int s, int prog, int j) {
    if constexpr (MODE == GF_MODE_INLINE || MODE == GF_MODE_INLINE_LAT) {
        return a.isrc[j];
    } else if constexpr (MODE == GF_MODE_PTRS) {
        return cst(a.src_ptrs)[(size_t)s * a.k + j];
    } else {
        const long long sa = a.stripe_of ? (long long)cst(a.stripe_of)[s] : (long long)s;
        return a.in_base + sa * a.in_sstride + (long long)cst(a.src_ids)[prog * a.k + j] * a.in_bstride;
    }
}

__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) {
    return __builtin_amdgcn_perm(hi, lo, sel);
}

// gfx950 v_bitop3_b32, LUT index = S0<<2 | S1<<1 | S2.  0x96 = a ^ b ^ c.
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// NT policy bits: 1 = non-temporal loads, 2 = non-temporal stores.
template <int NT>
__device__ __forceinline__ void load16(const uint8_t* p, uint32_t (&x)[4]) {
    u32x4 v;
    if constexpr (NT & 1) v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    else v = *reinterpret_cast<const u32x4*>(p);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
}

// Bit-field split of one input dword: the v_perm selectors shared by every output row.
struct Split {
    uint32_t i0, i1, i2;
};

__device__ __forceinline__ Split split(uint32_t x) {
    return {x & 0x07070707u, (x >> 3) & 0x07070707u, (x >> 6) & 0x03030303u};
}

// c * x for the four bytes of one dword: three v_perm lookups + one v_bitop3.
__device__ __forceinline__ uint32_t gmul(const ECG_CONST CoefTab& t, const Split& s) {
    return xor3(perm(t.t0hi, t.t0lo, s.i0), perm(t.t1hi, t.t1lo, s.i1), perm(t.t2, t.t2, s.i2));
}

// GENERAL flavour: U inputs folded into MT accumulators, input pairs share one v_bitop3.  Every
// coefficient goes through the tables (c = 0 and c = 1 tables are exact).
template <int MT, int U>
__device__ __forceinline__ void fold_general(const uint32_t (&x)[U][4], const ECG_CONST CoefTab* t,
                                             uint32_t (&acc)[MT][4]) {
#pragma unroll
    for (int u = 0; u + 1 < U; u += 2) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const Split s0 = split(x[u][d]);
            const Split s1 = split(x[u + 1][d]);
#pragma unroll
            for (int p = 0; p < MT; ++p)
                acc[p][d] = xor3(acc[p][d], gmul(t[u * MT + p], s0), gmul(t[(u + 1) * MT + p], s1));
        }
    }
    if constexpr (U & 1) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const Split s0 = split(x[U - 1][d]);
#pragma unroll
            for (int p = 0; p < MT; ++p) acc[p][d] ^= gmul(t[(U - 1) * MT + p], s0);
        }
    }
}

// BINARY flavour (every coefficient 0 or 1: perform_addition, LRC local rows, PC merges):
// acc ^= x & mask in one v_bitop3 (0x78 = S0 ^ (S1 & S2)), mask = 0 or ~0 from SGPRs.
template <int MT, int U>
__device__ __forceinline__ void fold_binary(const uint32_t (&x)[U][4], const ECG_CONST CoefTab* t,
                                            uint32_t (&acc)[MT][4]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int p = 0; p < MT; ++p) {
            const uint32_t msk = t[u * MT + p].mask;
#pragma unroll
            for (int d = 0; d < 4; ++d) acc[p][d] = __builtin_amdgcn_bitop3_b32(acc[p][d], x[u][d], msk, 0x78);
        }
}

template <int MT, int U, bool BIN>
__device__ __forceinline__ void fold(const uint32_t (&x)[U][4], const ECG_CONST CoefTab* t, uint32_t (&acc)[MT][4]) {
    if constexpr (BIN) fold_binary<MT, U>(x, t, acc);
    else fold_general<MT, U>(x, t, acc);
}

// Minimum waves per EU the register allocator must allow (r01 sweep, tools/gpu_variants.sh): 8 for the
// 1-2-output kernels (decode, repair, XOR: +2 % at 8 vs 6), 6 for 3-4 outputs (encode: 8 costs 1 %),
// 4 above -- except 5 outputs: under the 128-VGPR cap of 4 waves the allocator spilled 12 bytes per lane
// in the GENERAL flavour, while a hint of 3 lets it settle at 82 VGPRs (5 waves) with no scratch (r01; with
// two inputs per load batch since r06 it takes 61, 7 waves).
// ECG_OCC_OVERRIDE is for tuning builds only.
constexpr int occupancy_for(int MT) {
#ifdef ECG_OCC_OVERRIDE
    return MT <= 4 ? ECG_OCC_OVERRIDE : 4;
#else
    return MT <= 2 ? 8 : MT <= 4 ? 6 : MT == 5 ? 3 : 4;  // MT 9-16 (BINARY only): 64 accumulator VGPRs at 16
#endif
}

// Workgroup -> (stripe, column chunk).  grid_map 0: linear (workgroup b takes chunk b).  grid_map 1:
// XCD-contiguous -- the dispatcher deals workgroups round-robin over the 8 XCDs, so b % 8 names the
// XCD group; each group is given a contiguous 1/8 of the chunk list (T1 in the HIP guide; here for
// DRAM locality of the concurrently active chunks, not L2 reuse).  grid_map 2: runs of G = map_group
// adjacent launch stripes are dealt round-robin to the XCD groups (G = 1: stripe s on group s % 8), each
// group takes its stripes and their chunks in order.  Speed only, never correctness.
__device__ __forceinline__ void wg_coords(const GfLaunch& a, int& s, int& w) {
    long long b = blockIdx.x;
    if (a.grid_map == 1) {
        const long long G = (long long)gridDim.x;
        const long long per = G >> 3;  // G % 8 == 0 is checked by the host
        b = (b & 7) * per + (b >> 3);
    } else if (a.grid_map == 2) {  // runs of G stripes dealt to the XCD groups (S % (8 G) == 0 checked by the host)
        const long long i = b >> 3;                  // the i-th workgroup dealt to this XCD group
        const long long ls = i / a.wg_per_stripe;    // the group's ls-th stripe, chunks in order
        const long long G = a.map_group;
        s = (int)(((ls / G) * 8 + (b & 7)) * G + ls % G);
        w = (int)(i - ls * a.wg_per_stripe);
        return;
    }
    s = (int)(b / a.wg_per_stripe);
    w = (int)(b - (long long)s * a.wg_per_stripe);
}

// The program of launch stripe s; s becomes the stripe it addresses.  Row split (STRIDED, row_split = R):
// launch stripe s is output row s % R of stripe s / R, run as its own program (the host split each
// program into R single-row programs whose inputs are that row's own, engine.cpp run_strided).
template <int MODE>
__device__ __forceinline__ int launch_prog(const GfLaunch& a, int& s) {
    int r = 0;
    if constexpr (MODE == GF_MODE_STRIDED) {
        if (a.row_split) {
            r = s % a.row_split;
            s = s / a.row_split;
        }
    }
    const int p = a.prog_of_stripe ? cst(a.prog_of_stripe)[s] : 0;
    if constexpr (MODE == GF_MODE_STRIDED) return a.row_split ? p * a.row_split + r : p;
    return p;
}

// ---------------------------------------------------------------------------------------------
// Input blocks whose loads a lane keeps in flight before folding them (ECG_TUNE_LOAD_BATCH: tuning builds only).
#ifdef ECG_TUNE_LOAD_BATCH
constexpr int kLoadBatch = ECG_TUNE_LOAD_BATCH;
#else
constexpr int kLoadBatch = 4;
#endif
// GENERAL tiles of 5+ outputs take two: with four, 4 inputs x MT tables (5 dwords each) outgrow the SGPR file and the
// tile needs 87 VGPRs at MT = 5 (5 waves per SIMD); with two it takes 61 (7 waves), and a 12 -> 5 launch (the
// Azure+1 encode) runs 0.745 of 8 TB/s instead of 0.684-0.694, 12 -> 6 0.70 instead of 0.66, 10 -> 8 0.665 instead
// of 0.61 (profiles/r06/families/shape_probe/sp_glb*.log, two processes each).
#ifdef ECG_TUNE_GEN_WIDE_LB
constexpr int kGenWideLB = ECG_TUNE_GEN_WIDE_LB;
#else
constexpr int kGenWideLB = 2;
#endif
#ifdef ECG_TUNE_GEN_LB
constexpr int kGenLB = ECG_TUNE_GEN_LB;  // GENERAL tiles of 1-4 outputs (tuning builds only)
#else
constexpr int kGenLB = 4;
#endif

}  // namespace ecg
