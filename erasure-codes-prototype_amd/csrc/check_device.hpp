// Device-side pieces shared by the kernels over a check matrix H: the scrub (scrub_kernels.hip), the locate
// (locate_kernels.hip), the heal (heal_kernels.hip) and heal2 (heal2_kernels.hip), on top of gf_device.hpp.  Each
// library compiles them into its own code object.  Everything here is inlined into the kernels that use it; the header
// defines no kernel and no host state.
//
//   all four                 fold_inputs (the load-batch ladder), nonzero_mask, wave_sum
//   locate, heal and heal2   the syndrome phase (syndromes16, syndrome_byte, clean_wave), the candidate loop (heal2: in
//                            a copy that keeps the masks), the counters of a wave in three registers (credit,
//                            post_counters) and the block pointers
//   heal and heal2           block_ptr, byte_mask: where and under which mask a correction is written
#pragma once
#include "gf_device.hpp"
#include "locate_kernels.hpp"

namespace ecg {

static_assert(kThreads % 64 == 0, "whole waves");
static_assert(kInlineSrc + 2 <= 3 * 64, "three counter registers per lane hold n + 2 counters");
constexpr int kSlots = 3;

// One bit (bit 7) per nonzero byte of a dword: adding 0x7f to the low 7 bits of a byte carries into its bit 7
// exactly when they are not all zero (no carry leaves the byte), OR-ing x brings in bit 7 itself.
__device__ __forceinline__ uint32_t nonzero_mask(uint32_t x) {
    const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
    return (t | x) & 0x80808080u;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// acc ^= XOR_j T[j][.] * (the 16 bytes at `off` of input j), j < k; ptr(j) is input j's block.  Loads go out in
// batches of LB before they are folded (gf_device.hpp kLoadBatch, kGenWideLB, kGenLB), the rest of k in a batch of
// four, of two, of one.
template <int MT, bool BIN, class Ptr>
__device__ __forceinline__ void fold_inputs(int k, const ECG_CONST CoefTab* T, long long off, uint32_t (&acc)[MT][4],
                                            Ptr ptr) {
    constexpr int LB = BIN ? kLoadBatch : MT >= 5 ? kGenWideLB : kGenLB;
    int j = 0;
    for (; j + LB <= k; j += LB) {
        uint32_t x[LB][4];
#pragma unroll
        for (int u = 0; u < LB; ++u) load16<1>(ptr(j + u) + off, x[u]);
        fold<MT, LB, BIN>(x, T + (size_t)j * MT, acc);
    }
    if constexpr (LB > 4) {
        if (j + 4 <= k) {
            uint32_t x[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) load16<1>(ptr(j + u) + off, x[u]);
            fold<MT, 4, BIN>(x, T + (size_t)j * MT, acc);
            j += 4;
        }
    }
    if constexpr (LB > 2) {
        if (j + 2 <= k) {
            uint32_t x[2][4];
#pragma unroll
            for (int u = 0; u < 2; ++u) load16<1>(ptr(j + u) + off, x[u]);
            fold<MT, 2, BIN>(x, T + (size_t)j * MT, acc);
            j += 2;
        }
    }
    if (j < k) {
        uint32_t x[1][4];
        load16<1>(ptr(j) + off, x[0]);
        fold<MT, 1, BIN>(x, T + (size_t)j * MT, acc);
    }
}

// ---------------------------------------------------------------------------------------------
// Locate, heal and heal2: one lane holds all R syndromes of its column (one row tile, GENERAL flavour).

// Block pointers.  STRIDED: `sbase` is the selected stripe's base, in_base + stripe_of[s] * in_sstride, worked out once
// per workgroup (gf_device.hpp src_ptr tests stripe_of at every load); INLINE: the pointers in the kernel arguments.
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

// the stored block of check row q of H = [C | I] (LocateLaunch::ident), folded in after the C part
template <int MODE>
__device__ __forceinline__ const uint8_t* ident_ptr(const LocateLaunch& sa, const uint8_t* sbase, int q) {
    if constexpr (MODE == GF_MODE_INLINE) return sa.g.isrc[sa.g.k + q];
    else return sbase + (long long)(sa.ident_base + q) * sa.g.in_bstride;
}

// Block b, to be written (heal, heal2): a table column, or -- the last R blocks of an [C | I] check, which the tables
// do not hold -- the stored block of check row b - k.  b is uniform.
template <int MODE>
__device__ __forceinline__ uint8_t* block_ptr(const LocateLaunch& sa, const uint8_t* sbase, int b) {
    const uint8_t* p = b < sa.g.k ? col_ptr<MODE>(sa.g, sbase, b) : ident_ptr<MODE>(sa, sbase, b - sa.g.k);
    return const_cast<uint8_t*>(p);
}

// acc ^= the R syndromes of the 16-byte column at byte `off` of the stripe's blocks (vector path).
template <int R, int MODE>
__device__ __forceinline__ void syndromes16(const LocateLaunch& sa, const uint8_t* sbase, long long off,
                                            uint32_t (&acc)[R][4]) {
    const GfLaunch& a = sa.g;
    fold_inputs<R, false>(a.k, cst(a.tabs), off, acc, [&](int j) { return col_ptr<MODE>(a, sbase, j); });
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

// acc ^= the R syndromes of the byte at `o` of the stripe's blocks, in the low byte of a dword (byte path).
template <int R, int MODE>
__device__ __forceinline__ void syndrome_byte(const LocateLaunch& sa, const uint8_t* sbase, long long o,
                                              uint32_t (&acc)[R][1]) {
    const GfLaunch& a = sa.g;
    const ECG_CONST CoefTab* T = cst(a.tabs);
    for (int j = 0; j < a.k; ++j) {
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

// No lane of the wave holds a nonzero syndrome: one OR-reduce per lane and one ballot.
template <int R, int W>
__device__ __forceinline__ bool clean_wave(const uint32_t (&syn)[R][W]) {
    uint32_t any = 0u;
#pragma unroll
    for (int p = 0; p < R; ++p)
#pragma unroll
        for (int d = 0; d < W; ++d) any |= syn[p][d];
    return __ballot(any != 0u) == 0ull;
}

// 0x80 bits -> 0xff bytes
__device__ __forceinline__ uint32_t byte_mask(uint32_t m) { return (m >> 7) * 0xffu; }

// counter idx += tot, in the lane that owns it: lane i of register j owns counter 64 j + i (idx and tot are uniform)
__device__ __forceinline__ void credit(unsigned (&mine)[kSlots], int idx, unsigned tot, int lane) {
    const unsigned add = lane == (idx & 63) ? tot : 0u;
    const int slot = idx >> 6;
#pragma unroll
    for (int j = 0; j < kSlots; ++j) mine[j] += slot == j ? add : 0u;
}

// The candidate test over the R syndromes of W dwords (W = 4: a 16-byte column; W = 1: one byte in a dword), for the
// candidate blocks [b0, b1) (uniform), counted into mine[]: counter b for the bytes block b explains, n for the bad
// bytes, n + 1 for the bad bytes no candidate explains.  Every lane of the wave is here (a lane past its chunk comes
// with zero syndromes and votes for nothing): the wave sums read every lane.  A lane that votes for b then calls
// on_vote(b, lead, vm): lead = its W dwords of s_p0, vm = one 0x80 bit per byte that voted.
template <int R, int W, class OnVote>
__device__ __forceinline__ void candidate_loop(const LocateLaunch& sa, const uint32_t (&syn)[R][W], int b0, int b1,
                                               int lane, unsigned (&mine)[kSlots], OnVote on_vote) {
    const ECG_CONST CoefTab* Q = cst(sa.ratios);
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
        if (p0 == kNoPivot) continue;  // a zero column explains nothing
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
        if (v != 0u) on_vote(b, lead, vm);
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

// A wave's counters -> out[0, ncount): one atomic instruction per register that holds a nonzero counter.
__device__ __forceinline__ void post_counters(const unsigned (&mine)[kSlots], unsigned* out, int ncount, int lane) {
    if (__ballot((mine[0] | mine[1] | mine[2]) != 0u) == 0ull) return;
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
        const int idx = j * 64 + lane;
        if (idx < ncount && mine[j] != 0u) atomicAdd(out + idx, mine[j]);
    }
}

}  // namespace ecg
