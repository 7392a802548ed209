// Two-block correction for MI355X (gfx950, CDNA4): the heal (heal_kernels.hip) with a second candidate pass over
// pairs of blocks.
//
// Per 16-byte column (byte path: per byte) of a stripe:
//   1. Syndromes, exactly the heal's (check_device.hpp syndromes16 / syndrome_byte): one lane holds all R <= 8
//      syndromes of its column, and one ballot sends a wave with all-zero syndromes on to its next column.  A clean wave
//      column costs what it costs in the heal and the locate.
//   2. Singles: the heal's candidate test over every block, b = 0 .. n-1, with its correction (e = s_p0 / H[p0][b],
//      masked byte-wise, XORed into the lane's own 16 bytes of block b), keeping the per-byte mask of what a single
//      block explained.
//   3. Pairs, only if a ballot finds a lane that still holds a bad byte no single block explained: a uniform loop over
//      the pairs {a < b} of the stripe's family (all of them, or the n - 1 that hold the target).  The host gave every
//      pair two pivot rows p < q with an invertible minor (heal2_kernels.hpp); s_p and s_q are picked with selects on
//      the uniform pivots -- the accumulators are never indexed dynamically, which would put them in scratch -- and one
//      pass over the R rows of the pair's two table columns gives e_a (row p), e_b (row q) and, for every other row, the
//      syndrome the pair predicts.  A byte votes when it is still unexplained and every prediction holds.  Voting lanes
//      mask e_a and e_b byte-wise, reload their own 16 bytes of block a, XOR, store, then the same for block b.
//   4. Counters: n + 3 <= 35 of them in the locate's three statically indexed registers, at most three atomic
//      instructions per wave at the end.
// No LDS, no barrier; vector stores only, and only from lanes whose vote mask is not empty.
//
// One lane may correct the same 16 bytes of a block more than once: a single at byte 0 and a pair at byte 5 of a column,
// or pairs {a, b} at byte 0 and {a, c} at byte 5.  Every correction is a plain load, XOR, plain store of the lane's
// own column in program order, so each sees the one before; a block's column is never kept in registers from one
// candidate to the next.
//
// Workgroups own disjoint chunks of a stripe, lanes disjoint columns: as long as the launch's stripe ids are distinct
// no two lanes read-modify-write the same bytes.
#include "check_device.hpp"
#include "launch_rule.hpp"
#include "heal2_kernels.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "heal2_kernels.hip is gfx950 (CDNA4) code"
#endif

namespace ecg {

namespace {

// The stripe's family, uniform per workgroup: singles over [0, nb) and the pairs that hold `tgt` (tgt < 0: every pair;
// nb == 0: none).
__device__ __forceinline__ void family(const Heal2Launch& ha, int s, int& nb, int& tgt) {
    nb = ha.l.n;
    tgt = -1;
    if (ha.any) return;
    const int t = ha.targets ? cst(ha.targets)[s] : ha.target;
    const bool named = t >= 0 && t < ha.l.n;
    nb = named ? ha.l.n : 0;
    tgt = named ? t : 0;
}

// v[x] ^= e in the bytes of vm, at p: the lane's own 16-byte column (W = 4) or byte (W = 1) of a block.
template <int W>
__device__ __forceinline__ void correct(uint8_t* p, const uint32_t (&e)[W], const uint32_t (&vm)[W]) {
    if constexpr (W == 4) {
        u32x4 x;
        x.x = e[0] & byte_mask(vm[0]);
        x.y = e[1] & byte_mask(vm[1]);
        x.z = e[2] & byte_mask(vm[2]);
        x.w = e[3] & byte_mask(vm[3]);
        u32x4* q = reinterpret_cast<u32x4*>(p);
        *q = *q ^ x;
    } else {
        *p = (uint8_t)(*p ^ (e[0] & byte_mask(vm[0])));
    }
}

// Phase 2: the heal's candidate test (check_device.hpp candidate_loop) over blocks [0, nb) with its correction at byte
// `off`, except that the bad / explained masks go back to the caller, who counts them after the pairs.
template <int R, int W, int MODE>
__device__ __forceinline__ void singles(const Heal2Launch& ha, const uint8_t* sbase, const uint32_t (&syn)[R][W],
                                        long long off, int nb, int lane, unsigned (&mine)[kSlots], uint32_t (&bad)[W],
                                        uint32_t (&expl)[W]) {
    const LocateLaunch& sa = ha.l;
    const ECG_CONST CoefTab* Q = cst(sa.ratios);
    const ECG_CONST CoefTab* I = cst(ha.invlead);
#pragma unroll
    for (int d = 0; d < W; ++d) {
        uint32_t any = syn[0][d];
#pragma unroll
        for (int p = 1; p < R; ++p) any |= syn[p][d];
        bad[d] = nonzero_mask(any);
        expl[d] = 0u;
    }
    for (int b = 0; b < nb; ++b) {  // uniform
        const unsigned p0 = (sa.p0[b >> 3] >> ((b & 7) * 4)) & 15u;
        if (p0 == kNoPivot) continue;  // a zero column explains nothing (the host refuses such a check)
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
        if (v != 0u) {
            uint32_t e[W];
#pragma unroll
            for (int d = 0; d < W; ++d) e[d] = gmul(I[b], split(lead[d]));
            correct<W>(block_ptr<MODE>(sa, sbase, b) + off, e, vm);
        }
    }
}

// Phase 3: the pairs of the family.  Returns this lane's count of bytes corrected as a pair; expl takes them in.
// Only bytes that are bad and that no single block (and no earlier pair) explained may vote.  For such a byte a pair
// that predicts every syndrome has e_a != 0 and e_b != 0 by construction: with e_b == 0 block a alone would explain
// the byte, and phase 2 has tried every block.
template <int R, int W, int MODE>
__device__ __forceinline__ unsigned pairs(const Heal2Launch& ha, const uint8_t* sbase, const uint32_t (&syn)[R][W],
                                          long long off, int tgt, int lane, unsigned (&mine)[kSlots],
                                          const uint32_t (&bad)[W], uint32_t (&expl)[W]) {
    const LocateLaunch& sa = ha.l;
    const ECG_CONST CoefTab* P = cst(ha.pairs);
    const ECG_CONST int* ids = cst(ha.pair_ids);
    const int n = sa.n;
    const int count = tgt < 0 ? ha.npairs : n - 1;
    unsigned np = 0u;
    for (int j = 0; j < count; ++j) {  // uniform
        int i = j;
        if (tgt >= 0) {  // the j-th partner of the target, and the pair's place in the order (0,1), (0,2), ..
            const int o = j + (j >= tgt ? 1 : 0);
            const int lo = min(o, tgt), hi = max(o, tgt);
            i = lo * n - ((lo * (lo + 1)) >> 1) + (hi - lo - 1);
        }
        const unsigned id = (unsigned)ids[2 * i];
        const int a = (int)(id & 255u), b = (int)((id >> 8) & 255u);
        const unsigned p = (id >> 16) & 15u, q = (id >> 24) & 15u;
        const ECG_CONST CoefTab* tp = P + (size_t)(2 * i) * R;
        const ECG_CONST CoefTab* tq = tp + R;
        uint32_t vm[W], ea[W], eb[W];
        unsigned v = 0u;
#pragma unroll
        for (int d = 0; d < W; ++d) {
            uint32_t sp = syn[0][d], sq = syn[0][d];
#pragma unroll
            for (int u = 1; u < R; ++u) {
                sp = p == (unsigned)u ? syn[u][d] : sp;
                sq = q == (unsigned)u ? syn[u][d] : sq;
            }
            const Split xp = split(sp), xq = split(sq);
            uint32_t res = 0u;
            ea[d] = 0u;
            eb[d] = 0u;
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const uint32_t val = gmul(tp[u], xp) ^ gmul(tq[u], xq);
                const bool at_p = p == (unsigned)u, at_q = q == (unsigned)u;
                ea[d] = at_p ? val : ea[d];
                eb[d] = at_q ? val : eb[d];
                res |= (at_p || at_q) ? 0u : (syn[u][d] ^ val);
            }
            vm[d] = bad[d] & ~expl[d] & ~nonzero_mask(res);
            v += (unsigned)__popc(vm[d]);
        }
        if (__ballot(v != 0u) == 0ull) continue;
#pragma unroll
        for (int d = 0; d < W; ++d) expl[d] |= vm[d];
        const unsigned tot = wave_sum(v);
        credit(mine, a, tot, lane);
        credit(mine, b, tot, lane);
        np += v;
        if (v != 0u) {  // block a, then block b: each a reload, an XOR and a store of the lane's own bytes
            correct<W>(block_ptr<MODE>(sa, sbase, a) + off, ea, vm);
            correct<W>(block_ptr<MODE>(sa, sbase, b) + off, eb, vm);
        }
    }
    return np;
}

// Phases 2 to 4 of a dirty wave column at byte `off`.  Every lane of the wave is here (a lane past its chunk comes with
// zero syndromes, votes for nothing and stores nothing): the wave sums read every lane.
template <int R, int W, int MODE>
__device__ __forceinline__ void mend(const Heal2Launch& ha, const uint8_t* sbase, const uint32_t (&syn)[R][W],
                                     long long off, int nb, int tgt, int lane, unsigned (&mine)[kSlots]) {
    uint32_t bad[W], expl[W];
    singles<R, W, MODE>(ha, sbase, syn, off, nb, lane, mine, bad, expl);
    unsigned left = 0u;
#pragma unroll
    for (int d = 0; d < W; ++d) left |= bad[d] & ~expl[d];
    if (nb != 0 && __ballot(left != 0u) != 0ull) {  // sparse single-block damage never comes here
        const unsigned np = pairs<R, W, MODE>(ha, sbase, syn, off, tgt, lane, mine, bad, expl);
        if (__ballot(np != 0u) != 0ull) credit(mine, ha.l.n + 2, wave_sum(np), lane);
    }
    unsigned nbad = 0u, nu = 0u;
#pragma unroll
    for (int d = 0; d < W; ++d) {
        nbad += (unsigned)__popc(bad[d]);
        nu += (unsigned)__popc(bad[d] & ~expl[d]);
    }
    credit(mine, ha.l.n, wave_sum(nbad), lane);
    if (__ballot(nu != 0u) != 0ull) credit(mine, ha.l.n + 1, wave_sum(nu), lane);
}

// Vector path: bytes [0, 16 * floor(B / 16)) of every block; all pointers 16-byte aligned.
// grid.x = S * wg_per_stripe (stripe-major).  The column loop is per wave, so that every lane reaches the wave sums.
template <int R, int MODE>
__global__ void __launch_bounds__(kThreads, occupancy_for(R)) gf_heal2_kernel(const Heal2Launch ha) {
    const LocateLaunch& sa = ha.l;
    const GfLaunch& a = sa.g;
    int s, w;
    wg_coords(a, s, w);
    const uint8_t* sbase = stripe_base<MODE>(a, s);
    int nb, tgt;
    family(ha, s, nb, tgt);
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
        mend<R, 4, MODE>(ha, sbase, acc, off, nb, tgt, lane, mine);
    }
    post_counters(mine, sa.votes + (size_t)s * (size_t)(sa.n + 3), sa.n + 3, lane);
}

// Byte path: bytes [off0, B) (tails, unaligned blocks).  cols_per_wg = bytes per workgroup.
template <int R, int MODE>
__global__ void __launch_bounds__(kThreads) gf_heal2_byte_kernel(const Heal2Launch ha) {
    const LocateLaunch& sa = ha.l;
    const GfLaunch& a = sa.g;
    int s, w;
    wg_coords(a, s, w);
    const long long by0 = a.off0 + (long long)w * a.cols_per_wg;
    const long long by1 = min(by0 + (long long)a.cols_per_wg, a.B);
    const uint8_t* sbase = stripe_base<MODE>(a, s);
    int nb, tgt;
    family(ha, s, nb, tgt);
    const int lane = threadIdx.x & 63;
    unsigned mine[kSlots] = {0u, 0u, 0u};
    for (long long ow = by0 + (threadIdx.x & ~63); ow < by1; ow += kThreads) {
        const long long o = ow + lane;
        uint32_t acc[R][1] = {};
        if (o < by1) syndrome_byte<R, MODE>(sa, sbase, o, acc);
        if (clean_wave(acc)) continue;
        mend<R, 1, MODE>(ha, sbase, acc, o, nb, tgt, lane, mine);
    }
    post_counters(mine, sa.votes + (size_t)s * (size_t)(sa.n + 3), sa.n + 3, lane);
}

// ---------------------------------------------------------------------------------------------
// Dispatch

struct Heal2Kernels {  // launch_rule.hpp candidate_kernel
    template <int R, int MODE, bool BYTE>
    static const void* kernel() {
        if constexpr (BYTE) return (const void*)gf_heal2_byte_kernel<R, MODE>;
        else return (const void*)gf_heal2_kernel<R, MODE>;
    }
};

CheckLaunchLog g_heal2_log;

}  // namespace

void heal2_traffic(long long* launches, long long* bytes) { g_heal2_log.traffic(launches, bytes); }

int heal2_last_launch(int* v, int cap) { return g_heal2_log.last_launch(v, cap); }

hipError_t launch_heal2(const Heal2Launch& base, int mode, bool vec_ok, hipStream_t st) {
    const LocateLaunch& bl = base.l;
    const GfLaunch& b = bl.g;
    if (b.k < 1 || b.m < kHeal2MinR || b.m > kMaxMT || b.MT != b.m || b.rtiles != 1 || b.S < 1 || b.B < 0 ||
        bl.n < 2 || bl.n > kHeal2MaxN || bl.n != b.k + (bl.ident ? b.m : 0) || !bl.votes || !bl.ratios ||
        !base.invlead || !b.tabs || !base.pairs || !base.pair_ids || base.npairs != bl.n * (bl.n - 1) / 2)
        return hipErrorInvalidValue;
    if (mode != GF_MODE_INLINE && mode != GF_MODE_STRIDED) return hipErrorInvalidValue;
    if (mode == GF_MODE_INLINE && (b.S != 1 || base.targets)) return hipErrorInvalidValue;
    if (mode == GF_MODE_STRIDED && !base.any && !base.targets) return hipErrorInvalidValue;
    if (b.B == 0) return hipSuccess;
    Heal2Launch ha = base;
    GfLaunch& a = ha.l.g;
    a.row_split = 0;
    a.prog_of_stripe = nullptr;
    return launch_paths(
        a, vec_ok, g_heal2_log, (long long)a.S * a.B * bl.n, 1,
        [&](dim3 g) { return launch_kernel(candidate_kernel<Heal2Kernels, kHeal2MinR, false>(a.m, mode), ha, g, st); },
        [&](dim3 g) { return launch_kernel(candidate_kernel<Heal2Kernels, kHeal2MinR, true>(a.m, mode), ha, g, st); });
}

}  // namespace ecg
