// Update sums for MI355X (gfx950, CDNA4): the recorded CRC-32C of blocks and pieces carried through the records of a
// delta update.  Only delta, the records and the sum table are touched; no block is read (usum_kernels.hpp).
//
// One kernel, crc_usum_kernel<NR>.  grid.x = R * wg_per_record, linear: workgroup b takes chunk b % wg_per_record of
// record b / wg_per_record, counted from the chunk that holds the record's first byte.  Chunks lie on the BLOCK's own
// grid (multiples of 16 * cols_per_wg bytes, whole rows of kThreads 16-byte columns), so a row of 2 KiB lies in one
// piece when P >= 2 KiB (or P == 0) and holds 2 or 4 whole pieces when P is 1 KiB or 512: a row is cut into SEGMENTS
// of min(P, 2 KiB) bytes, 32, 64 or 128 adjacent lanes each, and a segment never crosses a piece border.
// The record and its column's plan are uniform per workgroup and read through the constant address space; a refused
// record has its state written by lane 0 of its first workgroup and nothing else is read or written.
//
// A lane takes the 16 bytes of its column that lie in the record's range (a full column through one unaligned 16-byte
// load, a partial one byte by byte, zero elsewhere: delta IS zero outside the range), forms 1 + nnz streams (delta, and
// gmul per nonzero coefficient), and reduces each stream's four dwords to one 32-bit value with Horner through the
// x^32 step tables in LDS (kStepTables, 4 x 256 x 4 B, fetched once per workgroup): 12 lookups per stream.  One generic
// multiply by kLaneMul[columns to the segment's end] puts the value in place; XOR shuffles (and, for 128-lane
// segments, one exchange through LDS) fold a segment.  The bytes between the segment's end and the piece's end are one
// factor x^(8 d) per segment: lane j of a 32-lane group takes x^(8 * 2^j) if bit j of d is set and five shuffled
// multiplies give the product.  Lane p of a segment multiplies stream p by it and issues the one atomicXor of
// (workgroup row, segment, stream).  XOR commutes: the table is exact whatever the grid or the order.
// A block whose size is no multiple of 16 ends in a short column; its lane stands for the bytes [B - 16, B) with the
// column's bytes at their places in that window (leading zeros cost nothing), needs no factor and posts its own atomics.
// `nonzero` is counted per lane, summed per wave and added with one vector atomic per wave.  No scalar memory writes.
#include "check_device.hpp"
#include "launch_rule.hpp"
#include "usum_kernels.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "usum_kernels.hip is gfx950 (CDNA4) code"
#endif

namespace ecg {

namespace {

static_assert(kThreads == 128, "a row is two waves; segments are 32, 64 or 128 lanes");
static_assert(kUsumStreams <= 32, "lane p of a segment finishes stream p");

typedef u32x4 u32x4_unaligned __attribute__((aligned(1)));

// ---- compile-time tables

constexpr uint32_t kX32 = crc_shift(kCrcOne, 4, kCrcPowers.p);

// t[b * 256 + v] = (v << 8 b) * x^32: the four byte tables of the dword step.  Linear in v.
struct StepTables {
    uint32_t t[4 * 256];
};
constexpr StepTables make_step_tables() {
    StepTables r{};
    for (int b = 0; b < 4; ++b)
        for (int v = 1; v < 256; ++v) {
            const int low = v & -v;
            r.t[b * 256 + v] = v == low ? crc_mul((uint32_t)v << (8 * b), kX32)
                                        : r.t[b * 256 + (v ^ low)] ^ r.t[b * 256 + low];
        }
    return r;
}

// d[i] = x^(128 i + 32): i columns after this one, and the x^32 that turns the sum of words into a remainder.
struct LaneMul {
    uint32_t d[kThreads];
};
constexpr LaneMul make_lane_mul() {
    LaneMul r{};
    const uint32_t step = crc_shift(kCrcOne, 16, kCrcPowers.p);
    r.d[0] = kX32;
    for (int i = 1; i < kThreads; ++i) r.d[i] = crc_mul(r.d[i - 1], step);
    return r;
}

__device__ const StepTables kStepTables = make_step_tables();
__device__ const LaneMul kLaneMul = make_lane_mul();
__device__ const CrcPowers kLadder = kCrcPowers;

// ---- device pieces

// s * x^32 through the tables
__device__ __forceinline__ uint32_t step32(const uint32_t* tab, uint32_t s) {
    return tab[s & 0xffu] ^ tab[256 + ((s >> 8) & 0xffu)] ^ tab[512 + ((s >> 16) & 0xffu)] ^ tab[768 + (s >> 24)];
}

// w0 x^96 ^ w1 x^64 ^ w2 x^32 ^ w3
__device__ __forceinline__ uint32_t horner16(const uint32_t* tab, const uint32_t (&w)[4]) {
    uint32_t s = step32(tab, w[0]) ^ w[1];
    s = step32(tab, s) ^ w[2];
    return step32(tab, s) ^ w[3];
}

__device__ __forceinline__ uint32_t shfl_x(uint32_t v, int o) { return (uint32_t)__shfl_xor((int)v, o, 64); }

template <int NR>
__global__ void __launch_bounds__(kThreads) crc_usum_kernel(const UsumLaunch a) {
    constexpr int NS = 1 + NR;
    __shared__ __attribute__((aligned(16))) uint32_t tab[4 * 256];
    __shared__ uint32_t part[kThreads / 64][NS];
    __shared__ int scol[NS];
    const int t = threadIdx.x;
    const long long wg = blockIdx.x;
    const long long r = wg / a.wg_per_record;
    const long long w = wg - r * a.wg_per_record;
    const ECG_CONST long long* rec = cst(a.records) + r * kUpdateRecordWords;
    const long long stripe = rec[0], col = rec[1], off = rec[2], len = rec[3], in_off = rec[4];
    unsigned state = kUpdateApplied;
    if (a.update_report) state = cst(a.update_report)[2 * r];
    if (state != kUpdateApplied) {
    } else if (stripe < 0 || stripe >= a.S) state = kUpdateBadStripe;
    else if (col < 0 || col >= a.k_in) state = kUpdateBadCol;
    else if (off < 0 || len < 0 || off > a.B || len > a.B - off) state = kUpdateBadRange;
    else if (len > a.max_len) state = kUpdateTooLong;
    else if (in_off < 0 || in_off > a.in_bytes || len > a.in_bytes - in_off) state = kUpdateBadStaging;
    if (state != kUpdateApplied) {  // uniform
        if (w == 0 && t == 0) a.report[2 * r] = state;
        return;
    }
    const long long end = off + len;
    const long long chunk = 16LL * a.cols_per_wg;
    const long long c0 = (off / chunk + w) * chunk;
    const long long lo = max(off, c0), hi = min(end, c0 + chunk);
    if (lo >= hi) return;  // the chunk lies past the record's end (or the record is empty)

    const ECG_CONST CoefTab* T = cst(a.tabs) + col * NR;

    // stream p's column of the sum table, -1 if `which` leaves it out or no sum is recorded for its block
    if (t < NS) {
        const int id = t == 0 ? a.src_ids[col] : a.dst_ids[col * NR + (t - 1)];
        const bool wanted = t == 0 ? (a.which & kUsumData) != 0 : (a.which & kUsumParity) != 0 && id >= 0;
        int c = -1;
        if (wanted)
            for (int j = 0; j < a.n_sums; ++j) c = a.sum_ids[j] == id ? j : c;
        scol[t] = c;
    }
#pragma unroll
    for (int e = 4 * t; e < 4 * 256; e += 4 * kThreads)
        *reinterpret_cast<u32x4*>(tab + e) = *reinterpret_cast<const u32x4*>(kStepTables.t + e);
    __syncthreads();
    // bit p: stream p has a column (uniform, one SGPR); the lane that finishes stream p keeps its column
    int mask = 0;
#pragma unroll
    for (int p = 0; p < NS; ++p) mask |= scol[p] >= 0 ? 1 << p : 0;
    const int active = __builtin_amdgcn_readfirstlane(mask);

    const long long P = a.piece_bytes;
    const long long seg = (P == 0 || P > kUsumRowBytes) ? kUsumRowBytes : P;
    const int segcols = (int)(seg >> 4);  // 32, 64 or 128
    const int pshift = P ? __builtin_ctzll((unsigned long long)P) : 0;
    const long long Bv = a.B & ~15LL;
    const long long stage = in_off - off;  // staging index of block byte x: stage + x
    const int j32 = t & 31, jseg = t & (segcols - 1);
    const int at = jseg < NS ? scol[jseg] : -1;
    const uint32_t ladder = kLadder.p[j32];
    unsigned nonzero = 0u;

    for (long long xr = lo & ~(long long)(kUsumRowBytes - 1); xr < hi; xr += kUsumRowBytes) {  // uniform
        const long long x0 = xr + 16 * t;
        const long long cend = min(x0 + 16, a.B);
        const long long blo = max(x0, lo), bhi = min(cend, hi);
        uint32_t d[4] = {0u, 0u, 0u, 0u};
        if (bhi - blo == 16) {
            const u32x4 v = *reinterpret_cast<const u32x4_unaligned*>(a.delta + (stage + x0));
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        } else if (blo < bhi) {
            const long long wb = cend - 16;  // the lane's window: [x0, x0 + 16), or [B - 16, B) for the short column
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const long long x = wb + i;
                if (x >= blo && x < bhi) d[i >> 2] |= (uint32_t)a.delta[stage + x] << (8 * (i & 3));
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) nonzero += (unsigned)__popc(nonzero_mask(d[q]));

        // the lane's segment and piece
        const long long send = (x0 & ~(seg - 1)) + seg;
        const long long ev = min(send, Bv);  // where the segment's whole columns end
        const long long q = P ? x0 >> pshift : 0;
        const long long e = P ? min((q + 1) << pshift, a.B) : a.B;
        const bool own = x0 >= ev;           // the short last column (or a lane past the block: it holds zeros)
        const uint32_t mul = kLaneMul.d[own ? 0 : (int)((ev - x0 - 16) >> 4)];
        unsigned* const word = a.sums + ((size_t)stripe * a.n_sums * a.Q + (size_t)(q < a.Q ? q : 0));

        uint32_t g[NS];
#pragma unroll
        for (int p = 0; p < NS; ++p) g[p] = 0u;
        if (__ballot((d[0] | d[1] | d[2] | d[3]) != 0u) != 0ull) {  // per wave
            if (active & 1) g[0] = crc_mul(horner16(tab, d), mul);
            Split sp[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) sp[i] = split(d[i]);
#pragma unroll
            for (int p = 0; p < NR; ++p)
                if ((active >> (1 + p)) & 1) {
                    const uint32_t m[4] = {gmul(T[p], sp[0]), gmul(T[p], sp[1]), gmul(T[p], sp[2]), gmul(T[p], sp[3])};
                    g[1 + p] = crc_mul(horner16(tab, m), mul);
                }
        }
        if (own) {
#pragma unroll
            for (int p = 0; p < NS; ++p) {
                if (g[p] != 0u) atomicXor(word + (size_t)scol[p] * a.Q, g[p]);  // nonzero: the stream is active
                g[p] = 0u;
            }
        }
        // fold the segment
#pragma unroll
        for (int p = 0; p < NS; ++p) {
            if (!((active >> p) & 1)) continue;
#pragma unroll
            for (int o = 1; o <= 16; o <<= 1) g[p] ^= shfl_x(g[p], o);
            if (segcols >= 64) g[p] ^= shfl_x(g[p], 32);
        }
        if (segcols == 128) {  // uniform
            if ((t & 63) == 0) {
#pragma unroll
                for (int p = 0; p < NS; ++p) part[t >> 6][p] = g[p];
            }
            __syncthreads();
#pragma unroll
            for (int p = 0; p < NS; ++p) g[p] = part[0][p] ^ part[1][p];
            __syncthreads();
        }
        // x^(8 (e - ev)), the same for every lane of a segment
        const long long dist = e - ev;
        uint32_t m = kCrcOne;
        if (__ballot(dist != 0) != 0ull) {  // per wave
            m = ((dist >> j32) & 1) ? ladder : kCrcOne;
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) m = crc_mul(m, shfl_x(m, o));
        }
        uint32_t mine = 0u;
#pragma unroll
        for (int p = 0; p < NS; ++p) mine = jseg == p ? g[p] : mine;
        if (__ballot(mine != 0u) != 0ull) {
            const uint32_t v = crc_mul(mine, m);
            if (at >= 0 && v != 0u) atomicXor(word + (size_t)at * a.Q, v);
        }
    }
    const unsigned total = wave_sum(nonzero);  // every lane of the wave is here: the exits above are uniform
    if ((t & 63) == 0 && total != 0u) atomicAdd(a.report + 2 * r + 1, total);
}

LaunchLog<kUsumLaunchFields> g_usum_log;

}  // namespace

void usum_traffic(long long* launches, long long* records) { g_usum_log.traffic(launches, records); }

int usum_last_launch(int* v, int cap) { return g_usum_log.last_launch(v, cap); }

bool usum_grid(long long max_len, long long R, int& cols_per_wg, int& wg_per_record) {
    long long cpw = get_option(ECG_OPT_COLS_PER_WG);
    if (cpw <= 0) cpw = kThreads;
    if (cpw > (1LL << 20)) cpw = 1LL << 20;
    cpw = (cpw + kThreads - 1) / kThreads * kThreads;
    cols_per_wg = (int)cpw;
    const long long chunk = 16 * cpw;
    // a record of max_len bytes that starts at the last byte of a chunk
    const long long wpr = max_len < 1 ? 1 : (chunk + max_len - 2) / chunk + 1;
    wg_per_record = (int)wpr;
    return R * wpr <= 0x7fffffffLL;
}

hipError_t launch_usum(const UsumLaunch& base, int max_nnz, hipStream_t st) {
    const long long P = base.piece_bytes;
    if (base.R < 1 || base.k_in < 1 || base.mt < 1 || base.mt > kUpdateMaxNnz || max_nnz > base.mt || base.B < 0 ||
        base.B >= (1LL << 31) || base.max_len < 0 || base.in_bytes < 0 || !base.tabs || !base.src_ids ||
        !base.dst_ids || !base.records || !base.delta || !base.sums || !base.report || base.n_sums < 1 ||
        base.n_sums > kUsumIds || base.which < 1 || base.which > 3 ||
        (P != 0 && (P < 512 || P > (1LL << 30) || (P & (P - 1)) != 0)) ||
        base.Q != (P == 0 ? 1 : (base.B + P - 1) / P))
        return hipErrorInvalidValue;
    UsumLaunch a = base;
    if (!usum_grid(a.max_len, a.R, a.cols_per_wg, a.wg_per_record)) return hipErrorInvalidConfiguration;
    const void* kernel = pick_of8<1, const void*>(a.mt, nullptr, [&](auto n) -> const void* {
        return (const void*)crc_usum_kernel<decltype(n)::value>;
    });
    g_usum_log.count(1, a.R);
    g_usum_log.record({a.cols_per_wg, a.wg_per_record, a.R, max_nnz, (int)P});
    return launch_kernel(kernel, a, dim3((unsigned)((long long)a.R * a.wg_per_record)), st);
}

}  // namespace ecg
