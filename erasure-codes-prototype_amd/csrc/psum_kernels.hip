// Piece checksums for MI355X (gfx950, CDNA4): CRC-32C of every P-byte piece of every block of every selected stripe.
//
//   sums[(i * n + j) * Q + q] = crc32c(piece q of block src_ids[j] of stripe stripe_of[i])      (psum_kernels.hpp)
//
// The arithmetic is that of the block checksums (sum_kernels.hpp); what differs is where a remainder is due.  The block
// kernel folds its lanes once per 256 KiB segment and can afford bit-serial multiplies there; here a fold is due every
// P bytes, so every multiplication on the way is a table: four byte-indexed lookups in a 4 x 256-word LDS table per
// constant (kTables: * x^32, * x^(8 * 16 * 2^d) for d = 0..6, * x^(8 * 2048)), computed at compile time and fetched
// once per workgroup.
//
// A 128-lane workgroup owns one SPAN of one block and reads it in rows of 2 KiB, one non-temporal dwordx4 per lane.
//   * fold of a lane: its four dword states become the remainder of its 16 bytes, ((s0 x^32 ^ s1) x^32 ^ s2) x^32 ^ s3)
//     x^32, four passes through table 0;
//   * fold of G lanes (G = min(P, 1024) / 16, always inside a wave): a tree, level d computing v = T_d(v of the lane
//     2^d to the left) ^ v, after which the group's last lane holds the remainder of the group's 16 G bytes.
// P < 2048 (crc_psum_small_kernel): a row holds 2048 / P pieces, every row is folded, 5 or 6 levels.
// P >= 2048 (crc_psum_rows_kernel): the workgroup walks its span in RUNS, a run being the rows of one piece that lie
// in the span; a run goes down its rows by Horner with the row table, exactly as crc_sum_kernel does, and is folded
// once: 6 levels in either wave, wave 0's remainder times x^(8 * 1024) (level 6) for the half row behind it.  The two
// waves never meet: each XORs its own remainder into the sum.  A run that ends before its piece does (P larger than
// the span, or a span boundary inside a piece) multiplies by x^(8 * bytes to the piece's end) with the power ladder.
// Lanes are aligned to the END of what they fold (the piece's vector part, the run), so missing bytes are zeros in
// FRONT, where they cost nothing: a ragged last piece needs no other code.
// The last B % 16 bytes belong to the last piece: the vector path multiplies that piece's remainder by x^(8 * (B % 16))
// and the byte kernel XORs the tail's own remainder in.  The affine term crc32c(0^len) is per piece (length P, and
// the last piece's own length) and is XORed in by whoever holds the piece's first byte.
// Every contribution is an atomicXor into zeroed sums: exact and reproducible whatever the span.
#include <string.h>

#include "launch_rule.hpp"
#include "psum_device.hpp"
#include "psum_kernels.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "psum_kernels.hip is gfx950 (CDNA4) code"
#endif

namespace ecg {

namespace {

static_assert(kPsumMinPiece % kPsumRunBytes == 0, "a byte-path run never straddles two pieces");

// ---- device pieces (the tables and the folds are psum_device.hpp's)

template <int MODE>
__device__ __forceinline__ const uint8_t* block_ptr(const PsumLaunch& a, int i, int c) {
    if constexpr (MODE == SUM_MODE_INLINE) return a.src.ptrs[c];
    else {
        const long long st = a.stripe_of ? (long long)a.stripe_of[i] : (long long)i;
        return a.base + st * a.sstride + (long long)a.src.ids[c] * a.bstride;
    }
}

// blockIdx.x -> (launch stripe, column of this launch, span): a block's spans are adjacent workgroups
__device__ __forceinline__ void psum_coords(const PsumLaunch& a, int& i, int& c, int& g) {
    const unsigned blk = blockIdx.x / (unsigned)a.segs;
    g = (int)(blockIdx.x % (unsigned)a.segs);
    i = (int)(blk / (unsigned)a.cols);
    c = (int)(blk % (unsigned)a.cols);
}

__device__ __forceinline__ unsigned* sums_of(const PsumLaunch& a, int i, int c) {
    return a.sums + ((size_t)i * a.n + a.col0 + c) * (size_t)a.Q;
}

__device__ __forceinline__ u32x4 load_row(const uint8_t* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}

// Vector path, P < 2048: bytes [0, hi) of every block, hi a multiple of 16, every block 16-byte aligned.
// grid.x = S * cols * segs.  Lane t of a row is lane j = t % G of the row's piece t / G, G = P / 16.
template <int MODE>
__global__ void __launch_bounds__(kThreads) crc_psum_small_kernel(const PsumLaunch a) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[kPsumTablesSmall * kPsumTableWords];
    fetch_tables<kPsumTablesSmall>(tab);
    const int t = threadIdx.x;
    const int G = (int)(a.P >> 4);
    const int j = t & (G - 1);
    const long long sub = (long long)(t / G) * a.P;

    int i, c, g;
    psum_coords(a, i, c, g);
    const uint8_t* p = block_ptr<MODE>(a, i, c);
    unsigned* const out = sums_of(a, i, c);
    const long long s0 = (long long)g * a.span;
    const long long s1 = min(s0 + a.span, a.hi);
    const int T = (int)((s1 - s0 + kPsumRowBytes - 1) / kPsumRowBytes);
    const u32x4 zero = {0u, 0u, 0u, 0u};

    // row r: this lane's piece starts at ps and its vector part ends at pe; the lane reads the 16 bytes that end
    // 16 (G - 1 - j) before pe, or nothing if they lie before ps (a ragged last piece) or the row has no such piece
    auto load = [&](int r) -> u32x4 {
        const long long ps = s0 + (long long)r * kPsumRowBytes + sub;
        const long long o = min(ps + a.P, a.hi) - 16LL * (G - j);
        return (r < T && o >= ps) ? load_row(p + o) : zero;
    };
    u32x4 w0 = load(0), w1 = load(1);
    __syncthreads();  // the tables are in LDS

    for (int r = 0; r < T; ++r) {
        const u32x4 w2 = load(r + 2);
        const uint32_t s[4] = {w0.x, w0.y, w0.z, w0.w};
        uint32_t f = lane_fold(tab, s);
#pragma unroll
        for (int d = 0; d < 5; ++d) f = tree_level(tab, f, d);
        if (G == 64) f = tree_level(tab, f, 5);
        const long long ps = s0 + (long long)r * kPsumRowBytes + sub;
        if (j == G - 1 && ps < a.hi) {
            const long long q = ps / a.P;
            const long long pe = min(ps + a.P, a.hi), te = min(ps + a.P, a.B);
            if (te != pe) f = crc_shift(f, (unsigned long long)(te - pe), a.pw);  // the tail, in the last piece only
            f ^= q == a.Q - 1 ? a.affine_last : a.affine_full;
            atomicXor(out + q, f);
        }
        w0 = w1;
        w1 = w2;
    }
}

// Vector path, P >= 2048 (a multiple of the row): as above, grid.x = S * cols * segs.
template <int MODE>
__global__ void __launch_bounds__(kThreads) crc_psum_rows_kernel(const PsumLaunch a) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[kPsumTablesRows * kPsumTableWords];
    fetch_tables<kPsumTablesRows>(tab);
    const int t = threadIdx.x;

    int i, c, g;
    psum_coords(a, i, c, g);
    const uint8_t* p = block_ptr<MODE>(a, i, c);
    unsigned* const out = sums_of(a, i, c);
    const long long s0 = (long long)g * a.span;
    const long long s1 = min(s0 + a.span, a.hi);
    const u32x4 zero = {0u, 0u, 0u, 0u};
    __syncthreads();  // the tables are in LDS

    for (long long pos = s0; pos < s1;) {
        // the run [pos, b): the rows of piece q inside the span, aligned to b; only row 0 can start before pos
        const long long q = pos / a.P;
        const long long b = min((q + 1) * a.P, s1);
        const int T = (int)((b - pos + kPsumRowBytes - 1) / kPsumRowBytes);
        const long long off = b - (long long)T * kPsumRowBytes + 16 * t;
        const uint8_t* rows = p + off;

        const u32x4 first = off >= pos ? load_row(rows) : zero;
        u32x4 r0 = T > 1 ? load_row(rows + kPsumRowBytes) : zero;
        u32x4 r1 = T > 2 ? load_row(rows + 2 * kPsumRowBytes) : zero;
        uint32_t s[4] = {first.x, first.y, first.z, first.w};
        int r = 1;
        for (; r + 1 < T; r += 2) {
            u32x4 n0 = zero, n1 = zero;
            if (r + 2 < T) n0 = load_row(rows + (long long)(r + 2) * kPsumRowBytes);
            if (r + 3 < T) n1 = load_row(rows + (long long)(r + 3) * kPsumRowBytes);
            row_step(tab, s, r0);
            row_step(tab, s, r1);
            r0 = n0;
            r1 = n1;
        }
        if (r < T) row_step(tab, s, r0);

        uint32_t f = lane_fold(tab, s);
#pragma unroll
        for (int d = 0; d < 6; ++d) f = tree_level(tab, f, d);
        if ((t & 63) == 63) {
            // lane 63 holds the remainder of its wave's 1 KiB of every row; wave 0's has half a row behind it
            if (t < 64) f = tmul(tab + kTabLevel6 * kPsumTableWords, f);
            const long long te = min((q + 1) * a.P, a.B);
            if (te != b) f = crc_shift(f, (unsigned long long)(te - b), a.pw);
            if (t >= 64 && pos == q * a.P) f ^= q == a.Q - 1 ? a.affine_last : a.affine_full;
            atomicXor(out + q, f);
        }
        pos = b;
    }
}

// Byte path: bytes [lo, B) of every block.  span = bytes per workgroup, kPsumRunBytes consecutive bytes per lane.  A
// run lies inside one piece: lo is 0 (runs start at multiples of kPsumRunBytes, which divides P) or the start of the
// tail (fewer than 16 bytes, all of the last piece).
template <int MODE>
__global__ void __launch_bounds__(kThreads) crc_psum_byte_kernel(const PsumLaunch a) {
    int i, c, g;
    psum_coords(a, i, c, g);
    const uint8_t* p = block_ptr<MODE>(a, i, c);
    const long long b0 = a.lo + (long long)g * a.span + (long long)threadIdx.x * kPsumRunBytes;
    const long long b1 = min(b0 + kPsumRunBytes, a.hi);
    if (b0 >= b1) return;
    uint32_t v = 0u;
    for (long long o = b0; o < b1; ++o) {
        v ^= p[o];
#pragma unroll
        for (int b = 0; b < 8; ++b) v = crc_mulx(v);
    }
    const long long q = b0 / a.P;
    const long long ps = q * a.P, te = min(ps + a.P, a.B);
    v = crc_shift(v, (unsigned long long)(te - b1), a.pw);
    if (b0 == ps) v ^= q == a.Q - 1 ? a.affine_last : a.affine_full;  // no vector part holds the piece's first byte
    atomicXor(sums_of(a, i, c) + q, v);
}

// One lane per piece row (i, q), after every sum of the call is complete (the same stream).
__global__ void __launch_bounds__(kThreads) crc_pverify_kernel(const PsumVerify v) {
    const long long row = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (row >= (long long)v.S * v.Q) return;
    const long long i = row / v.Q, q = row % v.Q;
    unsigned bad = 0u;
    int first = -1;
    for (int j = 0; j < v.n; ++j) {
        const size_t at = ((size_t)i * v.n + j) * (size_t)v.Q + (size_t)q;
        if (v.sums[at] != v.expected[at]) {
            if (bad == 0u) first = j;
            ++bad;
        }
    }
    v.bad[row] = bad;
    v.targets[row] = bad > 1u ? v.n : first;
}

// ---------------------------------------------------------------------------------------------
// Dispatch

enum Kind : int { KIND_SMALL, KIND_ROWS, KIND_BYTE };

template <int MODE>
const void* pick_of(int kind) {
    if (kind == KIND_SMALL) return (const void*)crc_psum_small_kernel<MODE>;
    if (kind == KIND_ROWS) return (const void*)crc_psum_rows_kernel<MODE>;
    if (kind == KIND_BYTE) return (const void*)crc_psum_byte_kernel<MODE>;
    return nullptr;
}

const void* pick(int mode, int kind) {
    if (mode == SUM_MODE_INLINE) return pick_of<SUM_MODE_INLINE>(kind);
    if (mode == SUM_MODE_STRIDED) return pick_of<SUM_MODE_STRIDED>(kind);
    return nullptr;
}

LaunchLog<kPsumLaunchFields> g_psum_log;  // the record has this library's own fields (psum_kernels.hpp)

unsigned zeros_sum(long long len) {  // crc32c(0^len)
    return crc_shift(0xFFFFFFFFu, (unsigned long long)len, kCrcPowers.p) ^ 0xFFFFFFFFu;
}

}  // namespace

void psum_traffic(long long* launches, long long* bytes) { g_psum_log.traffic(launches, bytes); }

int psum_last_launch(int* v, int cap) { return g_psum_log.last_launch(v, cap); }

hipError_t launch_psum(int mode, int n, const int* src_ids, const uint8_t* const* ptrs, const void* base,
                       long long sstride, long long bstride, long long B, long long P, const int* d_stripe_of, int S,
                       unsigned* d_sums, bool vec_ok, long long span_bytes, hipStream_t st) {
    if (n < 1 || S < 1 || B < 1 || B >= (1LL << 31) || !d_sums || span_bytes < 0 || span_bytes % kPsumRowBytes != 0 ||
        P < kPsumMinPiece || P > kPsumMaxPiece || (P & (P - 1)) != 0)
        return hipErrorInvalidValue;
    if (mode == SUM_MODE_INLINE ? (S != 1 || n > kPsumPtrs || !ptrs) : (mode != SUM_MODE_STRIDED || !src_ids || !base))
        return hipErrorInvalidValue;
    const long long Q = (B + P - 1) / P;
    if ((long long)S * n * Q >= (1LL << 31)) return hipErrorInvalidValue;
    // the geometry of both paths, the same for every group of columns; the first group is the widest.  A grid past
    // 2^31 - 1 workgroups is refused here, before anything is zeroed, counted or launched.
    const long long vec_bytes = vec_ok ? (B & ~15LL) : 0;
    const int per = mode == SUM_MODE_INLINE ? kPsumPtrs : kPsumIds;
    const int groups = (n + per - 1) / per;
    long long span = 0, vsegs = 0, bpw = 0, bsegs = 0;
    if (vec_bytes > 0) {
        span = span_bytes > 0 ? span_bytes : kPsumAutoSpan;
        const long long rows = (vec_bytes + kPsumRowBytes - 1) / kPsumRowBytes * kPsumRowBytes;
        if (span > rows) span = rows;
        vsegs = (vec_bytes + span - 1) / span;
    }
    if (vec_bytes < B) {
        const long long nbytes = B - vec_bytes;
        bpw = (long long)kPsumRunBytes * kThreads;
        if (nbytes < bpw) bpw = (nbytes + kPsumRunBytes - 1) / kPsumRunBytes * kPsumRunBytes;
        bsegs = (nbytes + bpw - 1) / bpw;
    }
    const long long widest = (long long)S * (n < per ? n : per);
    if (widest * vsegs > 0x7fffffffLL || widest * bsegs > 0x7fffffffLL) return hipErrorInvalidConfiguration;

    if (const hipError_t e = hipMemsetAsync(d_sums, 0, (size_t)S * (size_t)n * (size_t)Q * sizeof(unsigned), st);
        e != hipSuccess)
        return e;

    PsumLaunch a;
    memset(&a, 0, sizeof(a));
    a.base = (const uint8_t*)base;
    a.sstride = sstride;
    a.bstride = bstride;
    a.stripe_of = d_stripe_of;
    a.sums = d_sums;
    a.B = B;
    a.P = P;
    a.Q = Q;
    a.S = S;
    a.n = n;
    for (int j = 0; j < 32; ++j) a.pw[j] = kCrcPowers.p[j];
    a.affine_full = zeros_sum(P);
    a.affine_last = zeros_sum(B - (Q - 1) * P);
    g_psum_log.count(groups * ((vec_bytes > 0) + (vec_bytes < B)), (long long)S * n * B);

    for (int col0 = 0; col0 < n; col0 += per) {
        a.col0 = col0;
        a.cols = n - col0 < per ? n - col0 : per;
        for (int c = 0; c < a.cols; ++c) {
            if (mode == SUM_MODE_INLINE) a.src.ptrs[c] = ptrs[col0 + c];
            else a.src.ids[c] = src_ids[col0 + c];
        }
        const long long blocks = (long long)S * a.cols;
        if (vec_bytes > 0) {
            a.lo = 0;
            a.hi = vec_bytes;
            a.span = span;
            a.segs = (int)vsegs;
            g_psum_log.record({0, (int)P, (int)Q, S * n, (int)span});
            if (const hipError_t e = launch_kernel(pick(mode, P < kPsumRowBytes ? KIND_SMALL : KIND_ROWS), a,
                                                   dim3((unsigned)(blocks * a.segs)), st);
                e != hipSuccess)
                return e;
        }
        if (vec_bytes < B) {
            a.lo = vec_bytes;
            a.hi = B;
            a.span = bpw;
            a.segs = (int)bsegs;
            if (vec_bytes == 0) g_psum_log.record({1, (int)P, (int)Q, S * n, (int)bpw});
            if (const hipError_t e = launch_kernel(pick(mode, KIND_BYTE), a, dim3((unsigned)(blocks * a.segs)), st);
                e != hipSuccess)
                return e;
        }
    }
    return hipSuccess;
}

hipError_t launch_psum_verify(const PsumVerify& v, hipStream_t st) {
    if (v.S < 1 || v.n < 1 || v.Q < 1 || !v.sums || !v.expected || !v.targets || !v.bad) return hipErrorInvalidValue;
    g_psum_log.count(1, 0);
    const long long rows = (long long)v.S * v.Q;
    return launch_kernel((const void*)crc_pverify_kernel, v, dim3((unsigned)((rows + kThreads - 1) / kThreads)), st);
}

}  // namespace ecg
