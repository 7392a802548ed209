// Verified range read for MI355X (gfx950, CDNA4): byte ranges of stored blocks answered into a caller buffer, lost
// blocks rebuilt from the survivors, and the CRC-32C of every piece a record touches compared with the recorded one.
// Nothing of the stripes is written.  Three launches on one stream:
//
//   gf_vread_plan_kernel     one wave per record: the plan wave of vread_plan_device.hpp (a null d.lost = nothing lost).
//   gf_vread_small_kernel    P < 2048   \  grid.x = R * wg_per_record, linear: workgroup b takes span b % wg_per_record of
//   gf_vread_rows_kernel     P >= 2048  /  the COVER of record b / wg_per_record.  These are psum_kernels.hip's two vector
//       kernels with the block replaced by the record's cover [q0 P, min((q1 + 1) P, B)) and its vector part
//       [q0 P, hv), hv = min(cover end, B & ~15): where psum loads a lane's 16 bytes, a lane here folds the 16-byte
//       column over the record's sources (check_device.hpp fold_inputs through the plan's CoefTabs, read through the
//       constant address space as in gf_dread_kernel) and, where the column meets [off, off + len), stores to out as
//       dread stores: a full column by one unaligned 16-byte store, the range's partial first and last column byte by
//       byte.  The rest of the cover lives in registers.  Lane folds, tree levels, row Horner steps, the shift to the
//       piece's end and the affine terms are psum's (psum_device.hpp); contributions are atomicXor into the zeroed
//       sums[record][q - q0], exact whatever the span.  The record and its plan are uniform per workgroup; a refused
//       or empty record, and a workgroup whose span lies past the cover, exit after those loads.  The last B % 16 bytes
//       of a block belong to its last piece: lane 0 of the record's first workgroup takes them as a byte run.
//   gf_vread_byte_kernel     layouts whose base or strides are not 16-byte aligned: the same grid, every span of a
//       cover in byte runs of kPsumRunBytes per lane (crc_psum_byte_kernel's run, over folded bytes).  Slow, correct.
//   gf_vread_verdict_kernel  one lane per record, after every sum is complete: compares the record's sums with
//       expected[stripe][col][q0 ..] and writes the report {state, reads, bad, first_bad}.
// LDS holds the CRC tables only; no private segment; vector stores and vector atomics only.
#include <stddef.h>
#include <string.h>

#include "check_device.hpp"
#include "launch_rule.hpp"
#include "psum_device.hpp"
#include "vread_kernels.hpp"
#include "vread_plan_device.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "vread_kernels.hip is gfx950 (CDNA4) code"
#endif

namespace ecg {

namespace {

static_assert(offsetof(VreadLaunch, d) == 0, "the plan wave reads H and src_ids at DreadLaunch's offsets");
static_assert(kPsumMinPiece % kPsumRunBytes == 0, "a byte run never straddles two pieces");

typedef u32x4 u32x4_unaligned __attribute__((aligned(1)));

__global__ void __launch_bounds__(64) gf_vread_plan_kernel(const VreadLaunch a) { dread_plan_wave(a.d); }

// ---------------------------------------------------------------------------------------------
// The main kernels

// What a workgroup knows of its record; uniform.
struct Work {
    const ECG_CONST int* ids;      // the plan's sources
    const ECG_CONST CoefTab* T;
    const uint8_t* sbase;          // the record's stripe
    int reads;
    long long off, end, shift;     // the range [off, end) of the block; answer index of block byte x: shift + x
    long long q0, cs, ce;          // the cover [cs, ce), from piece q0
    long long w;                   // this workgroup's span of the cover starts at cs + w * span
    unsigned* sums;                // the record's row
};

// False: the workgroup has nothing to do (a refused or empty record, or a span past the cover's end).
__device__ __forceinline__ bool vread_work(const VreadLaunch& a, Work& k) {
    const DreadLaunch& d = a.d;
    const long long wg = blockIdx.x;
    const long long r = wg / d.wg_per_record;
    k.w = wg - r * d.wg_per_record;
    const ECG_CONST int* head = (const ECG_CONST int*)cst((const uint8_t*)d.work + r * d.plan_bytes);
    if ((unsigned)head[0] != kDreadAnswered) return false;  // uniform: nothing of a refused record is read or written
    k.reads = head[1];
    const ECG_CONST long long* rec = cst(d.records) + r * kDreadRecordWords;
    const long long len = rec[3];
    if (len == 0) return false;  // no piece covered
    k.off = rec[2];
    k.end = k.off + len;
    k.shift = rec[4] - k.off;
    k.q0 = k.off / a.P;
    k.cs = k.q0 * a.P;
    k.ce = min(((k.end - 1) / a.P + 1) * a.P, d.B);
    if (k.cs + k.w * a.span >= k.ce) return false;
    k.ids = head + kDreadHeadWords;
    k.T = (const ECG_CONST CoefTab*)(k.ids + dread_ids_words(d.n));
    k.sbase = d.base + rec[0] * d.sstride;
    k.sums = a.sums + r * a.NP;
    return true;
}

// The 16-byte column at byte o of the record's block: folded over the sources, and what of it lies in the range stored.
__device__ __forceinline__ u32x4 column(const VreadLaunch& a, const Work& k, long long o) {
    const long long bstride = a.d.bstride;
    const uint8_t* const sbase = k.sbase;
    const ECG_CONST int* const ids = k.ids;
    uint32_t acc[1][4] = {{0u, 0u, 0u, 0u}};
    fold_inputs<1, false>(k.reads, k.T, o, acc, [&](int j) { return sbase + (long long)ids[j] * bstride; });
    u32x4 v;
    v.x = acc[0][0], v.y = acc[0][1], v.z = acc[0][2], v.w = acc[0][3];
    const long long lo = max(o, k.off), hi = min(o + 16, k.end);
    if (hi - lo == 16) {
        *reinterpret_cast<u32x4_unaligned*>(a.d.out + (k.shift + o)) = v;
    } else if (hi > lo) {
        uint8_t* const out = a.d.out + (k.shift + o);
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (o + i >= lo && o + i < hi) out[i] = (uint8_t)((acc[0][i >> 2] >> (8 * (i & 3))) & 0xffu);
    }
    return v;
}

// Bytes [lo, hi) of the record's block in runs of kPsumRunBytes per lane, a run inside one piece: every byte folded
// over the sources, stored if it lies in the range, and the run's remainder shifted to its piece's end.
__device__ __forceinline__ void byte_runs(const VreadLaunch& a, const Work& k, long long lo, long long hi) {
    for (long long b0 = lo + (long long)threadIdx.x * kPsumRunBytes; b0 < hi; b0 += (long long)kThreads * kPsumRunBytes) {
        const long long b1 = min(b0 + kPsumRunBytes, hi);
        uint32_t v = 0u;
        for (long long o = b0; o < b1; ++o) {
            uint32_t x = 0u;
            for (int j = 0; j < k.reads; ++j)
                x ^= gmul(k.T[j], split((uint32_t)(k.sbase + (long long)k.ids[j] * a.d.bstride)[o]));
            x &= 0xffu;
            if (o >= k.off && o < k.end) a.d.out[k.shift + o] = (uint8_t)x;
            v ^= x;
#pragma unroll
            for (int b = 0; b < 8; ++b) v = crc_mulx(v);
        }
        const long long q = b0 / a.P;
        const long long ps = q * a.P, te = min(ps + a.P, a.d.B);
        v = crc_shift(v, (unsigned long long)(te - b1), a.pw);
        if (b0 == ps) v ^= q == a.Q - 1 ? a.affine_last : a.affine_full;  // no vector part holds the piece's first byte
        atomicXor(k.sums + (q - k.q0), v);
    }
}

// The tail of a block whose cover reaches it, by the record's first workgroup.
__device__ __forceinline__ void tail_run(const VreadLaunch& a, const Work& k) {
    const long long vb = a.d.B & ~15LL;
    if (k.w == 0 && k.ce == a.d.B && vb < a.d.B) byte_runs(a, k, vb, a.d.B);
}

// P < 2048.  Lane t of a row is lane j = t % G of the row's piece t / G, G = P / 16.
__global__ void __launch_bounds__(kThreads) gf_vread_small_kernel(const VreadLaunch a) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[kPsumTablesSmall * kPsumTableWords];
    Work k;
    if (!vread_work(a, k)) return;
    fetch_tables<kPsumTablesSmall>(tab);
    const int t = threadIdx.x;
    const int G = (int)(a.P >> 4);
    const int j = t & (G - 1);
    const long long sub = (long long)(t / G) * a.P;
    const long long hv = min(k.ce, a.d.B & ~15LL);
    const long long s0 = k.cs + k.w * a.span;
    const long long s1 = min(s0 + a.span, hv);
    const u32x4 zero = {0u, 0u, 0u, 0u};
    __syncthreads();  // the tables are in LDS

    // row r: this lane's piece starts at ps and its vector part ends at pe; the lane folds the 16 bytes that end
    // 16 (G - 1 - j) before pe, or nothing if they lie before ps (a ragged last piece) or the row has no such piece
    for (long long row = s0; row < s1; row += kPsumRowBytes) {
        const long long ps = row + sub;
        const long long o = min(ps + a.P, hv) - 16LL * (G - j);
        const u32x4 w = o >= ps ? column(a, k, o) : zero;
        const uint32_t s[4] = {w.x, w.y, w.z, w.w};
        uint32_t f = lane_fold(tab, s);
#pragma unroll
        for (int d = 0; d < 5; ++d) f = tree_level(tab, f, d);
        if (G == 64) f = tree_level(tab, f, 5);
        if (j == G - 1 && ps < hv) {
            const long long q = ps / a.P;
            const long long pe = min(ps + a.P, hv), te = min(ps + a.P, a.d.B);
            if (te != pe) f = crc_shift(f, (unsigned long long)(te - pe), a.pw);  // the tail, in the last piece only
            f ^= q == a.Q - 1 ? a.affine_last : a.affine_full;
            atomicXor(k.sums + (q - k.q0), f);
        }
    }
    tail_run(a, k);
}

// P >= 2048 (a multiple of the row): the workgroup walks its span in runs, a run being the rows of one piece that lie
// in the span, aligned to the run's end.
__global__ void __launch_bounds__(kThreads) gf_vread_rows_kernel(const VreadLaunch a) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[kPsumTablesRows * kPsumTableWords];
    Work k;
    if (!vread_work(a, k)) return;
    fetch_tables<kPsumTablesRows>(tab);
    const int t = threadIdx.x;
    const long long hv = min(k.ce, a.d.B & ~15LL);
    const long long s0 = k.cs + k.w * a.span;
    const long long s1 = min(s0 + a.span, hv);
    const u32x4 zero = {0u, 0u, 0u, 0u};
    __syncthreads();  // the tables are in LDS

    for (long long pos = s0; pos < s1;) {
        const long long q = pos / a.P;
        const long long b = min((q + 1) * a.P, s1);
        const int T = (int)((b - pos + kPsumRowBytes - 1) / kPsumRowBytes);
        const long long o0 = b - (long long)T * kPsumRowBytes + 16 * t;  // only row 0 can start before pos
        const u32x4 first = o0 >= pos ? column(a, k, o0) : zero;
        uint32_t s[4] = {first.x, first.y, first.z, first.w};
        for (int r = 1; r < T; ++r) row_step(tab, s, column(a, k, o0 + (long long)r * kPsumRowBytes));

        uint32_t f = lane_fold(tab, s);
#pragma unroll
        for (int d = 0; d < 6; ++d) f = tree_level(tab, f, d);
        if ((t & 63) == 63) {
            // lane 63 holds the remainder of its wave's 1 KiB of every row; wave 0's has half a row behind it
            if (t < 64) f = tmul(tab + kTabLevel6 * kPsumTableWords, f);
            const long long te = min((q + 1) * a.P, a.d.B);
            if (te != b) f = crc_shift(f, (unsigned long long)(te - b), a.pw);
            if (t >= 64 && pos == q * a.P) f ^= q == a.Q - 1 ? a.affine_last : a.affine_full;
            atomicXor(k.sums + (q - k.q0), f);
        }
        pos = b;
    }
    tail_run(a, k);
}

__global__ void __launch_bounds__(kThreads) gf_vread_byte_kernel(const VreadLaunch a) {
    Work k;
    if (!vread_work(a, k)) return;
    const long long s0 = k.cs + k.w * a.span;
    byte_runs(a, k, s0, min(s0 + a.span, k.ce));
}

// ---------------------------------------------------------------------------------------------
// The verdict

__global__ void __launch_bounds__(kThreads) gf_vread_verdict_kernel(const VreadLaunch a) {
    const DreadLaunch& d = a.d;
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= d.R) return;
    const int* head = reinterpret_cast<const int*>(d.work + r * d.plan_bytes);
    unsigned state = (unsigned)head[0], reads = 0u, bad = 0u, first = kVreadNoPiece;
    if (state == kDreadAnswered) {
        reads = (unsigned)head[1];
        const long long* rec = d.records + r * kDreadRecordWords;
        const long long off = rec[2], len = rec[3];
        if (len > 0) {
            const long long q0 = off / a.P, q1 = (off + len - 1) / a.P;
            const unsigned* want = a.expected + ((size_t)rec[0] * d.n + (size_t)rec[1]) * (size_t)a.Q + q0;
            const unsigned* got = a.sums + r * a.NP;
            for (long long p = 0; p <= q1 - q0; ++p) {
                if (got[p] != want[p]) {
                    if (bad == 0u) first = (unsigned)(q0 + p);
                    ++bad;
                }
            }
        }
        if (bad != 0u) state = kVreadMismatch;
    }
    unsigned* rep = d.report + r * kVreadReportWords;
    rep[0] = state;
    rep[1] = reads;
    rep[2] = bad;
    rep[3] = first;
}

LaunchLog<kVreadLaunchFields> g_vread_log;

unsigned zeros_sum(long long len) {  // crc32c(0^len)
    return crc_shift(0xFFFFFFFFu, (unsigned long long)len, kCrcPowers.p) ^ 0xFFFFFFFFu;
}

}  // namespace

void vread_traffic(long long* launches, long long* records) { g_vread_log.traffic(launches, records); }

int vread_last_launch(int* v, int cap) { return g_vread_log.last_launch(v, cap); }

bool vread_grid(long long max_len, long long P, long long B, long long R, long long span_bytes, long long& NP,
                long long& span, int& wg_per_record) {
    NP = vread_max_pieces(max_len, P, B);
    long long cover = NP * P < B ? NP * P : B;  // the largest cover
    if (cover < 1) cover = 1;
    span = span_bytes > 0 ? span_bytes : kPsumAutoSpan;
    const long long rows = (cover + kPsumRowBytes - 1) / kPsumRowBytes * kPsumRowBytes;
    if (span > rows) span = rows;
    const long long wpr = (cover + span - 1) / span;
    wg_per_record = (int)wpr;
    return R * wpr <= 0x7fffffffLL;
}

hipError_t launch_vread(const VreadLaunch& base, bool vec_ok, long long span_bytes, hipStream_t st) {
    const DreadLaunch& d = base.d;
    if (d.R < 1 || d.n < 1 || d.n > kInlineSrc || d.r < 1 || d.r > kMaxMT || d.S < 0 || d.B < 0 || d.max_len < 0 ||
        d.out_bytes < 0 || !d.base || !d.records || !d.out || !d.work || !d.report || !base.expected || !base.sums ||
        base.P < kPsumMinPiece || (base.P & (base.P - 1)) != 0 || span_bytes < 0 || span_bytes % kPsumRowBytes != 0)
        return hipErrorInvalidValue;
    VreadLaunch a = base;
    a.d.plan_bytes = dread_plan_bytes(d.n);
    a.d.cols_per_wg = 0;
    a.Q = d.B > 0 ? (d.B + a.P - 1) / a.P : 1;
    if (!vread_grid(d.max_len, a.P, d.B, d.R, span_bytes, a.NP, a.span, a.d.wg_per_record))
        return hipErrorInvalidConfiguration;
    for (int j = 0; j < 32; ++j) a.pw[j] = kCrcPowers.p[j];
    a.affine_full = zeros_sum(a.P);
    a.affine_last = zeros_sum(d.B - (a.Q - 1) * a.P);
    void* argv[] = {(void*)&a};
    if (const hipError_t e = hipLaunchKernel((const void*)gf_vread_plan_kernel, dim3((unsigned)d.R), dim3(64), argv, 0, st);
        e != hipSuccess)
        return e;
    if (a.NP > 0) {  // max_len == 0: no record covers a piece
        const void* kernel = !vec_ok                 ? (const void*)gf_vread_byte_kernel
                             : a.P < kPsumRowBytes ? (const void*)gf_vread_small_kernel
                                                     : (const void*)gf_vread_rows_kernel;
        g_vread_log.count(1, d.R);
        g_vread_log.record({vec_ok ? 0 : 1, (int)(a.P > 0x7fffffffLL ? 0x7fffffffLL : a.P), (int)a.NP, (int)a.span,
                            a.d.wg_per_record, d.R});
        if (const hipError_t e = launch_kernel(kernel, a, dim3((unsigned)((long long)d.R * a.d.wg_per_record)), st);
            e != hipSuccess)
            return e;
    }
    return launch_kernel((const void*)gf_vread_verdict_kernel, a, dim3((unsigned)((d.R + kThreads - 1) / kThreads)), st);
}

}  // namespace ecg
