// Launch descriptors of the verified range read (vread_kernels.hip, libecg_vread.so): the degraded range read of
// dread_kernels.hpp -- records, lost flags, plan rule and plan layout are those, not restated -- that also takes the
// CRC-32C of every piece its records touch and compares it with the store's recorded table.
//
// An answered record with len > 0 COVERS pieces q0 = off / P .. q1 = (off + len - 1) / P of its block, bytes
// [q0 P, min((q1 + 1) P, B)).  The main kernel computes column `col` over the whole cover (a copy, or the fold over the
// plan's sources), stores bytes [off, off + len) of it to out and XORs the CRC-32C of every covered piece into
// sums[record][q - q0]; the verdict kernel compares those with expected[stripe][col][q] and writes the report
// {state, reads, bad, first_bad}: state 7 when a covered piece differs.  Block sums (piece_bytes 0 at the C ABI) are
// the case P >= B: one piece, Q = 1.
#pragma once
#include "dread_kernels.hpp"
#include "psum_kernels.hpp"

namespace ecg {

constexpr unsigned kVreadMismatch = 7;       // answered, and a covered piece's sum differs from the recorded one
constexpr unsigned kVreadNoPiece = 0xFFFFFFFFu;
constexpr int kVreadReportWords = 4;         // state, reads, bad, first_bad
constexpr int kVreadLaunchFields = 6;        // path, piece_bytes, max_pieces, span_bytes, wg_per_record, R

struct VreadLaunch {
    DreadLaunch d;             // first: the plan wave finds H and src_ids at DreadLaunch's offsets in the arguments.
                               // d.lost may be null (nothing lost); d.report is [R][4]; d.cols_per_wg is not used
    const unsigned* expected;  // [S][n][Q], only read
    unsigned* sums;            // [R][NP], zeroed by the caller before the launch; XORed into
    long long P, Q;            // the kernels' piece: piece_bytes, or with block sums the power of two >= max(B, 512)
    long long NP;              // columns of a row of `sums`
    long long span;            // bytes of a cover per workgroup: a multiple of kPsumRowBytes
    unsigned affine_full, affine_last;  // crc32c(0^P); crc32c(0^(B - (Q - 1) P)), the last piece's
    uint32_t pw[32];           // kCrcPowers
};
static_assert(sizeof(VreadLaunch) <= 4096, "kernel arguments");

// The kernels' piece for piece_bytes at the C ABI (0 = block sums).
constexpr long long vread_piece(long long piece_bytes, long long B) {
    if (piece_bytes != 0) return piece_bytes;
    long long P = kPsumMinPiece;
    while (P < B) P <<= 1;
    return P;
}
// The most pieces of P bytes a range of len bytes inside a block of B bytes can cover.
constexpr long long vread_max_pieces(long long len, long long P, long long B) {
    if (len <= 0) return 0;
    const long long Q = (B + P - 1) / P, most = len == 1 ? 1 : (len - 2) / P + 2;
    return most < Q ? most : Q;
}

// The launch geometry for max_len: NP, the span (span_bytes, 0 = kPsumAutoSpan, cut down to the largest cover) and the
// workgroups per record.  False if R * wg_per_record exceeds 2^31 - 1.
bool vread_grid(long long max_len, long long P, long long B, long long R, long long span_bytes, long long& NP,
                long long& span, int& wg_per_record);
// The plan launch, the main launch and the verdict launch over d.R records on `stream`; sums and report are zeroed by
// the caller, on the stream, before.  `base` has d, expected, sums and P filled in; the rest is worked out here.
// vec_ok = base and strides are 16-byte aligned; otherwise every byte takes the byte kernel.  Returns a hipError_t.
hipError_t launch_vread(const VreadLaunch& base, bool vec_ok, long long span_bytes, hipStream_t stream);
// Main kernels launched in this process and the records they covered.
void vread_traffic(long long* launches, long long* records);
// path (0 vector, 1 byte), piece_bytes, max_pieces, span_bytes, wg_per_record, R of the most recent main launch.
int vread_last_launch(int* v, int cap);

}  // namespace ecg
