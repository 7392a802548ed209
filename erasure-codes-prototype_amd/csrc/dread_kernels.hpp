// Launch descriptors of the degraded range read (dread_kernels.hip, libecg_dread.so): byte ranges of stored blocks
// answered into a caller buffer, lost blocks rebuilt from the survivors their reconstruction really needs.
//
// A record {stripe, col, off, len, out_off} asks for bytes [off, off + len) of column `col` of one stripe at
// out[out_off ..).  lost[stripe][0..n) flags the stripe's lost columns E.  A column that is not lost is copied; a lost
// one is  out[x] = XOR_{j not in E} c_j * v_j[x]  with c = Plan(H, E, col) (include/ecg_dread.h): Gauss-Jordan over the
// lost columns in ascending order, the pivot of a column the unused row with the fewest nonzeros outside E (ties: the
// lower row) whose eliminated entry is nonzero, w = the transform's row that became col's pivot, c = w * H; the record
// is not recoverable when col found no pivot or w * H is not the unit vector of col on E.
//
// The plan of a record is what the plan kernel leaves in the caller's scratch and the main kernel reads through uniform
// loads: a header {state, reads}, the block ids of the record's `reads` sources (the columns with c_j != 0, in
// ascending column order) and one ready CoefTab per source.  A copy is one source with c = 1.
#pragma once
#include "gf_kernels.hpp"

namespace ecg {

constexpr int kDreadRecordWords = 5;
constexpr int kDreadLaunchFields = 4;  // cols_per_wg, wg_per_record, R, max_reads
constexpr int kDreadHeadWords = 8;     // state, reads, six words of padding: the ids start 32 bytes in

enum DreadState : unsigned {
    kDreadAnswered = 0,
    kDreadBadStripe = 1,      // stripe not in [0, S)
    kDreadBadCol = 2,         // col not in [0, n)
    kDreadBadRange = 3,       // off < 0, len < 0 or off + len > B
    kDreadTooLong = 4,        // len > max_len
    kDreadBadOut = 5,         // out_off < 0 or out_off + len > out_bytes
    kDreadUnrecoverable = 6,  // col is lost and the survivors do not determine it
};

// A record's plan in the scratch: kDreadHeadWords ints, ids_of(n) ints of block ids, n CoefTabs; 32-byte aligned.
constexpr long long dread_ids_words(int n) { return ((long long)n + 7) & ~7LL; }
constexpr long long dread_plan_bytes(int n) {
    return 4 * (kDreadHeadWords + dread_ids_words(n)) + (long long)sizeof(CoefTab) * n;
}

struct DreadLaunch {
    // the strided layout: block b of stripe s at base + s * sstride + b * bstride; never written
    const uint8_t* base;
    long long sstride, bstride;
    const uint8_t* lost;        // [S][n], nonzero = lost
    const long long* records;   // [R][5]
    uint8_t* out;               // out_bytes bytes
    uint8_t* work;              // [R] plans of plan_bytes each
    unsigned* report;           // [R][2]: state, reads
    long long B, max_len, out_bytes, plan_bytes;
    int S, n, r, R;
    int cols_per_wg;    // 16-byte columns of a record per workgroup
    int wg_per_record;  // grid.x = R * wg_per_record
    // the plan kernel only
    int src_ids[kInlineSrc];         // column j is block src_ids[j]
    uint8_t H[kMaxMT * kInlineSrc];  // r x n, row-major
};
static_assert(sizeof(DreadLaunch) <= 4096, "kernel arguments");

// The plan launch (one wave per record) and the main launch over R records, both on `stream`.  `vec_ok` = base and
// strides are 16-byte aligned: full columns then move as 16-byte vectors; otherwise every byte takes the byte lanes
// and the launch is not recorded as a column launch.  max_reads: the columns of H that are not all zero, the most
// sources a record can have.  Returns a hipError_t; hipErrorInvalidConfiguration for a grid past 2^31 - 1 workgroups
// (dread_grid says so before anything is launched).
hipError_t launch_dread(const DreadLaunch& base, bool vec_ok, int max_reads, hipStream_t stream);
// The launch geometry for max_len under ECG_OPT_COLS_PER_WG: false if R * wg_per_record exceeds 2^31 - 1.
bool dread_grid(long long max_len, long long R, int& cols_per_wg, int& wg_per_record);
// Main kernels launched in this process and the records they covered (the plan launches are not counted).
void dread_traffic(long long* launches, long long* records);
// cols_per_wg, wg_per_record, R, max_reads of the most recent launch that covered 16-byte columns.
int dread_last_launch(int* v, int cap);

}  // namespace ecg
