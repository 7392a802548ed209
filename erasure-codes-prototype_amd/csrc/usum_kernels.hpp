// Launch descriptor of the update sums (usum_kernels.hip, libecg_usum.so): the recorded CRC-32C of blocks and pieces
// carried through the records of a delta update (update_kernels.hpp) without reading a block.
//
// By the linearity stated in sum_kernels.hpp, a change D on bytes [a, b) of a summed range that ends at e turns its sum
// into  sum ^ raw(D[a..b)) * x^(8 (e - b)).  For a record {stripe, col, off, len, in_off} D is delta, the len bytes at
// delta[in_off ..), for the data block src_ids[col], and G[i][col] * delta byte by byte for parity dst_ids[i]
// (include/ecg_usum.h).  The sum table is sums[S][n_sums][Q]: column c is block sum_ids[c], piece q of a block ends at
// min((q + 1) P, B) (P = piece_bytes; P == 0: one sum per block, Q = 1).
//
// The plan of a column is the update's own: program `col` of the program set update.cpp requests (one source, mt rows,
// tabs[col * mt + p], dst_ids[col * mt + p], -1 past the column's nnz), so both libraries share one cache entry.
#pragma once
#include "sum_kernels.hpp"
#include "update_kernels.hpp"

namespace ecg {

constexpr int kUsumIds = 128;          // columns of a row of the sum table
constexpr int kUsumStreams = 1 + kUpdateMaxNnz;  // delta and its product with each nonzero coefficient
constexpr int kUsumRowBytes = 16 * kThreads;     // one workgroup row: a lane per 16-byte column
constexpr int kUsumLaunchFields = 5;   // cols_per_wg, wg_per_record, R, max_nnz, piece_bytes

enum UsumWhich : int { kUsumData = 1, kUsumParity = 2 };

struct UsumLaunch {
    const CoefTab* tabs;       // [k_in][mt]
    const int* src_ids;        // [k_in]
    const int* dst_ids;        // [k_in][mt], -1 past the column's nnz
    const long long* records;  // [R][5] device memory
    const uint8_t* delta;      // the staging buffer that holds delta
    const unsigned* update_report;  // [R][2] of the update, or nullptr
    unsigned* sums;            // [S][n_sums][Q], XORed into
    unsigned* report;          // [R][2]: state, nonzero
    long long B, max_len, in_bytes;
    long long piece_bytes;     // 0, or a power of two in [512, 2^30]
    long long Q;               // sums per block
    int S, k_in, mt, R, which, n_sums;
    int cols_per_wg;           // 16-byte columns of a block per workgroup, a multiple of kThreads
    int wg_per_record;         // grid.x = R * wg_per_record
    int sum_ids[kUsumIds];     // block id of column c of the table
};

// One launch over R records.  max_nnz: the true maximum (mt = max(max_nnz, 1)).  Returns a hipError_t;
// hipErrorInvalidConfiguration for a grid past 2^31 - 1 workgroups (usum_grid says so before anything is launched).
hipError_t launch_usum(const UsumLaunch& base, int max_nnz, hipStream_t stream);
// The launch geometry for max_len under ECG_OPT_COLS_PER_WG (rounded up to whole workgroup rows): chunks are cut on
// the block's own grid, so a record of max_len bytes meets at most (chunk + max_len - 2) / chunk + 1 of them.  False if
// R * wg_per_record exceeds 2^31 - 1.
bool usum_grid(long long max_len, long long R, int& cols_per_wg, int& wg_per_record);
// Usum kernels launched in this process and the records they covered.
void usum_traffic(long long* launches, long long* records);
// cols_per_wg, wg_per_record, R, max_nnz, piece_bytes of the most recent launch.
int usum_last_launch(int* v, int cap);

}  // namespace ecg
