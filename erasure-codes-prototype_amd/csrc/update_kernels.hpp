// Launch descriptor of the delta update (update_kernels.hip, libecg_update.so): small overwrites applied to data and
// parity in place.
//
// A record {stripe, col, off, len, in_off} names bytes [off, off + len) of data block src_ids[col] of one stripe and
// len input bytes at in[in_off ..).  WRITE: delta = data ^ in, data = in; DELTA: delta = in.  Then, for the rows i with
// G[i][col] != 0, parity dst_ids[i] ^= G[i][col] * delta over the same range (include/ecg_update.h).
//
// The plan of a column is what a workgroup reads through uniform loads: program `col` of a program set with one
// source (the column's data block), mt "rows" -- the column's nonzero coefficients in row order, as ready CoefTab
// entries, tabs[col * mt + p] -- and mt destination ids, dst_ids[col * mt + p], -1 after the column's nnz.  mt is the
// most nonzero coefficients any column has (at least 1) and the kernels' template argument.
#pragma once
#include "gf_kernels.hpp"

namespace ecg {

constexpr int kUpdateMaxNnz = 8;  // nonzero coefficients per column: one lane holds that many parity columns
constexpr int kUpdateRecordWords = 5;
constexpr int kUpdateLaunchFields = 4;  // cols_per_wg, wg_per_record, R, max_nnz

enum UpdateMode : int { kUpdateWrite = 0, kUpdateDelta = 1 };

enum UpdateState : unsigned {
    kUpdateApplied = 0,
    kUpdateBadStripe = 1,   // stripe not in [0, S)
    kUpdateBadCol = 2,      // col not in [0, k_in)
    kUpdateBadRange = 3,    // off < 0, len < 0 or off + len > B
    kUpdateTooLong = 4,     // len > max_len
    kUpdateBadStaging = 5,  // in_off < 0 or in_off + len > in_bytes
};

struct UpdateLaunch {
    const CoefTab* tabs;  // [k_in][mt]
    const int* src_ids;   // [k_in]
    const int* dst_ids;   // [k_in][mt], -1 past the column's nnz
    // the strided layout (records != nullptr): block b of stripe s at base + s * sstride + b * bstride
    uint8_t* base;
    long long sstride, bstride;
    const long long* records;  // [R][5] device memory, or nullptr: the one record `rec` on the blocks idata / ipar
    const uint8_t* in;         // the staging buffer
    uint8_t* delta_out;        // WRITE: delta at the record's staging range, or nullptr
    unsigned* report;          // [R][2]: state, changed
    long long B, max_len, in_bytes;
    int S, k_in, mt, mode, R;
    int cols_per_wg;    // 16-byte columns of a record per workgroup
    int wg_per_record;  // grid.x = R * wg_per_record
    // the single-record form
    long long rec[kUpdateRecordWords];
    uint8_t* idata;                 // the record's data block
    uint8_t* ipar[kUpdateMaxNnz];   // the parity blocks of the column's nonzero rows, in row order
};

// One launch over R records.  `vec_ok` = base and strides (or every block pointer) are 16-byte aligned: full columns
// then move as 16-byte vectors; otherwise every byte takes the byte lanes and the launch is not recorded as a column
// launch.  max_nnz: the true maximum (mt = max(max_nnz, 1)).  Returns a hipError_t; hipErrorInvalidConfiguration for a
// grid past 2^31 - 1 workgroups (update_grid says so before anything is launched).
hipError_t launch_update(const UpdateLaunch& base, bool vec_ok, int max_nnz, hipStream_t stream);
// The launch geometry for max_len under ECG_OPT_COLS_PER_WG: false if R * wg_per_record exceeds 2^31 - 1.
bool update_grid(long long max_len, long long R, int& cols_per_wg, int& wg_per_record);
// Update kernels launched in this process and the records they covered.
void update_traffic(long long* launches, long long* records);
// cols_per_wg, wg_per_record, R, max_nnz of the most recent launch that covered 16-byte columns.
int update_last_launch(int* v, int cap);

}  // namespace ecg
