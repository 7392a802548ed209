// Launch descriptors of named-block restoration (restore_kernels.hip, libecg_restore.so): the heal's pass over the
// selected stripes, with a named SET of blocks per stripe in place of one named block.
//
// With s[x] = H * v[x] as in locate_kernels.hpp and E the stripe's flagged columns, t = |E|: where the stripe is usable
// (1 <= t <= r, H[:, E] of full column rank) every bad x with a solution of H_E * e = s[x] gets v_b[x] ^= e_b for the
// b in E with e_b != 0.  Per selected stripe
//   report[b]     = #{ x corrected in block b }                            (b < n)
//   report[n]     = #{ x : s[x] != 0 }                                     (bad positions)
//   report[n + 1] = #{ bad x left untouched }
//   report[n + 2] = the state (kRestoreUsable .. kRestoreDependent)
//
// The plan of a stripe.  Gauss-Jordan on H_E with row pivoting and no row swaps leaves a row transform T (r x r) with
// T * H_E = the unit vector e_c in pivot row P[c] and 0 in the r - t rows Q that were never a pivot.  So
//   e_c = (T s)[P[c]]        -- row P[c] of T is supported on the pivot rows: it is row c of M = H[P, E]^-1
//   0   = (T s)[q], q in Q   -- row q of T is the unit vector of q plus, on the pivot rows, row q of G = H[Q, E] * M:
//                               the position is consistent iff s_Q = G s_P
// The plan keeps those r rows as one r x r coefficient set A, A[p][i] = T[row(i)][p] with row(i) = P[i] for i < t and
// the rows of Q in ascending order after them, as ready CoefTab entries in the order the fold reads them
// (A[p * r + i]): a dirty lane column folds its r syndromes through A as the syndrome phase folds r inputs, output
// i < t is e of flagged block ids[i] and the outputs i >= t are the residual.  Only r t + (r - t) of the r r entries
// are nonzero; the zeros keep every index of the fold static.
#pragma once
#include "locate_kernels.hpp"

namespace ecg {

enum RestoreState : int {
    kRestoreUsable = 0,     // 1 <= t <= r, H[:, E] independent
    kRestoreNone = 1,       // no block flagged
    kRestoreTooMany = 2,    // t > r
    kRestoreDependent = 3,  // the flagged columns are dependent (a zero column included)
};

struct alignas(32) RestorePlan {
    int state;
    int t;               // flagged blocks (as counted, also when > r)
    int ids[kMaxMT];     // the flagged columns in ascending order (the first min(t, 8)), -1 after them
    int rows[kMaxMT];    // usable: the t pivot rows P[0..t), then the r - t residual rows; -1 after them
    int pad[6];
    CoefTab A[kMaxMT * kMaxMT];  // [p * r + i], see above; entries past r * r are not read
};
static_assert(sizeof(RestorePlan) == 96 + 32 * kMaxMT * kMaxMT, "header of 24 dwords, then the tables");
constexpr int kRestorePlanWords = 24;

// The plan kernel's arguments: one wave per selected stripe turns flags[i][0..n) into plans[i].
struct RestorePlanLaunch {
    const uint8_t* named;  // [S][n], nonzero = flagged
    RestorePlan* plans;    // [S]
    int n, r, S;
    uint8_t H[kMaxMT * kInlineSrc];  // r x n, row-major
};

struct RestoreLaunch {
    // The check and the counters (`votes` is the report, [S][n + 3]) as the locate takes them; ratios and p0 are not
    // read.  The blocks g names are written: the kernels cast the const away.
    LocateLaunch l;
    const RestorePlan* plans;  // STRIDED: [S], device memory written by the plan kernel earlier on the stream
    int post_state;            // this launch adds the state to report[n + 2] (the first launch of a call does)
    RestorePlan inl;           // INLINE: the one stripe's plan, solved on the host
};
static_assert(sizeof(RestoreLaunch) <= 4096, "kernel arguments");

// Plans for S stripes on `stream`.  Returns a hipError_t.
hipError_t launch_restore_plan(const RestorePlanLaunch& p, hipStream_t stream);
// Restore over bytes [0, B) of every selected stripe.  mode: GF_MODE_INLINE (S == 1, base.inl) or GF_MODE_STRIDED
// (base.plans).  `vec_ok` = every block is 16-byte aligned; otherwise the byte kernel covers everything.
hipError_t launch_restore(const RestoreLaunch& base, int mode, bool vec_ok, hipStream_t stream);
// named[i][q][j] = sums[i][j][q] != expected[i][j][q], count[i][q] = the flags set in the row.
hipError_t launch_restore_names(int n, int Q, const unsigned* sums, const unsigned* expected, int S, uint8_t* named,
                                int* count, hipStream_t stream);
// Main kernels launched in this process, and the bytes they read as planned (S * B * n: every block once; the plan
// and names kernels are not counted).
void restore_traffic(long long* launches, long long* bytes);
// Geometry of this process's most recent vector-path launch: the six fields of locate_last_launch.
int restore_last_launch(int* v, int cap);

}  // namespace ecg
