// Launch descriptor of corruption localisation (locate_kernels.hip, libecg_locate.so): which block of a stripe
// that fails its check is the damaged one?
//
// With s[x] = H * v[x] the r syndrome bytes of byte position x (H: r x n check matrix, r <= kMaxMT), per
// selected stripe
//   votes[b]     = #{ x : s[x] = e * H[:, b] for some e != 0 }            (b < n: the positions block b explains)
//   votes[n]     = #{ x : s[x] != 0 }                                     (bad positions)
//   votes[n + 1] = #{ x : s[x] != 0 and no single block explains x }
// The data path is the scrub's (scrub_kernels.hip): the same tables, loads, chunk maps and the H = [C | I] shortcut;
// nothing is written but the counters, and those only where a syndrome is nonzero.
#pragma once
#include "gf_kernels.hpp"

namespace ecg {

struct LocateLaunch {
    // The check, as in ScrubLaunch: tables [k][R] of the columns that go through them (one row tile, MT = m = R,
    // always the GENERAL flavour), source ids / pointers, strides, chunk geometry.  g.stripe_of is the selection
    // (STRIDED: launch stripe i reads stripe stripe_of[i], NULL = i) and row i of `votes` is its result.
    GfLaunch g;
    unsigned* votes;  // [S][n + 2], zeroed by the caller before the launch
    // H = [C | I]: g describes C alone (g.k = n - R columns) and check row q also XORs in the stored block it
    // checks: block ident_base + q of the stripe (STRIDED), g.isrc[g.k + q] (INLINE).
    int ident;
    int ident_base;
    // Candidate test.  n candidate blocks (the columns of H, in order); ratio tables [n][R] for
    // H[q][b] / H[p0(b)][b], p0(b) the first row with H[p0][b] != 0 (ratio[b][p0] = 1; a zero column is all zero);
    // p0 packed four bits per candidate, 15 for a zero column, which explains nothing.
    const CoefTab* ratios;
    int n;
    unsigned p0[kInlineSrc / 8];
};

constexpr unsigned kNoPivot = 15u;

// Locate over bytes [0, B) of every selected stripe.  mode: GF_MODE_INLINE (S == 1) or GF_MODE_STRIDED.  `vec_ok` =
// every block is 16-byte aligned; otherwise the byte kernel covers everything.  Returns a hipError_t.
hipError_t launch_locate(const LocateLaunch& base, int mode, bool vec_ok, hipStream_t stream);
// Locate kernels launched in this process, and the bytes they read as planned (S * B * n: every block once).
void locate_traffic(long long* launches, long long* bytes);
// Geometry of this process's most recent vector-path launch, as placed in its descriptor after the fallbacks
// (launch_rule.hpp CheckLaunchLog): grid_map, map_group, cols_per_wg, wg_per_stripe, S, rtiles (all zero before the
// first).  Returns the field count; v is written when cap suffices.  A diagnostic for tests: it says which
// workgroup -> chunk map a call ran.
int locate_last_launch(int* v, int cap);

}  // namespace ecg
