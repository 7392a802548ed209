// Launch descriptor of the read-only GF(2^8) parity check (scrub_kernels.hip, libecg_scrub.so).
//
//   counts[s * m + p] = number of byte positions x in [0, B) with  XOR_j H[p][j] * in_j[x] != 0
//
// The same tables, tiles and chunk maps as the region product (gf_kernels.hpp GfLaunch); nothing is written
// but the counters, and those only where a check fails.
#pragma once
#include "gf_kernels.hpp"

namespace ecg {

struct ScrubLaunch {
    GfLaunch g;        // tables, source ids / pointers, strides, tile and chunk geometry; its output fields are unused
    unsigned* counts;  // [S][m], zeroed by the caller before the launch
    // Encode-shaped checks, H = [C | I]: g describes C alone (k inputs, tables), and check row q also XORs in the
    // stored block it checks -- block id ident_base + q of the stripe (STRIDED), g.isrc[g.k + q] (INLINE) -- read
    // once, by the row's own tile, with no table fold.  ident = 0: a general H, every column through the tables.
    int ident;
    int ident_base;
};

// Check bytes [0, B) of every stripe.  mode: GF_MODE_INLINE (S == 1) or GF_MODE_STRIDED.  `vec_ok` = every
// block is 16-byte aligned; otherwise the byte kernel covers everything.  Returns a hipError_t.
hipError_t launch_scrub(const ScrubLaunch& base, int mode, bool vec_ok, hipStream_t stream);
// Scrub kernels launched in this process, and the bytes they read as planned (S * B * k per row tile, plus S * B * m
// for the identity part of an encode-shaped check).
void scrub_traffic(long long* launches, long long* bytes);
// Geometry of this process's most recent vector-path launch, as placed in its descriptor after the fallbacks
// (launch_rule.hpp CheckLaunchLog): grid_map, map_group, cols_per_wg, wg_per_stripe, S, rtiles (all zero before the
// first).  Returns the field count; v is written when cap suffices.  A diagnostic for tests: it says which
// workgroup -> chunk map a call ran.
int scrub_last_launch(int* v, int cap);

}  // namespace ecg
