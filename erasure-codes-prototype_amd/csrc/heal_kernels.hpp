// Launch descriptor of in-place correction (heal_kernels.hip, libecg_heal.so): the locate's pass over the dirty
// stripes, which also XORs the error value back into the block that explains a bad position.
//
// With s[x] = H * v[x] as in locate_kernels.hpp and K the stripe's candidate set (one named block, or every block):
// for every bad x and every b in K with s[x] = e * H[:, b], e != 0, byte x of block b becomes v_b[x] ^ e, where
// e = s_p0[x] / H[p0(b)][b].  Per selected stripe
//   report[b]     = #{ x corrected in block b }                            (b < n)
//   report[n]     = #{ x : s[x] != 0 }                                     (bad positions)
//   report[n + 1] = #{ bad x left untouched }
// The syndrome phase, the chunk maps and the counters are the locate's; only lanes that hold a correction store, and
// only the 16-byte column (byte path: the byte) they hold.
#pragma once
#include "locate_kernels.hpp"

namespace ecg {

struct HealLaunch {
    // The check, the candidate ratios and pivots, and the counters (`votes` is the report), as the locate takes them.
    // The blocks g names are written: the kernels cast the const away.
    LocateLaunch l;
    // 1 / H[p0(b)][b] tables [n][1] (a 1 x n product's tables; a zero column is 0)
    const CoefTab* invlead;
    // Candidate set.  any != 0: every block.  Otherwise one block: targets[i] for launch stripe i (STRIDED, device
    // memory), or `target` when targets is NULL (INLINE).  A value outside [0, n) is the empty set.
    const int* targets;
    int target;
    int any;
};

// Heal over bytes [0, B) of every selected stripe.  mode: GF_MODE_INLINE (S == 1) or GF_MODE_STRIDED.  `vec_ok` =
// every block is 16-byte aligned; otherwise the byte kernel covers everything.  Returns a hipError_t.
hipError_t launch_heal(const HealLaunch& base, int mode, bool vec_ok, hipStream_t stream);
// Heal kernels launched in this process, and the bytes they read as planned (S * B * n: every block once; the bytes
// written depend on the data and are not counted).
void heal_traffic(long long* launches, long long* bytes);
// Geometry of this process's most recent vector-path launch: the six fields of locate_last_launch.
int heal_last_launch(int* v, int cap);

}  // namespace ecg
