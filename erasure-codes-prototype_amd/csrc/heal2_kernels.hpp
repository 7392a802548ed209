// Launch descriptor of two-block correction (heal2_kernels.hip, libecg_heal2.so): the heal's pass over the dirty
// stripes (heal_kernels.hpp), which also corrects a bad position that no single block explains but a PAIR of blocks
// does.
//
// With s[x] = H * v[x] as in locate_kernels.hpp and F the stripe's family of admissible sets (every single block, and
// every pair -- or every pair that holds the named block): for every bad x and A = {a} or {a, b} in F with
// s[x] = XOR_{a in A} e_a * H[:, a], every e_a != 0, byte x of block a becomes v_a[x] ^ e_a.  Per selected stripe
//   report[b]     = #{ x corrected in block b }, a pair counted in both of its blocks   (b < n)
//   report[n]     = #{ x : s[x] != 0 }                                                 (bad positions)
//   report[n + 1] = #{ bad x left untouched }
//   report[n + 2] = #{ x corrected as a pair }
// The syndrome phase, the chunk maps and the counters are the locate's; only lanes that hold a correction store, and
// only the 16-byte column (byte path: the byte) they hold.
#pragma once
#include "locate_kernels.hpp"

namespace ecg {

constexpr int kHeal2MaxN = 32;  // blocks: the pair tables grow with n (n - 1) / 2 <= 496
constexpr int kHeal2MinR = 3;   // a pair plus one row to test it against

struct Heal2Launch {
    // The check, the single-block ratios and pivots, and the counters (`votes` is the report, [S][n + 3]), as the
    // locate takes them.  The blocks g names are written: the kernels cast the const away.
    LocateLaunch l;
    // 1 / H[p0(b)][b] tables [n][1], as HealLaunch::invlead
    const CoefTab* invlead;
    // Pair tables [2 * npairs][R].  Pair i = {a < b}, in the order (0,1), (0,2), .., (n-2,n-1), has pivot rows p < q
    // whose 2 x 2 minor of (H[:, a], H[:, b]) is invertible; the syndromes of a position that the pair explains are
    // all determined by s_p and s_q.  Column 2 i multiplies s_p, column 2 i + 1 multiplies s_q, and row u of the two
    // gives
    //   u == p          e_a, the error value of block a
    //   u == q          e_b, the error value of block b
    //   any other row   the s_u the pair predicts.
    const CoefTab* pairs;
    // [2 * npairs]: entry 2 i packs pair i as a | b << 8 | p << 16 | q << 24 (entry 2 i + 1 repeats it)
    const int* pair_ids;
    // The family.  any != 0: every single block and every pair.  Otherwise the stripe's target t is targets[i] for
    // launch stripe i (STRIDED, device memory), or `target` when targets is NULL (INLINE): every single block and every
    // pair that holds t -- or, for a t outside [0, n), nothing at all.
    const int* targets;
    int target;
    int any;
    int npairs;  // n (n - 1) / 2
};

// Heal over bytes [0, B) of every selected stripe.  mode: GF_MODE_INLINE (S == 1) or GF_MODE_STRIDED.  `vec_ok` =
// every block is 16-byte aligned; otherwise the byte kernel covers everything.  Returns a hipError_t.
hipError_t launch_heal2(const Heal2Launch& base, int mode, bool vec_ok, hipStream_t stream);
// Kernels launched in this process, and the bytes they read as planned (S * B * n: every block once; what a correction
// reads again and writes depends on the data and is not counted).
void heal2_traffic(long long* launches, long long* bytes);
// Geometry of this process's most recent vector-path launch: the six fields of locate_last_launch.
int heal2_last_launch(int* v, int cap);

}  // namespace ecg
