// The candidate plan of a check matrix H, shared by the entry points that test "does block b alone explain this
// syndrome?": locate.cpp (libecg_locate.so) and heal.cpp (libecg_heal.so).  Header-only; no HIP launch and no state.
#pragma once
#include <string.h>

#include "check_common.hpp"
#include "gf256.hpp"
#include "locate_kernels.hpp"

namespace ecg {

struct CandidatePlan {
    Check chk;
    LinearOp ratio;  // r x n: H[q][b] / H[p0(b)][b]; an all-zero column for a zero column of H
    unsigned p0[kInlineSrc / 8];
    int n = 0, r = 0;
};

inline CandidatePlan make_plan(int n, int r, const int* H, const int* src_ids, bool consecutive) {
    CandidatePlan pl;
    pl.n = n;
    pl.r = r;
    pl.chk = make_check(n, r, H, src_ids, consecutive);
    pl.ratio.src_ids = iota(n);
    pl.ratio.dst_ids = iota(r);
    pl.ratio.coef.assign((size_t)r * n, 0);
    memset(pl.p0, 0, sizeof(pl.p0));
    for (int b = 0; b < n; b++) {
        int p0 = 0;
        while (p0 < r && (H[(size_t)p0 * n + b] & 0xff) == 0) p0++;
        pl.p0[b >> 3] |= (p0 < r ? (unsigned)p0 : kNoPivot) << ((b & 7) * 4);
        if (p0 == r) continue;
        const int lead = H[(size_t)p0 * n + b] & 0xff;
        for (int q = p0; q < r; q++) pl.ratio.coef[(size_t)q * n + b] = (uint8_t)gf::div(H[(size_t)q * n + b], lead);
    }
    return pl;
}

}  // namespace ecg
