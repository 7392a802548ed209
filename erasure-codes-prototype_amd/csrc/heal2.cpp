// extern "C" entry points declared in include/ecg_heal2.h (libecg_heal2.so): the host side of two-block correction.
// A call reads four table sets, all LinearOps kept by the engine's program cache (Engine::program_set), so that the
// cache, ensure_ready, note_launch and retirement cover them alike: the check, the single-block ratios and the pivot
// inverses, the heal's own plan (candidate_plan.hpp make_heal_plan), and the pair tables: one op of r rows over 2 * n (n - 1) / 2 <= 992
// "sources", two per pair, whose source ids carry the pair's blocks and pivot rows (heal2_kernels.hpp).  program_set
// puts no bound on an op's sources, and r <= 8 rows are one row tile whatever the coefficients: one op holds them all.
#include <string.h>

#include <string>
#include <vector>

#include "../../include/ecg_heal2.h"
#include "candidate_plan.hpp"
#include "capi_handle.hpp"
#include "check_common.hpp"
#include "engine.hpp"
#include "gf256.hpp"
#include "heal2_kernels.hpp"

using namespace ecg;

namespace {

// ---- k-wise independence of the columns of H, by Gaussian elimination

// A set of columns in echelon form: vector i has a 1 in its pivot row and 0 in the pivot rows of the vectors before it.
struct Echelon {
    uint8_t v[4][kMaxMT];
    int piv[4];
};

// Column c of H reduced against vectors [0, depth) and stored as vector `depth`: false if nothing is left of it.
bool extend(Echelon& e, int depth, int n, int r, const int* H, int c) {
    uint8_t w[kMaxMT];
    for (int p = 0; p < r; p++) w[p] = (uint8_t)(H[(size_t)p * n + c] & 0xff);
    for (int i = 0; i < depth; i++) {
        const int f = w[e.piv[i]];
        if (f)
            for (int p = 0; p < r; p++) w[p] ^= (uint8_t)gf::mul(f, e.v[i][p]);
    }
    int piv = 0;
    while (piv < r && !w[piv]) piv++;
    if (piv == r) return false;
    const int s = gf::inv(w[piv]);
    for (int p = 0; p < r; p++) e.v[depth][p] = (uint8_t)gf::mul(s, w[p]);
    e.piv[depth] = piv;
    return true;
}

// The first (in lexicographic order) linearly dependent set of at most `kwise` columns: its size, the columns in
// set[], or 0 when every `kwise` columns are independent.  At most C(32, 4) = 35 960 sets of rank <= 4.
int dependent_set(int n, int r, const int* H, int kwise, int depth, int from, Echelon& e, int* set) {
    if (depth == kwise) return 0;
    for (int c = from; c < n; c++) {
        set[depth] = c;
        if (!extend(e, depth, n, r, H, c)) return depth + 1;
        if (const int found = dependent_set(n, r, H, kwise, depth + 1, c + 1, e, set)) return found;
    }
    return 0;
}

// ANY2 needs every 4 columns independent, TARGET2 every 3 (include/ecg_heal2.h: the explanation is then unique).
int find_dependent(int n, int r, const int* H, bool any) {
    Echelon e;
    int set[4];
    const int kwise = any ? 4 : 3;
    int found = 0;
    for (int c = 0; c < n && !found; c++) {  // a zero column first: it is the better message
        set[0] = c;
        if (!extend(e, 0, n, r, H, c)) found = 1;
    }
    if (!found) found = dependent_set(n, r, H, kwise, 0, 0, e, set);
    if (!found) return ECG_OK;
    std::string cols;
    for (int i = 0; i < found; i++) cols += (i ? (i + 1 == found ? " and " : ", ") : "") + std::to_string(set[i]);
    set_last_error(std::string("heal2: column") + (found > 1 ? "s " : " ") + cols + " of the check matrix " +
                   (found > 1 ? "are linearly dependent" : "is zero") + " (r = " + std::to_string(r) + "): " +
                   (any ? "ANY2 needs every 4 columns independent" : "TARGET2 needs every 3 columns independent") +
                   (any ? "; name one block with d_targets, which needs every 3" : ""));
    return ECG_EINVAL;
}

// ECG_OK, or the refusal of a shape the pair pass is not built for.
int check_shape(long long n, long long r) {
    if (r >= kHeal2MinR && r <= kMaxMT && n >= 2 && n <= kHeal2MaxN) return ECG_OK;
    set_last_error("heal2: r = " + std::to_string(r) + ", n = " + std::to_string(n) + " is outside " +
                   std::to_string(kHeal2MinR) + " <= r <= " + std::to_string(kMaxMT) + ", 2 <= n <= " +
                   std::to_string(kHeal2MaxN) + " (a pair needs a third row to be tested against; the pair tables " +
                   "grow with n (n - 1) / 2)");
    return ECG_EINVAL;
}

// ---- the plan

struct Heal2Plan {
    HealPlan heal;   // candidate_plan.hpp: the check, the single-block ratios and the pivot inverses, as the heal's
    LinearOp pairs;  // r x (2 * npairs): heal2_kernels.hpp Heal2Launch::pairs; src_ids are the packed pairs
    int npairs = 0;
};

// H has passed check_independent: no zero column, and every two columns have an invertible 2 x 2 minor.
Heal2Plan make_heal2_plan(int n, int r, const int* H, const int* src_ids, bool consecutive) {
    Heal2Plan hp;
    hp.heal = make_heal_plan(n, r, H, src_ids, consecutive);
    hp.npairs = n * (n - 1) / 2;
    const size_t cols = 2 * (size_t)hp.npairs;
    hp.pairs.src_ids.assign(cols, 0);
    hp.pairs.dst_ids = iota(r);
    hp.pairs.coef.assign((size_t)r * cols, 0);
    auto h = [&](int p, int b) { return H[(size_t)p * n + b] & 0xff; };
    size_t i = 0;
    for (int a = 0; a < n; a++)
        for (int b = a + 1; b < n; b++, i++) {
            int p = 0, q = 0, det = 0;  // the first rows p < q with an invertible minor of (h_a, h_b)
            for (p = 0; p < r && !det; p++)
                for (q = p + 1; q < r && !det; q++) det = gf::mul(h(p, a), h(q, b)) ^ gf::mul(h(p, b), h(q, a));
            p--;
            q--;
            // e_a = A s_p ^ B s_q,  e_b = C s_p ^ D s_q
            const int di = gf::inv(det);
            const int A = gf::mul(h(q, b), di), Bq = gf::mul(h(p, b), di), C = gf::mul(h(q, a), di),
                      D = gf::mul(h(p, a), di);
            for (int u = 0; u < r; u++) {
                // every other row: s_u = h_a[u] e_a ^ h_b[u] e_b
                int cp = gf::mul(h(u, a), A) ^ gf::mul(h(u, b), C), cq = gf::mul(h(u, a), Bq) ^ gf::mul(h(u, b), D);
                if (u == p) cp = A, cq = Bq;
                if (u == q) cp = C, cq = D;
                hp.pairs.coef[(size_t)u * cols + 2 * i] = (uint8_t)cp;
                hp.pairs.coef[(size_t)u * cols + 2 * i + 1] = (uint8_t)cq;
            }
            const int id = a | b << 8 | p << 16 | q << 24;
            hp.pairs.src_ids[2 * i] = hp.pairs.src_ids[2 * i + 1] = id;
        }
    return hp;
}

// The calling thread's last check matrix with what was worked out for it: a store heals with one code, call after
// call, and neither the <= 35 960 ranks nor the pair tables' coefficients need to be redone for it.
struct LastCheck {
    std::vector<int> H;
    int n = 0, r = 0;
    int verdict[2] = {-1, -1};  // [any]: -1 not asked yet, 0 accepted, 1 refused
    std::string refusal[2];
    // the plan of the last (src_ids, consecutive); ids is empty before the first
    std::vector<int> ids;
    bool consecutive = false;
    Heal2Plan plan;
};

LastCheck& last_check(int n, int r, const int* H) {
    thread_local LastCheck c;
    const size_t cells = (size_t)n * r;
    if (c.n != n || c.r != r || c.H.size() != cells || memcmp(c.H.data(), H, cells * sizeof(int)) != 0) {
        c = LastCheck();
        c.n = n;
        c.r = r;
        c.H.assign(H, H + cells);
    }
    return c;
}

// The verdict on H for a family, worked out once; a refusal is replayed word for word.
int check_independent(LastCheck& c, bool any) {
    if (c.verdict[any] < 0) {
        c.verdict[any] = find_dependent(c.n, c.r, c.H.data(), any) == ECG_OK ? 0 : 1;
        if (c.verdict[any]) c.refusal[any] = last_error_string();
    }
    if (!c.verdict[any]) return ECG_OK;
    set_last_error(c.refusal[any]);
    return ECG_EINVAL;
}

// The plan of H over these blocks: the same check over the same blocks needs no new one.
const Heal2Plan& cached_plan(LastCheck& c, const int* src_ids, bool consecutive) {
    if (c.consecutive != consecutive || c.ids.size() != (size_t)c.n ||
        memcmp(c.ids.data(), src_ids, (size_t)c.n * sizeof(int)) != 0) {
        c.plan = make_heal2_plan(c.n, c.r, c.H.data(), src_ids, consecutive);
        c.ids.assign(src_ids, src_ids + c.n);
        c.consecutive = consecutive;
    }
    return c.plan;
}

// ---- the launch

// The locate's launch descriptor with the n + 3 counters of the report zeroed (candidate_plan.hpp prepare_launch, which
// fetches the pivot inverses' and the pairs' tables with the others), the family on top of it, then the launch.  `fill`
// sets the launch's sources.
template <class Fill>
int run_heal2(const Heal2Plan& hp, int mode, long long B, int S, const int* d_stripe_ids, const int* d_targets,
              int target, bool any, unsigned* d_report, bool vec_ok, hipStream_t st, Fill fill) {
    Heal2Launch h;
    CandidateTables t;
    if (const int rc = prepare_launch(hp.heal.cand, {&hp.heal.inv, &hp.pairs}, hp.heal.cand.n + 3, B, S, d_stripe_ids,
                                      d_report, "hipMemsetAsync(heal2 report)", st, fill, h.l, t);
        rc != ECG_OK)
        return rc;
    h.invlead = t.extra(0).d_tabs;
    h.pairs = t.extra(1).d_tabs;
    h.pair_ids = t.extra(1).d_src;
    h.npairs = hp.npairs;
    h.targets = d_targets;
    h.target = target;
    h.any = any ? 1 : 0;
    if (const hipError_t e = launch_heal2(h, mode, vec_ok, st); e != hipSuccess) return hip_fail(e, "launch_heal2");
    t.note_launch(st);
    return ECG_OK;
}

// The strided forms after their own argument checks: the independence refusal, the no-op, the launch.
int run_strided_heal2(int n, int r, const int* H, const int* src_ids, void* d_base, long long sstride,
                      long long bstride, long long B, const int* d_stripe_ids, const int* d_targets, int S,
                      unsigned* d_report, hipStream_t st) {
    LastCheck& c = last_check(n, r, H);
    if (const int rc = check_independent(c, d_targets == nullptr); rc != ECG_OK) return rc;
    if (S == 0 || B == 0) return ECG_OK;
    const StridedSrc src{d_base, sstride, bstride};
    return run_heal2(cached_plan(c, src_ids, true), GF_MODE_STRIDED, B, S, d_stripe_ids, d_targets, -1,
                     d_targets == nullptr, d_report, src.vec_ok(), st, src);
}

}  // namespace

extern "C" {

int ecg_heal2_matrix_batch(int n, int r, const int* H, const int* src_ids, void* d_base, long long sstride,
                           long long bstride, long long B, const int* d_stripe_ids, const int* d_targets, int S_sel,
                           unsigned* d_report, void* stream) {
    if (n < 1 || r < 1 || bad_sizes(B, S_sel) || !H || !src_ids || !d_base || !d_report) return ECG_EINVAL;
    if (const int rc = check_shape(n, r); rc != ECG_OK) return rc;
    return run_strided_heal2(n, r, H, src_ids, d_base, sstride, bstride, B, d_stripe_ids, d_targets, S_sel, d_report,
                             (hipStream_t)stream);
}

int ecg_heal2_encode_batch(int k, int m, const int* matrix, void* d_stripes, long long sstride, long long bstride,
                           long long B, const int* d_stripe_ids, const int* d_targets, int S_sel, unsigned* d_report,
                           void* stream) {
    if (k < 1 || m < 1 || bad_sizes(B, S_sel) || !matrix || !d_stripes || !d_report) return ECG_EINVAL;
    if (const int rc = check_shape((long long)k + m, m); rc != ECG_OK) return rc;
    const std::vector<int> H = encode_check(k, m, matrix), ids = iota(k + m);
    return run_strided_heal2(k + m, m, H.data(), ids.data(), d_stripes, sstride, bstride, B, d_stripe_ids, d_targets,
                             S_sel, d_report, (hipStream_t)stream);
}

int ecg_heal2_ec_batch(ecg_ec* ec, void* d_stripes, long long sstride, long long bstride, long long B,
                       const int* d_stripe_ids, const int* d_targets, int S_sel, unsigned* d_report, void* stream) {
    if (!ec || bad_sizes(B, S_sel) || !d_stripes || !d_report || ec->impl->mem != ECG_MEM_DEVICE) return ECG_EINVAL;
    std::vector<int> H;
    int n, r;
    if (const int rc = ec_check(ec, check_shape, H, n, r); rc != ECG_OK) return rc;
    const std::vector<int> ids = iota(n);
    return run_strided_heal2(n, r, H.data(), ids.data(), d_stripes, sstride, bstride, B, d_stripe_ids, d_targets,
                             S_sel, d_report, (hipStream_t)stream);
}

int ecg_heal2_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size, int target,
                 unsigned* d_report) {
    if (!ec || block_size < 0 || !d_data_ptrs || !d_coding_ptrs || !d_report || ec->impl->mem != ECG_MEM_DEVICE)
        return ECG_EINVAL;
    std::vector<int> H;
    int n, r;
    if (const int rc = ec_check(ec, check_shape, H, n, r); rc != ECG_OK) return rc;
    if (target < -1 || target >= n) return ECG_EINVAL;
    const BlockPtrs src{ec->impl->k, n, d_data_ptrs, d_coding_ptrs};
    if (src.any_null()) return ECG_EINVAL;
    LastCheck& c = last_check(n, r, H.data());
    if (const int rc = check_independent(c, target < 0); rc != ECG_OK) return rc;
    if (block_size == 0) return ECG_OK;
    const std::vector<int> ids = iota(n);
    return run_heal2(cached_plan(c, ids.data(), false), GF_MODE_INLINE, block_size, 1, nullptr, nullptr, target,
                     target < 0, d_report, src.vec_ok(), ec->impl->stream, src);
}

int ecg_heal2_counters(long long* launches, long long* bytes) {
    heal2_traffic(launches, bytes);
    return ECG_OK;
}

int ecg_heal2_last_launch(int* v, int cap) { return heal2_last_launch(v, cap); }

}  // extern "C"
