// extern "C" entry points declared in include/ecg_heal2.h (libecg_heal2.so): the host side of two-block correction.
// A call reads four table sets, all LinearOps kept by the engine's program cache (Engine::program_set), so that the
// cache, ensure_ready, note_launch and retirement cover them alike: the check, the single-block ratios and the pivot
// inverses, as the heal builds them (heal.cpp), and the pair tables: one op of r rows over 2 * n (n - 1) / 2 <= 992
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

// The calling thread's last check matrix with what was worked out for it: a store heals with one code, call after
// call, and neither the <= 35 960 ranks nor the pair tables' coefficients need to be redone for it.
struct LastCheck {
    std::vector<int> H;
    int n = 0, r = 0;
    int verdict[2] = {-1, -1};  // [any]: -1 not asked yet, 0 accepted, 1 refused
    std::string refusal[2];
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

int find_dependent(int n, int r, const int* H, bool any);

// ANY2 needs every 4 columns independent, TARGET2 every 3 (include/ecg_heal2.h: the explanation is then unique).
int check_independent(int n, int r, const int* H, bool any) {
    LastCheck& c = last_check(n, r, H);
    if (c.verdict[any] < 0) {
        c.verdict[any] = find_dependent(n, r, H, any) == ECG_OK ? 0 : 1;
        if (c.verdict[any]) c.refusal[any] = last_error_string();
    }
    if (!c.verdict[any]) return ECG_OK;
    set_last_error(c.refusal[any]);
    return ECG_EINVAL;
}

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

int bad_shape(long long n, long long r) {
    set_last_error("heal2: r = " + std::to_string(r) + ", n = " + std::to_string(n) + " is outside " +
                   std::to_string(kHeal2MinR) + " <= r <= " + std::to_string(kMaxMT) + ", 2 <= n <= " +
                   std::to_string(kHeal2MaxN) + " (a pair needs a third row to be tested against; the pair tables " +
                   "grow with n (n - 1) / 2)");
    return ECG_EINVAL;
}

bool shape_ok(long long n, long long r) { return r >= kHeal2MinR && r <= kMaxMT && n >= 2 && n <= kHeal2MaxN; }

// ---- the plan

struct Heal2Plan {
    CandidatePlan cand;
    LinearOp inv;    // 1 x n: 1 / H[p0(b)][b], as the heal's
    LinearOp pairs;  // r x (2 * npairs): heal2_kernels.hpp Heal2Launch::pairs; src_ids are the packed pairs
    int npairs = 0;
};

unsigned pivot_of(const CandidatePlan& pl, int b) { return (pl.p0[b >> 3] >> ((b & 7) * 4)) & 15u; }

// H has passed check_independent: no zero column, and every two columns have an invertible 2 x 2 minor.
Heal2Plan make_heal2_plan(int n, int r, const int* H, const int* src_ids, bool consecutive) {
    Heal2Plan hp;
    hp.cand = make_plan(n, r, H, src_ids, consecutive);
    hp.inv.src_ids = iota(n);
    hp.inv.dst_ids = iota(1);
    hp.inv.coef.assign((size_t)n, 0);
    for (int b = 0; b < n; b++) {
        const unsigned p0 = pivot_of(hp.cand, b);
        if (p0 != kNoPivot) hp.inv.coef[b] = (uint8_t)gf::inv(H[(size_t)p0 * n + b] & 0xff);
    }
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

// The calling thread's last plan (see LastCheck): the same check over the same blocks needs no new one.
const Heal2Plan& cached_plan(int n, int r, const int* H, const int* src_ids, bool consecutive) {
    struct LastPlan {
        std::vector<int> H, ids;
        int r = 0;
        bool consecutive = false;
        Heal2Plan plan;
    };
    thread_local LastPlan c;
    const size_t cells = (size_t)n * r;
    if (c.r != r || c.consecutive != consecutive || c.ids.size() != (size_t)n || c.H.size() != cells ||
        memcmp(c.ids.data(), src_ids, (size_t)n * sizeof(int)) != 0 ||
        memcmp(c.H.data(), H, cells * sizeof(int)) != 0) {
        c.plan = make_heal2_plan(n, r, H, src_ids, consecutive);
        c.H.assign(H, H + cells);
        c.ids.assign(src_ids, src_ids + n);
        c.r = r;
        c.consecutive = consecutive;
    }
    return c.plan;
}

// ---- the launch

// What candidate_plan.hpp prepare_launch does for n + 2 counters, here for n + 3, then the pivot inverses and the pair
// tables on top of it, the family, and the launch.  `fill` sets the launch's sources.
template <class Fill>
int run_heal2(const Heal2Plan& hp, int mode, long long B, int S, const int* d_stripe_ids, const int* d_targets,
              int target, bool any, unsigned* d_report, bool vec_ok, hipStream_t st, Fill fill) {
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;
    const CandidatePlan& pl = hp.cand;
    Engine& eng = Engine::instance();
    int status = ECG_OK;
    const LinearOp* ops[4] = {&pl.chk.op, &pl.ratio, &hp.inv, &hp.pairs};
    std::shared_ptr<ProgramSet> sets[4];
    for (int i = 0; i < 4; i++) {
        sets[i] = eng.program_set(ops[i], 1, &status, st);
        if (!sets[i]) return status;
    }
    for (int i = 0; i < 4; i++)
        if (const int rc = sets[i]->ensure_ready(st); rc != ECG_OK) return rc;
    const ProgramSet &ps = *sets[0], &rs = *sets[1], &is = *sets[2], &qs = *sets[3];
    if (ps.MT != pl.r || ps.rtiles != 1 || rs.MT != pl.r || rs.rtiles != 1 || rs.k != pl.n || is.MT != 1 ||
        is.rtiles != 1 || is.k != pl.n || qs.MT != pl.r || qs.rtiles != 1 || qs.k != 2 * hp.npairs)
        return ECG_EINVAL;
    Heal2Launch h;
    memset(&h, 0, sizeof(h));
    LocateLaunch& a = h.l;
    a.g.tabs = ps.d_tabs;
    a.g.src_ids = ps.d_src;
    a.g.dst_ids = ps.d_dst;
    a.g.stripe_of = d_stripe_ids;
    a.g.B = B;
    a.g.k = ps.k;
    a.g.m = ps.m;
    a.g.S = S;
    a.g.MT = ps.MT;
    a.g.rtiles = ps.rtiles;
    a.g.binary = 0;  // the GENERAL flavour always: the tables of 0 and 1 are exact
    a.votes = d_report;
    a.ident = pl.chk.ident;
    a.ident_base = pl.chk.ident_base;
    a.ratios = rs.d_tabs;
    a.n = pl.n;
    memcpy(a.p0, pl.p0, sizeof(a.p0));
    fill(a.g);
    h.invlead = is.d_tabs;
    h.pairs = qs.d_tabs;
    h.pair_ids = qs.d_src;
    h.npairs = hp.npairs;
    h.targets = d_targets;
    h.target = target;
    h.any = any ? 1 : 0;
    if (const hipError_t e = hipMemsetAsync(d_report, 0, (size_t)S * (size_t)(pl.n + 3) * sizeof(unsigned), st);
        e != hipSuccess)
        return hip_fail(e, "hipMemsetAsync(heal2 report)");
    if (const hipError_t e = launch_heal2(h, mode, vec_ok, st); e != hipSuccess) return hip_fail(e, "launch_heal2");
    for (int i = 0; i < 4; i++) eng.note_launch(*sets[i], st);
    return ECG_OK;
}

// The strided forms after their own argument checks: the independence refusal, the no-op, the launch.
int run_strided_heal2(int n, int r, const int* H, const int* src_ids, void* d_base, long long sstride,
                      long long bstride, long long B, const int* d_stripe_ids, const int* d_targets, int S,
                      unsigned* d_report, hipStream_t st) {
    if (const int rc = check_independent(n, r, H, d_targets == nullptr); rc != ECG_OK) return rc;
    if (S == 0 || B == 0) return ECG_OK;
    const Heal2Plan& hp = cached_plan(n, r, H, src_ids, true);
    const bool vec_ok = aligned16(d_base) && sstride % 16 == 0 && bstride % 16 == 0;
    return run_heal2(hp, GF_MODE_STRIDED, B, S, d_stripe_ids, d_targets, -1, d_targets == nullptr, d_report, vec_ok, st,
                     [&](GfLaunch& g) {
                         g.in_base = (const uint8_t*)d_base;
                         g.in_sstride = sstride;
                         g.in_bstride = bstride;
                     });
}

// The check matrix of an ErasureCode handle, r x n: ECG_OK, the code's own error, or the refusal of its shape.
int ec_check2(ecg_ec* ec, std::vector<int>& H, int& n, int& r) {
    r = ec->impl->check_matrix(H);
    if (r < 0) return r;
    if (r < 1) return ECG_EINVAL;
    n = (int)(H.size() / (size_t)r);
    return shape_ok(n, r) ? ECG_OK : bad_shape(n, r);
}

}  // namespace

extern "C" {

int ecg_heal2_matrix_batch(int n, int r, const int* H, const int* src_ids, void* d_base, long long sstride,
                           long long bstride, long long B, const int* d_stripe_ids, const int* d_targets, int S_sel,
                           unsigned* d_report, void* stream) {
    if (n < 1 || r < 1 || bad_sizes(B, S_sel) || !H || !src_ids || !d_base || !d_report) return ECG_EINVAL;
    if (!shape_ok(n, r)) return bad_shape(n, r);
    return run_strided_heal2(n, r, H, src_ids, d_base, sstride, bstride, B, d_stripe_ids, d_targets, S_sel, d_report,
                             (hipStream_t)stream);
}

int ecg_heal2_encode_batch(int k, int m, const int* matrix, void* d_stripes, long long sstride, long long bstride,
                           long long B, const int* d_stripe_ids, const int* d_targets, int S_sel, unsigned* d_report,
                           void* stream) {
    if (k < 1 || m < 1 || bad_sizes(B, S_sel) || !matrix || !d_stripes || !d_report) return ECG_EINVAL;
    if (!shape_ok((long long)k + m, m)) return bad_shape((long long)k + m, m);
    const std::vector<int> H = encode_check(k, m, matrix), ids = iota(k + m);
    return run_strided_heal2(k + m, m, H.data(), ids.data(), d_stripes, sstride, bstride, B, d_stripe_ids, d_targets,
                             S_sel, d_report, (hipStream_t)stream);
}

int ecg_heal2_ec_batch(ecg_ec* ec, void* d_stripes, long long sstride, long long bstride, long long B,
                       const int* d_stripe_ids, const int* d_targets, int S_sel, unsigned* d_report, void* stream) {
    if (!ec || bad_sizes(B, S_sel) || !d_stripes || !d_report || ec->impl->mem != ECG_MEM_DEVICE) return ECG_EINVAL;
    std::vector<int> H;
    int n, r;
    if (const int rc = ec_check2(ec, H, n, r); rc != ECG_OK) return rc;
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
    if (const int rc = ec_check2(ec, H, n, r); rc != ECG_OK) return rc;
    const int k = ec->impl->k;
    if (target < -1 || target >= n) return ECG_EINVAL;
    for (int b = 0; b < n; b++)
        if (!(b < k ? d_data_ptrs[b] : d_coding_ptrs[b - k])) return ECG_EINVAL;
    if (const int rc = check_independent(n, r, H.data(), target < 0); rc != ECG_OK) return rc;
    if (block_size == 0) return ECG_OK;
    const std::vector<int> ids = iota(n);
    const Heal2Plan& hp = cached_plan(n, r, H.data(), ids.data(), false);
    bool vec_ok = true;
    for (int b = 0; b < n; b++) vec_ok &= aligned16(b < k ? d_data_ptrs[b] : d_coding_ptrs[b - k]);
    return run_heal2(hp, GF_MODE_INLINE, block_size, 1, nullptr, nullptr, target, target < 0, d_report, vec_ok,
                     ec->impl->stream, [&](GfLaunch& g) {
                         for (int b = 0; b < n; b++)
                             g.isrc[b] = (const uint8_t*)(b < k ? d_data_ptrs[b] : d_coding_ptrs[b - k]);
                     });
}

int ecg_heal2_counters(long long* launches, long long* bytes) {
    heal2_traffic(launches, bytes);
    return ECG_OK;
}

int ecg_heal2_last_launch(int* v, int cap) { return heal2_last_launch(v, cap); }

}  // extern "C"
