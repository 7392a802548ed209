// Host-only state of the region product: the run-time option table (ecg_set_option; ECG_OPT_* in include/ecg.h), which
// launch_gf and the check libraries read through get_option, and the coefficient tables the kernels multiply with.
#include <atomic>
#include <stdlib.h>

#include "gf_kernels.hpp"
#include "gf256.hpp"

namespace ecg {

namespace {

std::atomic<long long> g_opt[ECG_OPT_COUNT] = {};
std::atomic<int> g_opt_init{0};

void init_options() {
    if (g_opt_init.load(std::memory_order_acquire)) return;
    auto env = [](const char* n, long long d) {
        const char* e = getenv(n);
        return e ? atoll(e) : d;
    };
    g_opt[ECG_OPT_NT].store(env("ECG_NT", 3));
    g_opt[ECG_OPT_COLS_PER_WG].store(env("ECG_COLS_PER_WG", 0));
    g_opt[ECG_OPT_GRID_MAP].store(env("ECG_GRID_MAP", 3));
    // every staged call (r02 host_latency.py --sweep-zc: zero-copy with completion flags beats DMA staging
    // at every block size up to kStagedMaxBlock)
    g_opt[ECG_OPT_ZEROCOPY_BYTES].store(env("ECG_ZEROCOPY_BYTES", 8 << 20));
    g_opt[ECG_OPT_PROGRAM_CACHE].store(env("ECG_PROGRAM_CACHE", 4096));
    g_opt[ECG_OPT_MAP_GROUP].store(env("ECG_MAP_GROUP", 1));
    g_opt[ECG_OPT_LAT_DWORD_BYTES].store(env("ECG_LAT_DWORD_BYTES", 1 << 20));
    g_opt[ECG_OPT_CALL_WORKER].store(env("ECG_CALL_WORKER", 0));
    g_opt[ECG_OPT_ROW_SPLIT].store(env("ECG_ROW_SPLIT", 16));
    g_opt[ECG_OPT_GRAVEYARD].store(env("ECG_GRAVEYARD", 16384));
    g_opt[ECG_OPT_MT1_LDS_PAD].store(env("ECG_MT1_LDS_PAD", -1));
    g_opt_init.store(1, std::memory_order_release);
}

}  // namespace

long long get_option(int opt) {
    init_options();
    if (opt < 0 || opt >= ECG_OPT_COUNT) return -1;
    return g_opt[opt].load();
}

int set_option(int opt, long long value) {
    init_options();
    if (opt < 0 || opt >= ECG_OPT_COUNT) return -1;
    if (opt == ECG_OPT_NT && (value < 0 || value > 3)) return -1;
    if (opt == ECG_OPT_COLS_PER_WG && (value < 0 || (value % kThreads) != 0)) return -1;
    if (opt == ECG_OPT_GRID_MAP && (value < 0 || value > 3)) return -1;
    if (opt == ECG_OPT_ZEROCOPY_BYTES && value < 0) return -1;
    if (opt == ECG_OPT_PROGRAM_CACHE && value < 2) return -1;
    if (opt == ECG_OPT_MAP_GROUP && (value < 1 || value > (1 << 20))) return -1;
    if (opt == ECG_OPT_LAT_DWORD_BYTES && value < 0) return -1;
    if (opt == ECG_OPT_CALL_WORKER && (value < 0 || value > 1000000)) return -1;  // idle limit <= 1 s
    if (opt == ECG_OPT_ROW_SPLIT && value < 0) return -1;
    if (opt == ECG_OPT_GRAVEYARD && value < 1) return -1;
    if (opt == ECG_OPT_MT1_LDS_PAD && (value < -1 || value > 65536)) return -1;
    g_opt[opt].store(value);
    return 0;
}

void make_coef_tab(int c, CoefTab* t) {
    c &= 0xff;
    uint8_t e0[8], e1[8], e2[4];
    for (int e = 0; e < 8; ++e) {
        e0[e] = (uint8_t)gf::mul(c, e);
        e1[e] = (uint8_t)gf::mul(c, e << 3);
    }
    for (int e = 0; e < 4; ++e) e2[e] = (uint8_t)gf::mul(c, e << 6);
    auto pack = [](const uint8_t* b) {
        return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    };
    t->t0lo = pack(e0);
    t->t0hi = pack(e0 + 4);
    t->t1lo = pack(e1);
    t->t1hi = pack(e1 + 4);
    t->t2 = pack(e2);
    t->mask = (c == 1) ? 0xffffffffu : 0u;
    t->pad0 = 0u;
    t->pad1 = 0u;
}

}  // namespace ecg
