// The record rule of the range reads on the host (dread.cpp, vread.cpp): the device's rule for states 1-5
// (record_state of dread_kernels.hip and vread_plan_device.hpp) and the check of ecg_dread_check_records / ecg_vread_check_records over it.
// Host-only and header-only.
#pragma once
#include <iterator>
#include <map>
#include <string>

#include "dread_kernels.hpp"

namespace ecg {

inline int dread_record_state(const long long* r, int n, long long B, int S, long long max_len, long long out_bytes) {
    const long long stripe = r[0], col = r[1], off = r[2], len = r[3], out_off = r[4];
    if (stripe < 0 || stripe >= S) return kDreadBadStripe;
    if (col < 0 || col >= n) return kDreadBadCol;
    if (off < 0 || len < 0 || off > B || len > B - off) return kDreadBadRange;
    if (len > max_len) return kDreadTooLong;
    if (out_off < 0 || out_off > out_bytes || len > out_bytes - out_off) return kDreadBadOut;
    return kDreadAnswered;
}

// [lo, hi) into a set of pairwise disjoint ranges keyed by lo: false if it overlaps one of them.
typedef std::map<long long, long long> RangeSet;
inline bool insert_disjoint(RangeSet& set, long long lo, long long hi) {
    if (hi <= lo) return true;  // an empty range overlaps nothing
    auto next = set.lower_bound(lo);
    if (next != set.end() && next->first < hi) return false;
    if (next != set.begin() && std::prev(next)->second > lo) return false;
    set[lo] = hi;
    return true;
}

// -1 if no record of h_records[R][5] is refused with a state 1-5 and the out ranges are pairwise disjoint; else the
// index of the first offending record, with `why` saying which rule broke.
inline int dread_check_records(const long long* h_records, int R, int n, long long B, int S, long long max_len,
                               long long out_bytes, std::string& why) {
    static const char* const rule[] = {"", "stripe is not in [0, S)", "col is not in [0, n)",
                                       "off < 0, len < 0 or off + len > B", "len > max_len",
                                       "out_off < 0 or out_off + len > out_bytes"};
    RangeSet outs;
    for (int i = 0; i < R; i++) {
        const long long* r = h_records + (size_t)i * kDreadRecordWords;
        if (const int st = dread_record_state(r, n, B, S, max_len, out_bytes); st != kDreadAnswered) {
            why = "record " + std::to_string(i) + " is refused with state " + std::to_string(st) + ": " + rule[st];
            return i;
        }
        if (!insert_disjoint(outs, r[4], r[4] + r[3])) {
            why = "record " + std::to_string(i) + " overlaps an earlier record's out range";
            return i;
        }
    }
    return -1;
}

}  // namespace ecg
