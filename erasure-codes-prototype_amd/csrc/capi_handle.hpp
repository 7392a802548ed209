// The C ABI's ErasureCode handle (include/ecg.h ecg_ec), shared by the translation units that implement
// entry points over it: capi.cpp (libecg.so) and scrub.cpp (libecg_scrub.so).
#pragma once
#include "codes.hpp"

struct ecg_ec {
    ecg::ErasureCode* impl;
};
