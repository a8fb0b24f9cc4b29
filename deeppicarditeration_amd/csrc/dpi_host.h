// Host helpers shared by the library's three host units (dpi_kernels.hip, dpi_net.hip, dpi_fit.hip):
// the error string behind dpi_last_error, the HIP call check and the environment knobs.  One
// definition each for all units, none of them an exported dynamic symbol.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <string>

#include "../../include/dpi.h"

#define DPI_HIDDEN __attribute__((visibility("hidden")))

DPI_HIDDEN inline thread_local std::string g_err;

static inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIPCHK(x)                                                                                    \
  do {                                                                                               \
    hipError_t _e = (x);                                                                             \
    if (_e != hipSuccess) return fail(DPI_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(_e)); \
  } while (0)

// The integer / real environment knobs: unset gives dflt, a set value is clamped
// to [lo, hi].  A knob read once per process keeps the result in a function-local static; the ones
// a test flips inside one process call these afresh.
static inline int env_int(const char* name, int dflt, int lo = INT_MIN, int hi = INT_MAX) {
  const char* e = std::getenv(name);
  return e ? std::max(lo, std::min(hi, std::atoi(e))) : dflt;
}
static inline double env_real(const char* name, double dflt, double lo, double hi) {
  const char* e = std::getenv(name);
  return e ? std::max(lo, std::min(hi, std::atof(e))) : dflt;
}

// dpi_label_prepare's records naming a destroyed handle (defined in dpi_kernels.hip, with the
// workspace tags)
extern "C" DPI_HIDDEN void prep_tags_drop(const void* owner);
