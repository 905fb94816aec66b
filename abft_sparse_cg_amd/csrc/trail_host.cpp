// trail_host.cpp -- the host's view of a protected trail (include/abft_hip.h: abft_hip_trail_encode,
// abft_hip_trail_decode), compiled as plain C++ from trail_ecc.h, the text the kernels compile, behind the shims a
// host build of it needs.  abft_hip.hip checks the arguments and calls these.
#include <cstdint>
#include <cstring>

#define __device__
#define __forceinline__ inline
static inline long long __double_as_longlong(double v) { long long b; memcpy(&b, &v, sizeof b); return b; }
static inline double __longlong_as_double(long long b) { double v; memcpy(&v, &b, sizeof v); return v; }
#ifndef __clang__  // (a builtin there)
static inline uint32_t __builtin_bitreverse32(uint32_t x) { uint32_t r = 0; for (int b = 0; b < 32; b++) r |= ((x >> b) & 1u) << (31 - b); return r; }
#endif

#include "trail_ecc.h"

void trail_host_encode(const double *values, int n, int first_ordinal, double *slots) {
  for (int i = 0; i < n; i++) {
    uint32_t w[4];
    trail_encode((uint64_t)__double_as_longlong(values[i]), (uint32_t)(first_ordinal + i), w);
    trail_store(slots, i, w);
  }
}

void trail_host_decode(const double *slots, int n, double *values, int *status, int *bits) {
  for (int i = 0; i < n; i++) {
    uint32_t w[4];
    trail_load(slots, i, w);
    const TrailWord t = trail_decode(w);
    values[i] = __longlong_as_double((long long)t.bits);
    if (status) status[i] = t.rc;
    if (bits) bits[i] = t.rc > 0 ? (int)t.bit : 0;
  }
}
