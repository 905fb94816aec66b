// guard_protocol.h -- the stop test of the device-resident CG loops (cg.cpp:94; DESIGN.md sections 5f, 5g, 5h, 5q) and
// the scalars that ride on it, written once.  Nothing of HIP is included: kernels.hip compiles this text for the
// device, tests/host/guard_protocol_play.cpp for the host (its shims: __device__, __forceinline__,
// __double_as_longlong, __longlong_as_double).
//
// A guarded iteration is two launches, the r half and the x / p half.  Both read the RECORD the iteration started from
// (`in`), which neither writes, so they decide alike and uniformly over their grids; the r half leaves the next record
// (`out`).  Records are plain doubles: GuardPair {r.r, queued events}, GuardQuad {r.r, queued events, r.z, 0.0} -- both
// beside the SpMV's {p.w, events} --, GuardBlock<K> {r.r[K], r.z[K], queued events, 0.0} beside {P.W[K], events}.
// A record (a column of the block record) is LIVE when its r.r > threshold -- false for NaN, as `while (rr > conv)`
// is.  Then alpha = r.z / p.w and beta = r.z of `out` / r.z of `in` (no preconditioner: r.r, whose bits the block
// record's r.z holds), IEEE quotients, and the r half's new sums go into `out`.  Otherwise it is FROZEN: its words are
// handed on as integers, whatever they are (a NaN's payload and sign, -0.0), so the next iteration freezes as well.
// A launch with nothing live returns before it touches a vector, a partial or the ticket, and one thread of the r half
// hands the whole record on.  Either way the events word is the queued-event count as a double, the trailing word +0.0.
// What needs the device stays in kernels.hip and comes in as plain values: the event count, the reduction's totals.
#pragma once
#include <stdint.h>

// the one comparison
__device__ __forceinline__ bool guard_live(double rr, double threshold) { return rr > threshold; }

// a record word carried as an integer
__device__ __forceinline__ uint64_t guard_word(const double *rec, int i) { return (uint64_t)__double_as_longlong(rec[i]); }
__device__ __forceinline__ void guard_put(double *rec, int i, uint64_t w) { rec[i] = __longlong_as_double((long long)w); }

template <bool QUAD> struct GuardSingle {
  enum { RR = 0, EV = 1, RZ = QUAD ? 2 : RR, LEN = QUAD ? 4 : 2, PW_LEN = 2 };
  static __device__ __forceinline__ bool live(const double *in, double threshold) { return guard_live(in[RR], threshold); }
  static __device__ __forceinline__ double alpha(const double *in, double pw) { return in[RZ] / pw; }
  static __device__ __forceinline__ double beta(const double *in, const double *out) { return out[RZ] / in[RZ]; }
  static __device__ __forceinline__ void hand_on(const double *in, double *out, uint32_t nev) {
    const uint64_t rr = guard_word(in, RR), rz = guard_word(in, RZ);
    guard_put(out, RR, rr);
    out[EV] = (double)nev;
    if constexpr (QUAD) {
      guard_put(out, RZ, rz);
      out[LEN - 1] = 0.0;
    }
  }
};
using GuardPair = GuardSingle<false>;
using GuardQuad = GuardSingle<true>;

// the block record's lengths for a k known at run time (the entries' overlap checks)
constexpr int guard_block_len(int k) { return 2 * k + 2; }
constexpr int guard_block_pw_len(int k) { return k + 1; }

template <int K> struct GuardBlock {
  enum { RR = 0, RZ = K, EV = 2 * K, LEN = guard_block_len(K), PW_LEN = guard_block_pw_len(K) };
  // bit j: column j is live
  static __device__ __forceinline__ uint32_t live_mask(const double *in, double threshold) {
    uint32_t active = 0u;
#pragma unroll
    for (int j = 0; j < K; j++) active |= guard_live(in[RR + j], threshold) ? 1u << j : 0u;
    return active;
  }
  static __device__ __forceinline__ double alpha(const double *in, const double *pw, int j) { return in[RZ + j] / pw[j]; }
  static __device__ __forceinline__ double beta(const double *in, const double *out, int j) {
    return out[RZ + j] / in[RZ + j];
  }
  static __device__ __forceinline__ void finish(double *out, uint32_t nev) {
    out[EV] = (double)nev;
    out[LEN - 1] = 0.0;
  }
  // no column live: the whole record
  static __device__ __forceinline__ void hand_on(const double *in, double *out, uint32_t nev) {
    uint64_t b[2 * K];
#pragma unroll
    for (int j = 0; j < 2 * K; j++) b[j] = guard_word(in, j);
#pragma unroll
    for (int j = 0; j < 2 * K; j++) guard_put(out, j, b[j]);
    finish(out, nev);
  }
  // The record behind a live launch.  tot, the r half's totals: tot[j] = column j's r.r, for both words; PRECOND:
  // tot[2j] = its r.z, tot[2j + 1] its r.r.  A frozen column's words stay as they were read, not those recomputed sums.
  template <bool PRECOND>
  static __device__ __forceinline__ void publish(const double *tot, uint32_t active, const double *in, double *out,
                                                 uint32_t nev) {
#pragma unroll
    for (int j = 0; j < K; j++) {
      const uint64_t rr_new = (uint64_t)__double_as_longlong(PRECOND ? tot[2 * j + 1] : tot[j]);
      const uint64_t rz_new = PRECOND ? (uint64_t)__double_as_longlong(tot[2 * j]) : rr_new;
      const bool on = (active >> j) & 1u;
      const uint64_t rr_old = guard_word(in, RR + j), rz_old = guard_word(in, RZ + j);
      guard_put(out, RR + j, on ? rr_new : rr_old);
      guard_put(out, RZ + j, on ? rz_new : rz_old);
    }
    finish(out, nev);
  }
};
