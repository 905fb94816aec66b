// vecc_walk.h -- the walk of the protected vector kernels (DESIGN.md sections 5e, 5k, 5l, 5p), written once, and the
// operations that run on it, each stated once.  Nothing of HIP is included: kernels.hip compiles this text for the
// device, tests/host/vecc_walk_play.cpp for the host (its shims: __device__, __forceinline__, __double_as_longlong,
// __longlong_as_double).
//
// An OPERATION is a struct with
//   N        its operands; the enumerators before it name them, in the order the cold decode visits them
//   WRITTEN  bit k: operand k is encoded and stored (every operand is loaded and checked)
//   DINV     the operand whose word, once the cold decode has repaired it, is stored back although the operation only
//            reads it (dinv outlives the iteration and no kernel rewrites it; the scrub's vector); -1: none
//   SUMS     its accumulators
//   step(s)       the arithmetic on one element: s.get(k) the value of operand k, s.put(k, v) encodes v into operand k.
//            An operand is read before it is put.
//   sums(s, acc)  what the element adds, read after the step: s.get(k) of a written operand is now its value AS STORED
//            (a step the hot loop carried out is summed from the words found in memory, which are those).
//   Every multiply and add is separate (-ffp-contract=off).
// The ordinal an event reports for operand k (VeccOperands::ord) stays the caller's: the host-scalar entries count
// their own arguments, the guarded entries count vec, x, r, p, w, dinv as 0..5.
#pragma once
#include <stdint.h>

#include "ecc_device.h"

struct alignas(16) VeccPair { double x, y; };

template <class OP> struct VeccOperands {
  double *v[OP::N];
  uint32_t ord[OP::N];
};

// One element of a step: the words of its operands
template <class OP> struct VeccStep {
  uint64_t w[OP::N];
  __device__ __forceinline__ double get(int k) const { return vecc_value(w[k]); }
  __device__ __forceinline__ void put(int k, double v) { w[k] = vecc_encode(v); }
};

// The first walk's step at elements i .. i + M - 1 (M == 2: one 16-byte load and store per operand): no call.  A step
// with a word that fails its check is only NOTED, by the result: nothing of it is stored (an operation that stores
// nothing is not held up: its sums are formed again in the second walk).  Per accumulator the adds run element 0,
// element 1.
template <int M, class OP>
__device__ __forceinline__ uint32_t vecc_hot_step(const OP &op, const VeccOperands<OP> &o, long i, double *acc) {
  VeccStep<OP> s[M];
  uint32_t sus = 0u;
  for (int k = 0; k < OP::N; k++) {
    if constexpr (M == 2) {
      const VeccPair t = *reinterpret_cast<const VeccPair *>(o.v[k] + i);
      s[0].w[k] = vecc_bits(t.x);
      s[1].w[k] = vecc_bits(t.y);
      sus |= vecc_suspect(s[0].w[k]) | vecc_suspect(s[1].w[k]);
    } else {
      s[0].w[k] = vecc_bits(o.v[k][i]);
      sus |= vecc_suspect(s[0].w[k]);
    }
  }
  if (OP::WRITTEN == 0 || !sus) {
    for (int e = 0; e < M; e++) op.step(s[e]);
    for (int k = 0; k < OP::N; k++) {
      if (!((OP::WRITTEN >> k) & 1)) continue;
      if constexpr (M == 2) {
        VeccPair t;
        t.x = vecc_double(s[0].w[k]);
        t.y = vecc_double(s[1].w[k]);
        *reinterpret_cast<VeccPair *>(o.v[k] + i) = t;
      } else {
        o.v[k][i] = vecc_double(s[0].w[k]);
      }
    }
    for (int e = 0; e < M; e++) op.sums(s[e], acc);
  }
  return sus;
}

// The walk of one thread's chain: elements first, first + stride, ... below n, VEC of them a step; the last step of a
// VEC == 2 chain may be the single odd element n - 1.  Behind the first walk a thread with a noted step walks its
// chain once more, its sums reset.  A step that now reads clean was carried out above: it adds from the words it
// finds -- the outputs it stored, the inputs nothing has changed.  A step that still fails is the noted one: every
// failing word of it goes through `cold` (word, element index, operand ordinal) -> VeccWord, the repair in registers;
// the step is carried out, stores, and adds what it stores.  (An operation that writes nothing takes
// every step for a noted one: carried out twice it leaves the same bits, and no step needs judging first.)  Same
// operands and the same order of adds as an undamaged call, so every vector and every sum has the undamaged call's
// bits.  Among the operands that are read and not written only DINV's repaired word is stored back.
// acc: OP::SUMS accumulators, zero on entry (unused when there are none).
template <int VEC, class OP, class COLD>
__device__ __forceinline__ void vecc_walk(const OP &op, const VeccOperands<OP> &o, int n, long first, long stride,
                                          COLD &cold, double *acc) {
  uint32_t bad = 0u;
  long i = first;
  for (; i + VEC <= n; i += stride) bad |= vecc_hot_step<VEC>(op, o, i, acc);
  if (VEC == 2 && i < n) bad |= vecc_hot_step<1>(op, o, i, acc);
  if (__builtin_expect(bad != 0u, 0)) {
    for (int j = 0; j < OP::SUMS; j++) acc[j] = 0.0;
    for (i = first; i < n; i += stride) {
      const int m = (VEC == 2 && i + 1 < n) ? 2 : 1;
      uint32_t sus = OP::WRITTEN == 0;
      for (int e = 0; e < m && OP::WRITTEN != 0; e++)
        for (int k = 0; k < OP::N; k++) sus |= vecc_suspect(vecc_bits(o.v[k][i + e]));
      if (!sus && OP::SUMS == 0) continue;  // carried out above, and nothing to add
      for (int e = 0; e < m; e++) {
        VeccStep<OP> s;
        for (int k = 0; k < OP::N; k++) {
          s.w[k] = vecc_bits(o.v[k][i + e]);
          if (sus && __builtin_expect(vecc_suspect(s.w[k]) != 0u, 0)) {
            const VeccWord f = cold(s.w[k], (uint32_t)(i + e), o.ord[k]);
            if (k == OP::DINV && f.rc > 0) o.v[k][i + e] = vecc_double(f.w);
            s.w[k] = f.w;
          }
        }
        if (sus) {
          op.step(s);
          for (int k = 0; k < OP::N; k++)
            if ((OP::WRITTEN >> k) & 1) o.v[k][i + e] = vecc_double(s.w[k]);
        }
        op.sums(s, acc);
      }
    }
  }
}

// ---- the operations ----

// sum a b; nothing is written
struct VeccDot {
  enum { A, B, N, WRITTEN = 0, DINV = -1, SUMS = 1 };
  template <class S> __device__ __forceinline__ void step(S &) const {}
  template <class S> __device__ __forceinline__ void sums(const S &s, double *acc) const { acc[0] += s.get(A) * s.get(B); }
};

// x <- enc(x + alpha p), r <- enc(r - alpha w); sum of the stored r's squares
struct VeccCalcXr {
  enum { X, R, P, W, N, WRITTEN = 1 << X | 1 << R, DINV = -1, SUMS = 1 };
  double alpha;
  template <class S> __device__ __forceinline__ void step(S &s) const {
    s.put(X, s.get(X) + alpha * s.get(P));
    s.put(R, s.get(R) - alpha * s.get(W));
  }
  template <class S> __device__ __forceinline__ void sums(const S &s, double *acc) const { acc[0] += s.get(R) * s.get(R); }
};

// p <- enc(r + beta p)
struct VeccCalcP {
  enum { P, R, N, WRITTEN = 1 << P, DINV = -1, SUMS = 0 };
  double beta;
  template <class S> __device__ __forceinline__ void step(S &s) const { s.put(P, s.get(R) + beta * s.get(P)); }
  template <class S> __device__ __forceinline__ void sums(const S &, double *) const {}
};

// The r half: r <- enc(r - alpha w) -> sum r' r', r' the stored r without its code bits.  PRECOND: {sum r' z',
// sum r' r'} with z' = dec(dinv) * r', one rounded product that is never stored.
template <bool PRECOND> struct VeccCalcR {
  enum { R, W, D, N = PRECOND ? 3 : 2, WRITTEN = 1 << R, DINV = PRECOND ? (int)D : -1, SUMS = PRECOND ? 2 : 1 };
  double alpha;
  template <class S> __device__ __forceinline__ void step(S &s) const { s.put(R, s.get(R) - alpha * s.get(W)); }
  template <class S> __device__ __forceinline__ void sums(const S &s, double *acc) const {
    const double rs = s.get(R);
    if constexpr (PRECOND) acc[0] += rs * (s.get(D) * rs);
    acc[SUMS - 1] += rs * rs;
  }
};

// The preconditioned x / p half: x <- enc(x + alpha p) and p <- enc(z + beta p), both from the old p, z the rounded
// product dec(dinv) * dec(r) that is never stored
struct VeccCalcPxPrecond {
  enum { X, P, R, D, N, WRITTEN = 1 << X | 1 << P, DINV = D, SUMS = 0 };
  double alpha, beta;
  template <class S> __device__ __forceinline__ void step(S &s) const {
    const double po = s.get(P);
    s.put(X, s.get(X) + alpha * po);
    s.put(P, s.get(D) * s.get(R) + beta * po);
  }
  template <class S> __device__ __forceinline__ void sums(const S &, double *) const {}
};

// the scrub: no arithmetic; every repaired word is stored back (the cold decode counts)
struct VeccScrub {
  enum { V, N, WRITTEN = 0, DINV = V, SUMS = 0 };
  template <class S> __device__ __forceinline__ void step(S &) const {}
  template <class S> __device__ __forceinline__ void sums(const S &, double *) const {}
};
