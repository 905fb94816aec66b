// trail_ecc.h -- the scalar trail of the device-resident CG loop under a SECDED code: the pure
// part.  No HIP in here: the kernels (kernels.hip), the C ABI's host code (abft_hip.hip) and a CPU program
// (tests/host/trail_ecc_play.cpp) compile this text.  The code is struct_ecc.h's row-block descriptor code -- the
// reference's 128-bit COO element in secded form --, unchanged: no new table.
//
// A protected trail word is a SLOT of 128 bits, two doubles of the trail vector, read as the COO element
//   word 0  bits 0..23   the word's ORDINAL in its record (record: 0 r.r, 1 events, 2 r.z, 3 the trailing 0.0;
//                        the SpMV's pair: 0 p.w, 1 events) -- its place in the record, not the record's place in the
//                        trail, so that a raw copy of a record to another place keeps its codewords valid
//           bits 24..31  the check byte
//   word 1               0
//   words 2, 3           the double, every bit: nothing is truncated, so values, quotients and histories keep the bits
//                        of the unprotected loop
// A record of LEN words is LEN slots, 2 LEN doubles; the pair is 2 slots.
//
// On top of the slot: TrailSingle<QUAD>, the protected twin of GuardSingle<QUAD> (guard_protocol.h).  It decodes the
// slots a decision depends on and answers with GuardSingle's own functions on the decoded values, so for values that
// decode clean it gives guard_protocol.h's bits by construction; every slot it writes is a fresh encode of a value
// that is moved as an integer (a NaN's payload and -0.0 survive).
//
// TrailBlock<K> is the same twin of GuardBlock<K>: every word of the block record {r.r[K],
// r.z[K], events, 0.0} a slot under GuardBlock's own ordinal (RR + j = j, RZ + j = K + j, EV = 2K, the trailing word
// 2K + 1), in the SpMM's tail P.W[j] under j and the events word under K.  A record is 2 (2K + 2) doubles, the tail
// 2 (K + 1).
#pragma once
#include <stdint.h>

#include "guard_protocol.h"
#include "struct_ecc.h"

#define ABFT_TRAIL_ORDINAL_MASK 0x00FFFFFFu
// the record of a trail event, bits 8..15 of abft_event::bit (bits 0..7: the slot's bit, numbered as the COO element's
// 128 with the parity bit 24); abft_event::index is the word's ordinal
#ifndef ABFT_TRAIL_START  // (include/abft_hip.h states the same three)
#define ABFT_TRAIL_START 0u  // the record the iteration starts from
#define ABFT_TRAIL_PW 1u     // the SpMV's pair {p.w, events}
#define ABFT_TRAIL_NEXT 2u   // the record the iteration leaves
#endif
#define ABFT_TRAIL_SLOT 2    // doubles per slot

// value (as its bits), ordinal -> the four stored words
__device__ __forceinline__ void trail_encode(uint64_t bits, uint32_t ordinal, uint32_t *w) {
  w[0] = ordinal & ABFT_TRAIL_ORDINAL_MASK;
  w[1] = 0u;
  w[2] = (uint32_t)bits;
  w[3] = (uint32_t)(bits >> 32);
  blk_encode(w);
}
__device__ __forceinline__ uint64_t trail_bits(const uint32_t *w) { return (uint64_t)w[2] | ((uint64_t)w[3] << 32); }
__device__ __forceinline__ uint32_t trail_ordinal(const uint32_t *w) { return w[0] & ABFT_TRAIL_ORDINAL_MASK; }
// hot test: blk_suspect(w) | trail_misplaced(w, ordinal) (below).  Cold decode: blk_repair(w, o, bit) -- o.rc 1 one
// flip put back (`bit` the one), -1 two flips, the words as they are.

// a slot as a decode leaves it: the words (repaired when rc == 1), the value's bits, the verdict, the flipped bit
struct TrailWord {
  uint32_t w[4];
  uint64_t bits;
  int rc;  // 0 clean, 1 repaired, -1 two flips
  uint32_t bit;
};
__device__ __forceinline__ TrailWord trail_decode(const uint32_t *w) {
  TrailWord t;
  t.w[0] = w[0]; t.w[1] = w[1]; t.w[2] = w[2]; t.w[3] = w[3];
  t.rc = 0;
  t.bit = 0u;
  if (blk_suspect(w)) {
    StructBlk o;
    blk_repair(w, o, t.bit);
    t.w[0] = o.w[0]; t.w[1] = o.w[1]; t.w[2] = o.w[2]; t.w[3] = o.w[3];
    t.rc = o.rc;
  }
  t.bits = trail_bits(t.w);
  return t;
}

// A codeword in the wrong place: the ordinal under the code is not the one being read, or word 1 is not 0 (non-zero
// iff so).  Part of the hot test of every read that knows its ordinal; such a slot cannot be repaired: rc -1, the
// words as they are.
__device__ __forceinline__ uint32_t trail_misplaced(const uint32_t *w, uint32_t ordinal) {
  return ((w[0] ^ ordinal) & ABFT_TRAIL_ORDINAL_MASK) | w[1];
}
__device__ __forceinline__ TrailWord trail_decode_at(const uint32_t *w, uint32_t ordinal) {
  TrailWord t = trail_decode(w);
  if (t.rc >= 0 && trail_misplaced(t.w, ordinal)) {
    t.w[0] = w[0]; t.w[1] = w[1]; t.w[2] = w[2]; t.w[3] = w[3];
    t.bits = trail_bits(w);
    t.rc = -1;
    t.bit = 0u;
  }
  return t;
}

// ---- slots in a trail of doubles (host and device alike: plain loads and stores of the two doubles) ----
__device__ __forceinline__ void trail_load(const double *rec, int ordinal, uint32_t *w) {
  const uint64_t a = guard_word(rec, ABFT_TRAIL_SLOT * ordinal), b = guard_word(rec, ABFT_TRAIL_SLOT * ordinal + 1);
  w[0] = (uint32_t)a; w[1] = (uint32_t)(a >> 32); w[2] = (uint32_t)b; w[3] = (uint32_t)(b >> 32);
}
__device__ __forceinline__ void trail_store(double *rec, int ordinal, const uint32_t *w) {
  guard_put(rec, ABFT_TRAIL_SLOT * ordinal, (uint64_t)w[0] | ((uint64_t)w[1] << 32));
  guard_put(rec, ABFT_TRAIL_SLOT * ordinal + 1, (uint64_t)w[2] | ((uint64_t)w[3] << 32));
}
// a fresh encode of a value into its slot
__device__ __forceinline__ void trail_put(double *rec, int ordinal, uint64_t bits) {
  uint32_t w[4];
  trail_encode(bits, (uint32_t)ordinal, w);
  trail_store(rec, ordinal, w);
}
__device__ __forceinline__ void trail_put_value(double *rec, int ordinal, double v) {
  trail_put(rec, ordinal, (uint64_t)__double_as_longlong(v));
}

// ---- the protected twin of GuardSingle<QUAD> ----
// What a launch knows of the record it starts from once its slots are decoded: the values r.r and r.z (pair: r.z is
// r.r) as plain doubles in GuardSingle's layout, so that GuardSingle's own live / alpha / beta answer.
template <bool QUAD> struct TrailSingle {
  using G = GuardSingle<QUAD>;
  enum { RR = G::RR, EV = G::EV, RZ = G::RZ, LEN = G::LEN, PW_LEN = G::PW_LEN,
         DOUBLES = ABFT_TRAIL_SLOT * G::LEN, PW_DOUBLES = ABFT_TRAIL_SLOT * G::PW_LEN };
  // decoded values -> a plain record GuardSingle reads (the events and trailing words are not decisions: 0)
  static __device__ __forceinline__ void plain(uint64_t rr, uint64_t rz, double *rec) {
    for (int i = 0; i < LEN; i++) rec[i] = 0.0;
    guard_put(rec, RR, rr);
    if (QUAD) guard_put(rec, RZ, rz);
  }
  static __device__ __forceinline__ bool live(uint64_t rr, double threshold) {
    double rec[LEN];
    plain(rr, rr, rec);
    return G::live(rec, threshold);
  }
  // alpha = r.z / p.w (pair: r.r / p.w), from the two checked slots: the same IEEE quotient in both halves
  static __device__ __forceinline__ double alpha(uint64_t rr, uint64_t rz, uint64_t pw) {
    double rec[LEN];
    plain(rr, rz, rec);
    return G::alpha(rec, __longlong_as_double((long long)pw));
  }
  // beta = r.z of the next record / r.z of the start record (pair: the r.r words)
  static __device__ __forceinline__ double beta(uint64_t rr, uint64_t rz, uint64_t next_rz) {
    double in[LEN], out[LEN];
    plain(rr, rz, in);
    plain(next_rz, next_rz, out);
    return G::beta(in, out);
  }
  // the frozen hand-on: the decoded (repaired) words through GuardSingle::hand_on, every word re-encoded
  static __device__ __forceinline__ void hand_on(uint64_t rr, uint64_t rz, double *out, uint32_t nev) {
    double in[LEN], plain_out[LEN];
    plain(rr, rz, in);
    G::hand_on(in, plain_out, nev);
    for (int i = 0; i < LEN; i++) trail_put(out, i, guard_word(plain_out, i));
  }
  // two flips in a slot the decision depends on: the record word for word, unrepaired
  static __device__ __forceinline__ void hand_on_raw(const double *in, double *out) {
    uint64_t b[DOUBLES];
    for (int i = 0; i < DOUBLES; i++) b[i] = guard_word(in, i);
    for (int i = 0; i < DOUBLES; i++) guard_put(out, i, b[i]);
  }
  // publication behind a live r half: the new sums (pair: rz is rr), the queued-event count, +0.0
  static __device__ __forceinline__ void publish(double rr_new, double rz_new, double *out, uint32_t nev) {
    trail_put_value(out, RR, rr_new);
    trail_put_value(out, EV, (double)nev);
    if (QUAD) {
      trail_put_value(out, RZ, rz_new);
      trail_put_value(out, LEN - 1, 0.0);
    }
  }
  // the SpMV's pair
  static __device__ __forceinline__ void publish_pw(double pw, double *out, uint32_t nev) {
    trail_put_value(out, 0, pw);
    trail_put_value(out, 1, (double)nev);
  }
};
using TrailPair = TrailSingle<false>;
using TrailQuad = TrailSingle<true>;

// ---- the protected twin of GuardBlock<K> ----
// What a launch knows of its start record once the slots are decoded: v[2K], the bits of r.r[K] then r.z[K] (the
// record's own order).  GuardBlock's functions answer on a plain record rebuilt from them.
// Slots come through get(record, ordinal) -> {bits, rc} (rc < 0: two flips): the kernels' checked loads (one lane a
// slot, the values broadcast: kernels.hip), a host's decode.  The read_* rules are the whole of what a launch reads: all 2K value slots of the start record,
// whatever is live; of the P.W tail and of the next record only a LIVE column's slot -- a frozen column's P.W is
// not a decision (the next fold overwrites it with a fresh encode), so damage there must not stop anything.
template <int K> struct TrailBlock {
  using G = GuardBlock<K>;
  enum { RR = G::RR, RZ = G::RZ, EV = G::EV, LEN = G::LEN, PW_LEN = G::PW_LEN, VALUES = 2 * K,
         DOUBLES = ABFT_TRAIL_SLOT * G::LEN, PW_DOUBLES = ABFT_TRAIL_SLOT * G::PW_LEN };
  // false: two flips in one of them; reading stops there (one event)
  template <class Get> static __device__ __forceinline__ bool read_start(Get &&get, uint64_t *v) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < VALUES; i++) {
      v[i] = 0u;
      if (ok) {
        const auto g = get(ABFT_TRAIL_START, i);
        v[i] = g.bits;
        ok = g.rc >= 0;
      }
    }
    return ok;
  }
  // The scalars of a launch with a live column, column by column: P.W[j] -- BETAS (the x / p half): then the next
  // record's r.z[j] -- of a LIVE column j, and its alpha_j (beta_j) at once: the slots' values need not be kept.  A frozen column's slots are not read; its alpha and beta are +0.0, which the walks' selects
  // drop.  false: two flips in a slot read; reading stops there (one event).
  template <bool BETAS, class Get>
  static __device__ __forceinline__ bool read_scalars(Get &&get, const uint64_t *v, uint32_t active, double *alpha,
                                                      double *beta) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < K; j++) {
      alpha[j] = 0.0;
      if (BETAS) beta[j] = 0.0;
      if (ok && ((active >> j) & 1u)) {
        const auto pw = get(ABFT_TRAIL_PW, j);
        ok = pw.rc >= 0;
        if (ok) alpha[j] = TrailBlock::alpha(v, pw.bits, j);
        if (BETAS && ok) {
          const auto nz = get(ABFT_TRAIL_NEXT, RZ + j);
          ok = nz.rc >= 0;
          if (ok) beta[j] = TrailBlock::beta(v, nz.bits, j);
        }
      }
    }
    return ok;
  }
  // decoded values -> a plain record GuardBlock reads (the events and trailing words are not decisions: 0)
  static __device__ __forceinline__ void plain(const uint64_t *v, double *rec) {
#pragma unroll
    for (int i = 0; i < VALUES; i++) guard_put(rec, i, v[i]);
    rec[EV] = 0.0;
    rec[LEN - 1] = 0.0;
  }
  static __device__ __forceinline__ uint32_t live_mask(const uint64_t *v, double threshold) {
    double rec[LEN];
    plain(v, rec);
    return G::live_mask(rec, threshold);
  }
  // alpha_j = r.z[j] / P.W[j], beta_j = the next record's r.z[j] / r.z[j]: GuardBlock's quotients, the same in both halves
  static __device__ __forceinline__ double alpha(const uint64_t *v, uint64_t pw, int j) {
    double rec[LEN], p[K];
    plain(v, rec);
#pragma unroll
    for (int i = 0; i < K; i++) guard_put(p, i, pw);
    return G::alpha(rec, p, j);
  }
  static __device__ __forceinline__ double beta(const uint64_t *v, uint64_t next_rz, int j) {
    double in[LEN], out[LEN];
    plain(v, in);
#pragma unroll
    for (int i = 0; i < LEN; i++) guard_put(out, i, next_rz);
    return G::beta(in, out, j);
  }
  // a plain record as GuardBlock left it -> slots, every word a fresh encode of its bits
  static __device__ __forceinline__ void put_record(const double *plain_out, double *out) {
#pragma unroll
    for (int i = 0; i < LEN; i++) {
      const uint64_t word = guard_word(plain_out, i);
      trail_put(out, i, word);
    }
  }
  // no column live: the decoded (repaired) words through GuardBlock::hand_on
  static __device__ __forceinline__ void hand_on(const uint64_t *v, double *out, uint32_t nev) {
    double in[LEN], plain_out[LEN];
    plain(v, in);
    G::hand_on(in, plain_out, nev);
    put_record(plain_out, out);
  }
  // two flips in a slot the decision depends on: the record word for word, unrepaired
  static __device__ __forceinline__ void hand_on_raw(const double *in, double *out) {
    for (int i = 0; i < DOUBLES; i++) guard_put(out, i, guard_word(in, i));
  }
  // the record behind a live launch: GuardBlock::publish<PRECOND> (tot as there), a frozen column's words the
  // repaired integers
  template <bool PRECOND>
  static __device__ __forceinline__ void publish(const double *tot, uint32_t active, const uint64_t *v, double *out,
                                                 uint32_t nev) {
    double in[LEN], plain_out[LEN];
    plain(v, in);
    G::template publish<PRECOND>(tot, active, in, plain_out, nev);
    put_record(plain_out, out);
  }
  // the SpMM's tail {P.W[K], queued events}
  static __device__ __forceinline__ void publish_pw(const double *tot, double *out, uint32_t nev) {
#pragma unroll
    for (int j = 0; j < K; j++) trail_put_value(out, j, tot[j]);
    trail_put_value(out, K, (double)nev);
  }
};
