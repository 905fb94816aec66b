// The protected scalar trail on a CPU (tests/test_trail_ecc_host.py builds this with AddressSanitizer and UBSan and runs
// it as a program of its own).  trail_ecc.h -- with struct_ecc.h, ecc_device.h and guard_protocol.h behind it -- is
// included as the kernels compile it, behind a few shims.  Every record lives in a heap block of exactly its length,
// the destinations filled with a pattern no case contains, so a word too many or too few shows.
//
// input (a file named on the command line, else stdin), one request a line, every double as the hex of its bits:
//   slot ORDINAL VALUE -> slot W0 W1 W2 W3 SUSPECT / s BIT RC VALUE W0 W1 W2 W3 REPORTED-BIT (x 128, every single flip) /
//                         d FATAL UNCHANGED (of the 8128 double flips: how many were fatal, how many left the words)
//   single QUAD THRESHOLD NEV rr rz pw new FRR FRZ FPW FNEW
//                      -> s LIVE alpha beta handed-on[LEN] published[LEN] REPAIRS
//      The record {rr, 5.0, rz, -3.0}, the pair {pw, 2.0} and the next record {new, 6.0, new, 8.0} are encoded; bit
//      FRR / FRZ / FPW / FNEW (128: none) of the slot of r.r / r.z / p.w / the next record's r.z is flipped; then the
//      slots are decoded as a launch decodes them and TrailSingle<QUAD> answers.  handed-on and published are printed
//      as the VALUES of the slots written, after the program has checked that each is a clean codeword of its ordinal
//      with word 1 zero.  REPAIRS: how many decodes returned rc 1.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#define __device__
#define __forceinline__ inline
static inline long long __double_as_longlong(double v) { long long b; memcpy(&b, &v, sizeof b); return b; }
static inline double __longlong_as_double(long long b) { double v; memcpy(&v, &b, sizeof v); return v; }
static inline uint32_t __builtin_bitreverse32(uint32_t x) { uint32_t r = 0; for (int b = 0; b < 32; b++) r |= ((x >> b) & 1u) << (31 - b); return r; }

#include "trail_ecc.h"

static const uint64_t POISON = 0x7ff4dead0000beefull;
static std::istream *src;

static uint64_t hex() {
  std::string t;
  if (!(*src >> t)) abort();
  return strtoull(t.c_str(), nullptr, 16);
}
static int number() {
  int v;
  if (!(*src >> v)) abort();
  return v;
}
static std::vector<double> poisoned(int n) {
  std::vector<double> r((size_t)n, __longlong_as_double((long long)POISON));
  r.shrink_to_fit();
  return r;
}
static void flip(uint32_t *w, int bit) {
  if (bit < 128) w[bit >> 5] ^= 1u << (bit & 31);
}

static void play_slot(uint32_t ordinal, uint64_t value) {
  uint32_t w[4];
  trail_encode(value, ordinal, w);
  printf("slot %08x %08x %08x %08x %u\n", w[0], w[1], w[2], w[3], blk_suspect(w));
  if (trail_bits(w) != value || trail_ordinal(w) != ordinal || w[1]) { fprintf(stderr, "a slot that does not hold its fields\n"); exit(2); }
  {  // in its place it decodes clean; a codeword of another ordinal, or with word 1 set, is as two flips, the words kept
    uint32_t moved[4] = {(ordinal + 1u) & ABFT_TRAIL_ORDINAL_MASK, 0u, w[2], w[3]}, set[4] = {ordinal, 1u, w[2], w[3]};
    blk_encode(moved);
    blk_encode(set);
    const TrailWord here = trail_decode_at(w, ordinal), a = trail_decode_at(moved, ordinal), b = trail_decode_at(set, ordinal);
    if (here.rc != 0 || trail_misplaced(w, ordinal) || blk_suspect(moved) || blk_suspect(set) || a.rc != -1 || b.rc != -1 ||
        memcmp(a.w, moved, sizeof moved) || memcmp(b.w, set, sizeof set) || !trail_misplaced(moved, ordinal) || !trail_misplaced(set, ordinal)) {
      fprintf(stderr, "a misplaced codeword is not told from one in its place\n");
      exit(2);
    }
  }
  for (int b = 0; b < 128; b++) {
    uint32_t f[4] = {w[0], w[1], w[2], w[3]};
    flip(f, b);
    if (!blk_suspect(f)) { fprintf(stderr, "flip of bit %d passes the hot test\n", b); exit(2); }
    const TrailWord t = trail_decode_at(f, ordinal);
    printf("s %d %d %016" PRIx64 " %08x %08x %08x %08x %u\n", b, t.rc, t.bits, t.w[0], t.w[1], t.w[2], t.w[3], t.bit);
  }
  unsigned fatal = 0, unchanged = 0;
  for (int a = 0; a < 128; a++)
    for (int b = a + 1; b < 128; b++) {
      uint32_t f[4] = {w[0], w[1], w[2], w[3]};
      flip(f, a);
      flip(f, b);
      const TrailWord t = trail_decode(f);
      fatal += blk_suspect(f) && t.rc == -1;
      unchanged += !memcmp(t.w, f, sizeof f) && t.bits == trail_bits(f);
    }
  printf("d %u %u\n", fatal, unchanged);
}

// slots as stored -> their values, each checked: a clean codeword of ordinal i, word 1 zero
static void print_values(const std::vector<double> &slots) {
  for (int i = 0; i < (int)slots.size() / ABFT_TRAIL_SLOT; i++) {
    uint32_t w[4];
    trail_load(slots.data(), i, w);
    if (blk_suspect(w) || trail_ordinal(w) != (uint32_t)i || w[1]) { fprintf(stderr, "written slot %d is no codeword of its ordinal\n", i); exit(2); }
    printf(" %016" PRIx64, trail_bits(w));
  }
}

template <class T> static void single(double threshold, uint32_t nev) {
  const uint64_t rr = hex(), rz = hex(), pw = hex(), nw = hex();
  const int frr = number(), frz = number(), fpw = number(), fnew = number();
  const double five = 5.0, m3 = -3.0, two = 2.0, six = 6.0, eight = 8.0;
  const uint64_t rec_in[4] = {rr, (uint64_t)__double_as_longlong(five), rz, (uint64_t)__double_as_longlong(m3)};
  const uint64_t rec_out[4] = {nw, (uint64_t)__double_as_longlong(six), nw, (uint64_t)__double_as_longlong(eight)};
  std::vector<double> in = poisoned(T::DOUBLES), pair = poisoned(T::PW_DOUBLES), out = poisoned(T::DOUBLES);
  for (int i = 0; i < T::LEN; i++) trail_put(in.data(), i, rec_in[i]);
  for (int i = 0; i < T::LEN; i++) trail_put(out.data(), i, rec_out[i]);
  trail_put(pair.data(), 0, pw);
  trail_put(pair.data(), 1, (uint64_t)__double_as_longlong(two));
  auto damage = [](std::vector<double> &rec, int ordinal, int bit) {
    uint32_t w[4];
    trail_load(rec.data(), ordinal, w);
    flip(w, bit);
    trail_store(rec.data(), ordinal, w);
  };
  damage(in, T::RR, frr);
  if (T::RZ != T::RR) damage(in, T::RZ, frz);
  damage(pair, 0, fpw);
  damage(out, T::RZ, fnew);
  int repairs = 0;
  auto get = [&](const std::vector<double> &rec, int ordinal) {
    uint32_t w[4];
    trail_load(rec.data(), ordinal, w);
    const TrailWord t = trail_decode(w);
    if (t.rc < 0) { fprintf(stderr, "a single flip decoded as two\n"); exit(2); }
    repairs += t.rc;
    return t.bits;
  };
  const uint64_t d_rr = get(in, T::RR), d_rz = T::RZ != T::RR ? get(in, T::RZ) : d_rr, d_pw = get(pair, 0);
  const uint64_t d_new = get(out, T::RZ);
  std::vector<double> handed = poisoned(T::DOUBLES), published = poisoned(T::DOUBLES);
  T::hand_on(d_rr, d_rz, handed.data(), nev);
  // (published: the next record's own values as the reduction's totals -- r.r' = r.z' = new --, whatever LIVE is)
  T::publish(__longlong_as_double((long long)nw), __longlong_as_double((long long)nw), published.data(), nev);
  printf("s %d %016" PRIx64 " %016" PRIx64, (int)T::live(d_rr, threshold),
         (uint64_t)__double_as_longlong(T::alpha(d_rr, d_rz, d_pw)), (uint64_t)__double_as_longlong(T::beta(d_rr, d_rz, d_new)));
  print_values(handed);
  print_values(published);
  printf(" %d\n", repairs);
}

int main(int argc, char **argv) {
  std::ifstream file;
  if (argc > 1) {
    file.open(argv[1]);
    if (!file) return 3;
  }
  src = argc > 1 ? static_cast<std::istream *>(&file) : &std::cin;
  std::string kind;
  while (*src >> kind) {
    if (kind == "slot") {
      const uint32_t ordinal = (uint32_t)number();
      play_slot(ordinal, hex());
    } else if (kind == "single") {
      const int quad = number();
      const double threshold = __longlong_as_double((long long)hex());
      const uint32_t nev = (uint32_t)hex();
      if (quad) single<TrailQuad>(threshold, nev);
      else single<TrailPair>(threshold, nev);
    } else {
      return 2;
    }
  }
  return 0;
}
