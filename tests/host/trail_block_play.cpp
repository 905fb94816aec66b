// The protected block trail on a CPU (tests/test_trail_block_host.py builds this with AddressSanitizer and UBSan and
// runs it as a program of its own).  trail_ecc.h -- with struct_ecc.h, ecc_device.h and guard_protocol.h behind it --
// is included as the kernels compile it, behind a few shims.  Every record lives in a heap block of exactly its length,
// the destinations filled with a pattern no case contains, so a word too many or too few shows.
//
// input (a file named on the command line, else stdin), one request a line, every double as the hex of its bits:
//   tblock K PRECOND THRESHOLD NEV in[2K+2] pw[K+1] out[2K+2] tot[PRECOND ? 2K : K] NF (RECORD ORDINAL BIT) x NF
//      The start record, the SpMM's tail and the next record are encoded, every word under its ordinal; then the NF
//      damages are applied in order: bit BIT (0..127) of slot ORDINAL of RECORD (0 start, 1 tail, 2 next) is flipped,
//      or, BIT >= 1000, the slot is overwritten with the record's slot BIT - 1000 (a codeword in the wrong place).
//      Then an iteration is played as the kernels play it, through TrailBlock<K>'s own rules: the r half reads
//      (read_start, live_mask, read_scalars<false>) with one flipped bit stored back repaired, then the x / p half
//      (read_start, live_mask, read_scalars<true>) on what the r half left.
//   output, one line a request:
//      b MASK alpha[K] beta[K] handed-on[LEN] published[LEN] REPAIRS
//         alpha, beta: +0.0 for a frozen column and when no column is live.  handed-on (TrailBlock::hand_on) and
//         published (TrailBlock::publish<PRECOND>) are printed as the VALUES of the slots written, after the program
//         has checked that each is a clean codeword of its ordinal with word 1 zero.  REPAIRS: decodes with rc 1.
//      f WHERE RAW REPAIRS
//         two flips in a slot read.  WHERE: 0 the start record, 1 the tail (both: the r half stops, the record is
//         handed on through hand_on_raw; RAW: 1 when what it wrote is the stored start record word for word), 2 the
//         next record (the x / p half stops; RAW is 1).
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
static uint64_t bits_of(double v) { return (uint64_t)__double_as_longlong(v); }

// slots as stored -> their values, each checked: a clean codeword of ordinal i, word 1 zero
static void print_values(const std::vector<double> &slots) {
  for (int i = 0; i < (int)slots.size() / ABFT_TRAIL_SLOT; i++) {
    uint32_t w[4];
    trail_load(slots.data(), i, w);
    if (blk_suspect(w) || trail_ordinal(w) != (uint32_t)i || w[1]) { fprintf(stderr, "written slot %d is no codeword of its ordinal\n", i); exit(2); }
    printf(" %016" PRIx64, trail_bits(w));
  }
}

// the three records of an iteration and the checked read of a slot, as a launch's owner does it
struct Records {
  std::vector<double> in, pw, out;
  int repairs = 0, fatal_where = -1;
  std::vector<double> &of(uint32_t record) { return record == ABFT_TRAIL_START ? in : record == ABFT_TRAIL_PW ? pw : out; }
  TrailWord operator()(uint32_t record, int ordinal) {
    std::vector<double> &rec = of(record);
    if (ordinal < 0 || ABFT_TRAIL_SLOT * (ordinal + 1) > (int)rec.size()) { fprintf(stderr, "slot %d outside record %u\n", ordinal, record); exit(2); }
    uint32_t w[4];
    trail_load(rec.data(), ordinal, w);
    TrailWord t;
    if (blk_suspect(w) | trail_misplaced(w, (uint32_t)ordinal)) {  // the kernels' hot test, then their cold decode
      t = trail_decode_at(w, (uint32_t)ordinal);
    } else {
      t = TrailWord{{w[0], w[1], w[2], w[3]}, trail_bits(w), 0, 0u};
    }
    if (t.rc > 0) {
      repairs++;
      trail_store(rec.data(), ordinal, t.w);  // the owner's store-back
    }
    if (t.rc < 0 && fatal_where < 0) fatal_where = (int)record;
    return t;
  }
};

template <int K> static void tblock(bool precond, double threshold, uint32_t nev) {
  using T = TrailBlock<K>;
  Records R;
  R.in = poisoned(T::DOUBLES);
  R.pw = poisoned(T::PW_DOUBLES);
  R.out = poisoned(T::DOUBLES);
  for (int i = 0; i < T::LEN; i++) trail_put(R.in.data(), i, hex());
  for (int i = 0; i < T::PW_LEN; i++) trail_put(R.pw.data(), i, hex());
  for (int i = 0; i < T::LEN; i++) trail_put(R.out.data(), i, hex());
  const int s_len = precond ? 2 * K : K;
  std::vector<double> tot((size_t)s_len);
  tot.shrink_to_fit();
  for (int i = 0; i < s_len; i++) tot[(size_t)i] = __longlong_as_double((long long)hex());
  const int nf = number();
  for (int f = 0; f < nf; f++) {
    const int record = number(), ordinal = number(), bit = number();
    std::vector<double> &rec = R.of((uint32_t)record);
    if (ordinal < 0 || ABFT_TRAIL_SLOT * (ordinal + 1) > (int)rec.size()) abort();
    uint32_t w[4];
    if (bit >= 1000) {
      if (ABFT_TRAIL_SLOT * (bit - 1000 + 1) > (int)rec.size()) abort();
      trail_load(rec.data(), bit - 1000, w);
    } else {
      trail_load(rec.data(), ordinal, w);
      w[bit >> 5] ^= 1u << (bit & 31);
    }
    trail_store(rec.data(), ordinal, w);
  }
  const std::vector<double> stored = R.in;

  // the r half
  uint64_t v[T::VALUES];
  double alpha_r[K], alpha[K], beta[K];
  for (int j = 0; j < K; j++) alpha_r[j] = alpha[j] = beta[j] = 0.0;
  std::vector<double> handed = poisoned(T::DOUBLES), published = poisoned(T::DOUBLES);
  bool ok = T::read_start(R, v);
  uint32_t active = 0u;
  if (ok) {
    active = T::live_mask(v, threshold);
    if (active) ok = T::template read_scalars<false>(R, v, active, alpha_r, nullptr);
  }
  if (!ok) {
    // (what a repair stored back before the fatal slot was met is part of the record handed on, as on the device)
    std::vector<double> raw = poisoned(T::DOUBLES);
    T::hand_on_raw(R.in.data(), raw.data());
    bool same = true;
    for (int i = 0; i < T::DOUBLES; i++) {
      uint32_t a[4], b[4];
      if (i % 2) continue;
      trail_load(raw.data(), i / 2, a);
      trail_load(stored.data(), i / 2, b);
      const TrailWord was = trail_decode(b);  // a slot repaired on the way: compare with its repaired words
      const bool raw_same = !memcmp(a, b, sizeof a), repaired_same = was.rc == 1 && !memcmp(a, was.w, sizeof a);
      same = same && (raw_same || repaired_same);
    }
    printf("f %d %d %d\n", R.fatal_where, (int)same, R.repairs);
    return;
  }
  T::hand_on(v, handed.data(), nev);
  T::template publish<false>(tot.data(), active, v, published.data(), nev);  // (overwritten below when PRECOND)
  if (precond) {
    published = poisoned(T::DOUBLES);
    T::template publish<true>(tot.data(), active, v, published.data(), nev);
  }
  // the x / p half, on what the r half left
  uint64_t v2[T::VALUES];
  if (!T::read_start(R, v2) || memcmp(v, v2, sizeof v) || T::live_mask(v2, threshold) != active) {
    fprintf(stderr, "the x / p half decodes another start record than the r half\n");
    exit(2);
  }
  if (active && !T::template read_scalars<true>(R, v2, active, alpha, beta)) {
    printf("f %d 1 %d\n", R.fatal_where, R.repairs);
    return;
  }
  if (memcmp(alpha, alpha_r, sizeof alpha)) { fprintf(stderr, "the two halves form different alphas\n"); exit(2); }
  printf("b %u", active);
  for (int j = 0; j < K; j++) printf(" %016" PRIx64, bits_of(alpha[j]));
  for (int j = 0; j < K; j++) printf(" %016" PRIx64, bits_of(beta[j]));
  print_values(handed);
  print_values(published);
  printf(" %d\n", R.repairs);
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
    if (kind != "tblock") return 2;
    const int k = number(), precond = number();
    const double threshold = __longlong_as_double((long long)hex());
    const uint32_t nev = (uint32_t)hex();
    if (k == 1) tblock<1>(precond != 0, threshold, nev);
    else if (k == 3) tblock<3>(precond != 0, threshold, nev);
    else if (k == 8) tblock<8>(precond != 0, threshold, nev);
    else return 2;
  }
  return 0;
}
