// The stop-test protocol of the guarded CG kernels on a CPU (tests/test_guard_protocol_host.py builds this with
// AddressSanitizer and UBSan and runs it as a program of its own).  guard_protocol.h is included as kernels.hip
// compiles it, behind a few shims.  Every record lives in a heap block of exactly its length, the destinations filled
// with a pattern no case contains, so a word too many or too few shows.
//
// input (a file named on the command line, else stdin), one case a line, every double as the hex of its bits:
//   single QUAD THRESHOLD NEV in[4] pw out[4]            (QUAD 0: GuardPair, the first two words of in / out count)
//   block K PRECOND THRESHOLD NEV in[2K+2] pw[K+1] out[2K+2] tot[PRECOND ? 2K : K]
// output, one line a case:
//   s LIVE alpha beta handed-on[LEN]
//   b MASK alpha[K] beta[K] handed-on[LEN] published[LEN]   (published: with MASK and tot, whatever MASK is)
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

#include "guard_protocol.h"

static const uint64_t POISON = 0x7ff4dead0000beefull;
static std::istream *src;

static uint64_t bits(double v) { return (uint64_t)__double_as_longlong(v); }
static uint64_t hex() {
  std::string t;
  if (!(*src >> t)) abort();
  return strtoull(t.c_str(), nullptr, 16);
}
static double value() { return __longlong_as_double((long long)hex()); }
// n doubles read from the input (fill) or holding the pattern
static std::vector<double> record(int n, bool fill) {
  std::vector<double> r((size_t)n);
  for (int i = 0; i < n; i++) r[(size_t)i] = fill ? value() : __longlong_as_double((long long)POISON);
  r.shrink_to_fit();
  return r;
}
static void print(const std::vector<double> &r) {
  for (double v : r) printf(" %016" PRIx64, bits(v));
}

template <class REC> static void single(double threshold, uint32_t nev) {
  std::vector<double> four = record(4, true);
  const double pw = value();
  std::vector<double> left = record(4, true);
  const std::vector<double> in(four.begin(), four.begin() + REC::LEN), out(left.begin(), left.begin() + REC::LEN);
  std::vector<double> handed = record(REC::LEN, false);
  REC::hand_on(in.data(), handed.data(), nev);
  printf("s %d %016" PRIx64 " %016" PRIx64, (int)REC::live(in.data(), threshold), bits(REC::alpha(in.data(), pw)),
         bits(REC::beta(in.data(), out.data())));
  print(handed);
  printf("\n");
}

template <int K> static void block(bool precond, double threshold, uint32_t nev) {
  using REC = GuardBlock<K>;
  const std::vector<double> in = record(REC::LEN, true), pw = record(REC::PW_LEN, true), out = record(REC::LEN, true);
  const std::vector<double> tot = record(precond ? 2 * K : K, true);
  const uint32_t active = REC::live_mask(in.data(), threshold);
  printf("b %u", active);
  for (int j = 0; j < K; j++) printf(" %016" PRIx64, bits(REC::alpha(in.data(), pw.data(), j)));
  for (int j = 0; j < K; j++) printf(" %016" PRIx64, bits(REC::beta(in.data(), out.data(), j)));
  std::vector<double> handed = record(REC::LEN, false), published = record(REC::LEN, false);
  REC::hand_on(in.data(), handed.data(), nev);
  if (precond) REC::template publish<true>(tot.data(), active, in.data(), published.data(), nev);
  else REC::template publish<false>(tot.data(), active, in.data(), published.data(), nev);
  print(handed);
  print(published);
  printf("\n");
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
    int a, b = 0;
    if (!(*src >> a)) abort();
    if (kind == "block" && !(*src >> b)) abort();
    const double threshold = value();
    const uint32_t nev = (uint32_t)hex();
    if (kind == "single" && a == 0) single<GuardPair>(threshold, nev);
    else if (kind == "single" && a == 1) single<GuardQuad>(threshold, nev);
    else if (kind == "block" && a == 1) block<1>(b != 0, threshold, nev);
    else if (kind == "block" && a == 2) block<2>(b != 0, threshold, nev);
    else if (kind == "block" && a == 3) block<3>(b != 0, threshold, nev);
    else if (kind == "block" && a == 8) block<8>(b != 0, threshold, nev);
    else return 2;
  }
  return 0;
}
