// The walk of the protected vector kernels on a CPU (tests/test_vecc_walk_host.py builds this with AddressSanitizer
// and UBSan and runs it as a program of its own).  ecc_device.h and vecc_walk.h are included as the kernels compile
// them, behind a few shims; the cold decode is a host functor over the shared repair (vecc_repair) that records what
// the device would queue.  A grid is simulated by running its chains one after another.
//
// stdin, one case after another, whitespace-separated:
//   OP VEC N THREADS BLOCKS RUNS ALPHA BETA   (OP: dot xr p r r_precond px_precond scrub; ALPHA, BETA: the
//                                              bits of the doubles, hex)
//   per operand, in the operation's order: its event ordinal, then its N words (hex)
// stdout, per case and run:
//   run R / v K words... (every operand after the run) / s CHAIN sums... (hex bits) / e STATUS INDEX BIT OPERAND (every
//   recorded event, in order) / c COLD-CALLS
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#define __device__
#define __forceinline__ inline
static inline long long __double_as_longlong(double v) { long long b; memcpy(&b, &v, sizeof b); return b; }
static inline double __longlong_as_double(long long b) { double v; memcpy(&v, &b, sizeof v); return v; }
// (a clang builtin that the matrix elements' code of ecc_device.h names, in a template nothing here instantiates)
static inline uint32_t __builtin_bitreverse32(uint32_t x) { uint32_t r = 0; for (int b = 0; b < 32; b++) r |= ((x >> b) & 1u) << (31 - b); return r; }

#include "ecc_device.h"
#include "vecc_walk.h"

struct Event { int status; uint32_t index, bit, operand; };

struct HostCold {
  std::vector<Event> events;
  long calls = 0;
  VeccWord operator()(uint64_t word, uint32_t index, uint32_t operand) {
    calls++;
    VeccWord o;
    uint32_t bit;
    vecc_repair(word, o, bit);
    if (o.rc) events.push_back({o.rc, index, bit, operand});
    return o;
  }
};

// an operand's storage: exactly n doubles, 16-byte aligned (the redzone starts behind the last one)
struct Vec {
  double *d = nullptr;
  explicit Vec(size_t n) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, (n ? n : 1) * sizeof(double))) abort();
    d = static_cast<double *>(p);
  }
  Vec(const Vec &) = delete;
  Vec(Vec &&o) noexcept : d(o.d) { o.d = nullptr; }
  ~Vec() { free(d); }
};

static double from_bits(uint64_t b) { return __longlong_as_double((long long)b); }
static uint64_t hex() {
  std::string t;
  if (!(std::cin >> t)) abort();
  return strtoull(t.c_str(), nullptr, 16);
}

template <int VEC, class OP>
static void grid(const OP &op, const VeccOperands<OP> &o, int n, int threads, int blocks, HostCold &cold) {
  for (int b = 0; b < blocks; b++) {
    for (int t = 0; t < threads; t++) {
      double acc[2] = {0.0, 0.0};
      vecc_walk<VEC>(op, o, n, ((long)b * threads + t) * VEC, (long)blocks * threads * VEC, cold, acc);
      printf("s %d", b * threads + t);
      for (int j = 0; j < OP::SUMS; j++) printf(" %016" PRIx64, vecc_bits(acc[j]));
      printf("\n");
    }
  }
}

template <class OP>
static void play(const OP &op, int vec, int n, int threads, int blocks, int runs) {
  std::vector<Vec> store;
  VeccOperands<OP> o;
  for (int k = 0; k < OP::N; k++) {
    int ord;
    if (!(std::cin >> ord)) abort();
    o.ord[k] = (uint32_t)ord;
    store.emplace_back((size_t)n);
    o.v[k] = store.back().d;
    for (int i = 0; i < n; i++) o.v[k][i] = from_bits(hex());
  }
  for (int r = 0; r < runs; r++) {
    HostCold cold;
    printf("run %d\n", r);
    if (vec == 2) grid<2>(op, o, n, threads, blocks, cold);
    else grid<1>(op, o, n, threads, blocks, cold);
    for (int k = 0; k < OP::N; k++) {
      printf("v %d", k);
      for (int i = 0; i < n; i++) printf(" %016" PRIx64, vecc_bits(o.v[k][i]));
      printf("\n");
    }
    for (const Event &e : cold.events) printf("e %d %u %u %u\n", e.status, e.index, e.bit, e.operand);
    printf("c %ld\n", cold.calls);
  }
}

int main() {
  std::string name;
  long cases = 0;
  while (std::cin >> name) {
    int vec, n, threads, blocks, runs;
    if (!(std::cin >> vec >> n >> threads >> blocks >> runs)) abort();
    const double alpha = from_bits(hex()), beta = from_bits(hex());
    printf("case %ld\n", cases++);
    if (name == "dot") play(VeccDot{}, vec, n, threads, blocks, runs);
    else if (name == "xr") play(VeccCalcXr{alpha}, vec, n, threads, blocks, runs);
    else if (name == "p") play(VeccCalcP{beta}, vec, n, threads, blocks, runs);
    else if (name == "r") play(VeccCalcR<false>{alpha}, vec, n, threads, blocks, runs);
    else if (name == "r_precond") play(VeccCalcR<true>{alpha}, vec, n, threads, blocks, runs);
    else if (name == "px_precond") play(VeccCalcPxPrecond{alpha, beta}, vec, n, threads, blocks, runs);
    else if (name == "scrub") play(VeccScrub{}, vec, n, threads, blocks, runs);
    else return 2;
  }
  return 0;
}
