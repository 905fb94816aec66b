// The protected CSR row structure on a CPU (tests/test_struct_ecc_host.py builds this with AddressSanitizer and UBSan
// and runs it as a program of its own).  struct_ecc.h and ecc_device.h are included as the kernels compile them, behind
// a few shims; layout_plan.h plans the test matrices as abft_hip.hip's create does for a structure-protected matrix
// (force_stream, neither compact nor packed blocks).
//
// stdin, one request per line, whitespace-separated (numbers decimal unless said otherwise):
//   row RS RE            -> row WORD / s BIT RC REPAIRED REPORTED-BIT (x 64, every single flip) / d FATAL UNCHANGED (of
//                           the 2016 double flips: how many were fatal, how many left the word as it was)
//   blk W0 W1 W2 W3      -> blk E0 E1 E2 E3 SUSPECT / s BIT RC R0 R1 R2 R3 REPORTED-BIT (x 128) / d FATAL UNCHANGED (of 8128)
//   limit N NNZ          -> limit RC
//   plan BLOCK CSR_TILE COO_TILE PANEL_ROWS SWEEP_EPT MAX_SEGMENTS N NNZ rows... cols...
//                        -> plan LAYOUT COMPACT PACKED NBLK then x y z w of every block
// words are printed in hex
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
static inline uint32_t __builtin_bitreverse32(uint32_t x) { uint32_t r = 0; for (int b = 0; b < 32; b++) r |= ((x >> b) & 1u) << (31 - b); return r; }

#include "struct_ecc.h"
#include "layout_plan.h"

static void play_row(uint32_t rs, uint32_t re) {
  const uint64_t w = rowext_encode(rs, re);
  if (vecc_suspect(w) || rowext_start(w) != rs || rowext_end(w) != re || (w >> 63)) { fprintf(stderr, "row word %016" PRIx64 " is no codeword of its fields\n", w); exit(2); }
  printf("row %016" PRIx64 "\n", w);
  for (uint32_t b = 0; b < 64; b++) {
    const uint64_t f = w ^ (1ull << b);
    VeccWord o;
    uint32_t bit = 999u;
    if (!vecc_suspect(f)) { fprintf(stderr, "flip of bit %u passes the hot test\n", b); exit(2); }
    vecc_repair(f, o, bit);
    printf("s %u %d %016" PRIx64 " %u\n", b, o.rc, o.w, bit);
  }
  unsigned fatal = 0, unchanged = 0;
  for (uint32_t a = 0; a < 64; a++)
    for (uint32_t b = a + 1; b < 64; b++) {
      const uint64_t f = w ^ (1ull << a) ^ (1ull << b);
      VeccWord o;
      uint32_t bit;
      const uint32_t sus = vecc_suspect(f);
      vecc_repair(f, o, bit);
      fatal += sus && o.rc == -1;
      unchanged += o.w == f;
    }
  printf("d %u %u\n", fatal, unchanged);
}

static void play_blk(const uint32_t in[4]) {
  uint32_t w[4] = {in[0], in[1], in[2], in[3]};
  blk_encode(w);
  printf("blk %08x %08x %08x %08x %u\n", w[0], w[1], w[2], w[3], blk_suspect(w));
  for (uint32_t b = 0; b < 128; b++) {
    uint32_t f[4] = {w[0], w[1], w[2], w[3]};
    f[b >> 5] ^= 1u << (b & 31u);
    if (!blk_suspect(f)) { fprintf(stderr, "flip of bit %u passes the hot test\n", b); exit(2); }
    StructBlk o;
    uint32_t bit = 999u;
    blk_repair(f, o, bit);
    printf("s %u %d %08x %08x %08x %08x %u\n", b, o.rc, o.w[0], o.w[1], o.w[2], o.w[3], bit);
  }
  unsigned fatal = 0, unchanged = 0;
  for (uint32_t a = 0; a < 128; a++)
    for (uint32_t b = a + 1; b < 128; b++) {
      uint32_t f[4] = {w[0], w[1], w[2], w[3]};
      f[a >> 5] ^= 1u << (a & 31u);
      f[b >> 5] ^= 1u << (b & 31u);
      StructBlk o;
      uint32_t bit;
      const uint32_t sus = blk_suspect(f);
      blk_repair(f, o, bit);
      fatal += sus && o.rc == -1;
      unchanged += !memcmp(o.w, f, sizeof f);
    }
  printf("d %u %u\n", fatal, unchanged);
}

static void play_plan() {
  PlanGeometry geo;
  int n = 0, nnz = 0;
  std::cin >> geo.block >> geo.csr_tile >> geo.coo_tile >> geo.panel_rows >> geo.sweep_ept >> geo.max_segments >> n >> nnz;
  std::vector<uint32_t> rows((size_t)nnz + 1), cols((size_t)nnz + 1);
  std::vector<double> vals((size_t)nnz + 1, 1.0);
  for (int i = 0; i < nnz; i++) std::cin >> rows[(size_t)i];
  for (int i = 0; i < nnz; i++) std::cin >> cols[(size_t)i];
  if (!std::cin) { fprintf(stderr, "short plan request\n"); exit(2); }
  LayoutKnobs knobs;  // as create_csr plans a structure-protected matrix
  knobs.compact = knobs.packed = false;
  PalettePool pool;
  CsrPlan plan;
  auto none = [](auto) { return (uint64_t)0; };
  for (int mode_none = 0; mode_none < 2; mode_none++) {
    plan_csr(geo, knobs, mode_none != 0, false, true, cols.data(), rows.data(), vals.data(), n, n, nnz, none, none, pool, plan);
    if (plan.layout != Layout::Stream || plan.compact.any || plan.packed.any) { fprintf(stderr, "not a plain streaming plan\n"); exit(2); }
  }
  printf("plan %zu", plan.blk.size());
  for (const Blk &b : plan.blk) printf(" %u %u %u %u", b.x, b.y, b.z, b.w);
  printf("\n");
}

int main() {
  std::string what;
  while (std::cin >> what) {
    if (what == "row") {
      uint32_t rs, re;
      std::cin >> rs >> re;
      play_row(rs, re);
    } else if (what == "blk") {
      uint32_t w[4];
      std::cin >> w[0] >> w[1] >> w[2] >> w[3];
      play_blk(w);
    } else if (what == "limit") {
      uint64_t n, nnz;
      std::cin >> n >> nnz;
      printf("limit %d\n", struct_limit(n, nnz));
    } else if (what == "plan") {
      play_plan();
    } else {
      fprintf(stderr, "unknown request %s\n", what.c_str());
      return 2;
    }
  }
  return 0;
}
