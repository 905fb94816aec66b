// The matrix digest on a CPU (tests/test_matrix_digest_host.py builds this with AddressSanitizer and UBSan and runs it
// as a program of its own).  matrix_digest.h is included as the kernels and the C ABI's host code compile it.
//
// stdin, one request per line, whitespace-separated; a segment is given as its bytes in hex ("-": no byte at all):
//   digest HEX     -> digest D WALK       D by digest_segment (the definition), WALK by the cut the kernel makes of a
//                                         table row: 16-byte groups in a scrambled order, then the tail bytes apart
//   flips HEX      -> flips S SC P PC     of the S single flips SC change D, of the P double flips PC do
//   swaps HEX      -> swaps P PC          of the P pairs of unequal words PC change D when swapped
//   limit BYTES    -> limit RC WORDS      digest_word_count, and digest_segment's refusal (which reads no byte)
//   names          -> name KIND NAME (x ABFT_SEG_COUNT), then name COUNT ? for the first kind past the list
// digests are printed in hex
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "matrix_digest.h"

static std::vector<unsigned char> bytes_of(const std::string &hex) {
  std::vector<unsigned char> out;
  if (hex == "-") return out;
  if (hex.size() % 2) { fprintf(stderr, "odd hex string\n"); exit(2); }
  for (size_t k = 0; k < hex.size(); k += 2) out.push_back((unsigned char)strtoul(hex.substr(k, 2).c_str(), nullptr, 16));
  return out;
}

static uint64_t digest(const std::vector<unsigned char> &b) {
  // an exact-size heap copy: a read past the segment is AddressSanitizer's to find
  unsigned char *p = (unsigned char *)malloc(b.size() ? b.size() : 1);
  if (!b.empty()) memcpy(p, b.data(), b.size());
  uint64_t d = 0xDEADu;
  const int rc = digest_segment(p, b.size(), &d);
  free(p);
  if (rc) { fprintf(stderr, "digest_segment refused %zu bytes\n", b.size()); exit(2); }
  return d;
}

// the same on the vector's own storage (the exhaustive loops: millions of digests of one small segment)
static uint64_t digest_in_place(const std::vector<unsigned char> &b) {
  uint64_t d = 0;
  if (digest_segment(b.data(), b.size(), &d)) { fprintf(stderr, "digest_segment refused %zu bytes\n", b.size()); exit(2); }
  return d;
}

// the kernel's cut of one table row: every 16-byte group once, in an order that is not the definition's, then the
// tail's words by digest_tail_word
static uint64_t walk(const std::vector<unsigned char> &b) {
  unsigned char *p = (unsigned char *)malloc(b.size() ? b.size() : 1);
  if (!b.empty()) memcpy(p, b.data(), b.size());
  const DigestSeg seg{p, (uint32_t)(b.size() >> 4), (uint32_t)(b.size() & 15u), ABFT_SEG_COLS, 0u};
  uint64_t lanes[7] = {0, 0, 0, 0, 0, 0, 0};  // partial sums, added up at the end as the workgroups' atomics are
  for (uint32_t q = seg.quads; q-- > 0;) {
    uint32_t w[4];
    memcpy(w, p + 16u * (size_t)q, 16);
    for (uint32_t j = 0; j < 4; j++) lanes[q % 7u] = digest_term(lanes[q % 7u], w[j], 4u * q + j);
  }
  for (uint32_t t = 0; t < (seg.tail + 3u) / 4u; t++) {
    const uint32_t left = seg.tail - 4u * t;
    lanes[t] = digest_term(lanes[t], digest_tail_word(p + (size_t)seg.quads * 16u + 4u * t, left < 4u ? left : 4u), 4u * seg.quads + t);
  }
  free(p);
  uint64_t d = 0;
  for (uint64_t l : lanes) d += l;
  return d;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, hex;
    in >> op;
    if (op == "digest") {
      in >> hex;
      const auto b = bytes_of(hex);
      printf("digest %016" PRIx64 " %016" PRIx64 "\n", digest(b), walk(b));
    } else if (op == "flips") {
      in >> hex;
      auto b = bytes_of(hex);
      const uint64_t d0 = digest_in_place(b);
      const size_t nbits = 8 * b.size();
      unsigned long long s = 0, sc = 0, p = 0, pc = 0;
      for (size_t i = 0; i < nbits; i++) {
        b[i >> 3] ^= (unsigned char)(1u << (i & 7));
        s++;
        sc += digest_in_place(b) != d0;
        for (size_t j = i + 1; j < nbits; j++) {
          b[j >> 3] ^= (unsigned char)(1u << (j & 7));
          p++;
          pc += digest_in_place(b) != d0;
          b[j >> 3] ^= (unsigned char)(1u << (j & 7));
        }
        b[i >> 3] ^= (unsigned char)(1u << (i & 7));
      }
      printf("flips %llu %llu %llu %llu\n", s, sc, p, pc);
    } else if (op == "swaps") {
      in >> hex;
      auto b = bytes_of(hex);
      const uint64_t d0 = digest_in_place(b);
      const size_t n = b.size() / 4;
      unsigned long long p = 0, pc = 0;
      for (size_t i = 0; i < n; i++)
        for (size_t j = i + 1; j < n; j++) {
          if (!memcmp(&b[4 * i], &b[4 * j], 4)) continue;
          unsigned char t[4];
          memcpy(t, &b[4 * i], 4); memcpy(&b[4 * i], &b[4 * j], 4); memcpy(&b[4 * j], t, 4);
          p++;
          pc += digest_in_place(b) != d0;
          memcpy(t, &b[4 * i], 4); memcpy(&b[4 * i], &b[4 * j], 4); memcpy(&b[4 * j], t, 4);
        }
      printf("swaps %llu %llu\n", p, pc);
    } else if (op == "limit") {
      unsigned long long bytes = 0;
      in >> bytes;
      uint64_t n = 0, d = 0x5EEDu;
      const bool fits = digest_word_count(bytes, &n);
      // a refused segment is not read: no memory stands behind this pointer
      const int rc = fits ? 0 : digest_segment(nullptr, bytes, &d);
      if (!fits && d != 0x5EEDu) { fprintf(stderr, "a refused digest wrote its output\n"); return 2; }
      printf("limit %d %" PRIu64 "\n", rc, n);
    } else if (op == "names") {
      for (uint32_t k = 0; k <= ABFT_SEG_COUNT; k++) printf("name %u %s\n", k, abft_seg_name(k));
    } else if (!op.empty()) {
      fprintf(stderr, "unknown request %s\n", op.c_str());
      return 2;
    }
  }
  return 0;
}
