// struct_ecc.h -- the protected CSR row structure: the pure part.  No HIP in here: the kernels
// (kernels.hip), the C ABI's host code (abft_hip.hip) and a CPU program (tests/host/struct_ecc_play.cpp) compile this
// text.  The codes themselves are ecc_device.h's, unchanged.
//
// A structure-protected matrix stores no plain rowptr.  It stores
//   * one ROW EXTENT WORD per row r, 64 bit, under the (64, 57) code of the protected vectors:
//       bits 0..6    the code (vecc_mask: bit 0 overall parity, bits 1..6 the Hamming checks)
//       bits 7..34   rowptr[r]
//       bits 35..62  rowptr[r + 1]
//       bit  63      a data bit, always 0
//     Each row's word is read by exactly one lane of one workgroup per launch, so a repair, its store-back and its event
//     have one owner; the neighbour's pointer is duplicated for that.
//   * the ROW-BLOCK DESCRIPTORS {first row, end row | uniform flag, first element, end element}, 128 bit, read as a COO
//     element {col = word 0, row = word 1, value = words 2, 3} of the reference's code in secded form: the check byte in
//     bits 24..31 of word 0 (first row < 2^24).  The uniform flag, bit 31 of word 1, is data like the rest.
// Both codes are SECDED whatever the elements' mode is.
#pragma once
#include <stdint.h>

#include "ecc_device.h"

#if defined(__HIPCC__)
#define ABFT_STRUCT_HD __host__ __device__ __forceinline__
#else
#define ABFT_STRUCT_HD inline
#endif

#define ABFT_STRUCT_PTR_BITS 28u
#define ABFT_STRUCT_PTR_MASK 0x0FFFFFFFull
#define ABFT_STRUCT_MAX_NNZ (1u << 28)   // nnz < this: a row pointer is a 28-bit field
#define ABFT_STRUCT_MAX_ROWS (1u << 24)  // N <= this: a descriptor's first row leaves bits 24..31 free
// the kind of a structure event, bits 8..15 of abft_event::bit (bits 0..7: the word bit)
#define ABFT_STRUCT_ROW 0u
#define ABFT_STRUCT_BLOCK 1u

// ---- the limit test: 0 fits, 1 too many non-zeros, 2 too many rows ----
ABFT_STRUCT_HD int struct_limit(uint64_t n_rows, uint64_t nnz) {
  if (nnz >= ABFT_STRUCT_MAX_NNZ) return 1;
  if (n_rows > ABFT_STRUCT_MAX_ROWS) return 2;
  return 0;
}

// ---- row extent words: fields ----
ABFT_STRUCT_HD uint64_t rowext_pack(uint32_t rs, uint32_t re) {
  return (((uint64_t)rs & ABFT_STRUCT_PTR_MASK) << 7) | (((uint64_t)re & ABFT_STRUCT_PTR_MASK) << 35);
}
ABFT_STRUCT_HD uint32_t rowext_start(uint64_t w) { return (uint32_t)((w >> 7) & ABFT_STRUCT_PTR_MASK); }
ABFT_STRUCT_HD uint32_t rowext_end(uint64_t w) { return (uint32_t)((w >> 35) & ABFT_STRUCT_PTR_MASK); }

// ---- row extent words: the code (vecc_encode's integer half: the 7 code bits over a word whose own are clear) ----
__device__ __forceinline__ uint64_t rowext_code(uint64_t w) {
  w &= ~ABFT_VECC_CODE_BITS;
  const uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
  const uint32_t c = ((popc(vecc_fold<0>(lo, hi)) & 1u) << 1) | ((popc(vecc_fold<1>(lo, hi)) & 1u) << 2) |
                     ((popc(vecc_fold<2>(lo, hi)) & 1u) << 3) | ((popc(vecc_fold<3>(lo, hi)) & 1u) << 4) |
                     ((popc(vecc_fold<4>(lo, hi)) & 1u) << 5) | ((popc(vecc_fold<5>(lo, hi)) & 1u) << 6);
  const uint32_t par = popc(lo ^ hi ^ c) & 1u;
  return w | c | par;
}
__device__ __forceinline__ uint64_t rowext_encode(uint32_t rs, uint32_t re) { return rowext_code(rowext_pack(rs, re)); }
// hot test: vecc_suspect(word); cold decode: vecc_repair(word, o, bit) -- o.rc 1 repaired (`bit` the one), -1 two flips

// ---- row-block descriptors ----
// what a cold decode hands back: the words as repaired and the verdict (1 repaired, -1 two flips: the words as they are)
struct StructBlk { uint32_t w[4]; int rc; };

// w: {first row, end row | flag, first element, end element}, first row < 2^24 -> the stored words
__device__ __forceinline__ void blk_encode(uint32_t *w) {
  w[0] &= ABFT_COLMASK;
  ecc_encode<FMT_COO>(MODE_SECDED, w);
}
// the first row of a stored descriptor
ABFT_STRUCT_HD uint32_t blk_first_row(uint32_t w0) { return w0 & ABFT_COLMASK; }
// hot test: one ecc_any_check plus parity
__device__ __forceinline__ uint32_t blk_suspect(const uint32_t *w) { return ecc_any_check<FMT_COO>(w) | ecc_parity<FMT_COO>(w); }
// Cold decode (the reference's secded rule, COO/CPUContext.cpp:346-373): odd parity is one flipped bit -- located by
// the syndrome, or the parity bit itself (bit 24) when the syndrome is clear -- and is flipped back; a set syndrome
// under even parity is two flips.  `bit`: the flipped bit, numbered as the COO element's 128.
__device__ __forceinline__ void blk_repair(const uint32_t *w, StructBlk &o, uint32_t &bit) {
  o.w[0] = w[0]; o.w[1] = w[1]; o.w[2] = w[2]; o.w[3] = w[3]; o.rc = 0;
  bit = 0u;
  const uint32_t h = ecc_hamming<FMT_COO>(w);
  if (ecc_parity<FMT_COO>(w)) {
    bit = h ? ecc_position_to_bit<FMT_COO>(h) : 24u;
    // static word selects keep the descriptor in registers (all 127 positions are taken: bit < 128)
    for (int k = 0; k < 4; k++)
      if ((bit >> 5) == (uint32_t)k) o.w[k] ^= 1u << (bit & 31u);
    o.rc = 1;
  } else if (h) {
    o.rc = -1;
  }
}
