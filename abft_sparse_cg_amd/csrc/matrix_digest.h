// matrix_digest.h -- digests of a matrix's stored arrays: the pure part.  No HIP in here: the
// kernels (kernels.hip), the C ABI's host code (abft_hip.hip) and a CPU program (tests/host/matrix_digest_play.cpp)
// compile this text.
//
// A SEGMENT is one device allocation of a matrix that kernels only read, or only repair (an ECC repair stores the
// original word back).  It is viewed as little-endian 32-bit words w[0..n) over the WHOLE allocation, padding included
// -- kernels may load the padding --; when the byte length is no multiple of 4 the last word is zero-extended.
//
//     D(segment) = sum over i of  w[i] * (2 i + 1)    mod 2^64,        n <= 2^31  (else ABFT_ERR_RANGE)
//
// The sum is commutative integer addition: any order of summation, and integer atomics, give the same bits.
//
// What it detects, with certainty.  With n <= 2^31 every weight 2 i + 1 is odd and below 2^32 (one 32 x 32 -> 64 bit
// multiply-add per word).
//   * ONE flipped bit, bit b of word i, changes D by +-2^b (2 i + 1).  The weight is odd, so the change is 2^b times an
//     odd number with b <= 31: never 0 mod 2^64.
//   * TWO flipped bits change D by t1 + t2 with t_k = +-2^(b_k) (2 i_k + 1).  Each |t_k| < 2^31 * 2^32 = 2^63, so
//     |t1 + t2| < 2^64 and the sum is 0 mod 2^64 only when it is 0 as an integer: t1 = -t2, hence
//     2^(b_1) (2 i_1 + 1) = 2^(b_2) (2 i_2 + 1), and -- an integer has one power of two times one odd number -- b_1 = b_2
//     and i_1 = i_2: the same bit of the same word, flipped twice, which is no change of the segment at all.
//   So every single and every double flip inside a segment changes D.  Three or more flips can cancel.
//   * Two unequal words w[i], w[j] swapped change D by (w[i] - w[j]) (2 j - 2 i): |.| < 2^32 * 2^32, not 0.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ABFT_DIGEST_HD __host__ __device__ __forceinline__
#else
#define ABFT_DIGEST_HD inline
#endif

#define ABFT_DIGEST_MAX_WORDS 0x80000000ull  // n <= 2^31

// The segment kinds.  An event (ABFT_EV_MATRIX_DIGEST) carries one as its index, so a line names its segment without
// the matrix.  The mutable buffers -- progress boards (pace), debug buffers, the moved list, fuse_partials -- are no
// segments: ABFT_SEG_NONE.
enum {
  ABFT_SEG_NONE = 0,
  // CSR (CsrDev, CsrCompact, CsrPacked, CsrPackedFast, CsrStruct)
  ABFT_SEG_COLS = 1,
  ABFT_SEG_VALS = 2,
  ABFT_SEG_ROWPTR = 3,
  ABFT_SEG_BLK = 4,
  ABFT_SEG_ORIG_INDEX = 5,
  ABFT_SEG_POS_OF_ORIG = 6,
  ABFT_SEG_GIDX = 7,
  ABFT_SEG_COLS16 = 8,
  ABFT_SEG_CBASE = 9,
  ABFT_SEG_CODE16 = 10,
  ABFT_SEG_PDESC = 11,
  ABFT_SEG_PAL = 12,
  ABFT_SEG_FAST = 13,
  ABFT_SEG_ROWEXT = 14,
  ABFT_SEG_SBLK = 15,
  // panels (CsrPanels; CSR and COO)
  ABFT_SEG_SEG_BASE = 16,
  ABFT_SEG_SEG_PTR = 17,
  // sweep (SweepLayout)
  ABFT_SEG_WBASE = 18,
  ABFT_SEG_COUNTS = 19,
  // slice (SliceLayout)
  ABFT_SEG_SUB = 20,
  ABFT_SEG_RID = 21,
  // COO (CooDev)
  ABFT_SEG_ELEMS = 22,
  ABFT_SEG_GRP_PTR = 23,
  ABFT_SEG_COO_BLK = 24,
  ABFT_SEG_AS_CREATED = 25,
  ABFT_SEG_COO_ORIG_INDEX = 26,
  ABFT_SEG_COO_POS_OF_ORIG = 27,
  ABFT_SEG_COO_GIDX = 28,
  ABFT_SEG_COUNT = 29
};

// the name of a kind ("?" outside the list); the names are distinct
ABFT_DIGEST_HD const char *abft_seg_name(uint32_t kind) {
  switch (kind) {
    case ABFT_SEG_NONE: return "none";
    case ABFT_SEG_COLS: return "cols";
    case ABFT_SEG_VALS: return "vals";
    case ABFT_SEG_ROWPTR: return "rowptr";
    case ABFT_SEG_BLK: return "blk";
    case ABFT_SEG_ORIG_INDEX: return "orig_index";
    case ABFT_SEG_POS_OF_ORIG: return "pos_of_orig";
    case ABFT_SEG_GIDX: return "gidx";
    case ABFT_SEG_COLS16: return "cols16";
    case ABFT_SEG_CBASE: return "cbase";
    case ABFT_SEG_CODE16: return "code16";
    case ABFT_SEG_PDESC: return "pdesc";
    case ABFT_SEG_PAL: return "pal";
    case ABFT_SEG_FAST: return "fast";
    case ABFT_SEG_ROWEXT: return "rowext";
    case ABFT_SEG_SBLK: return "sblk";
    case ABFT_SEG_SEG_BASE: return "seg_base";
    case ABFT_SEG_SEG_PTR: return "seg_ptr";
    case ABFT_SEG_WBASE: return "wbase";
    case ABFT_SEG_COUNTS: return "counts";
    case ABFT_SEG_SUB: return "sub";
    case ABFT_SEG_RID: return "rid";
    case ABFT_SEG_ELEMS: return "elems";
    case ABFT_SEG_GRP_PTR: return "grp_ptr";
    case ABFT_SEG_COO_BLK: return "coo_blk";
    case ABFT_SEG_AS_CREATED: return "as_created";
    case ABFT_SEG_COO_ORIG_INDEX: return "coo_orig_index";
    case ABFT_SEG_COO_POS_OF_ORIG: return "coo_pos_of_orig";
    case ABFT_SEG_COO_GIDX: return "coo_gidx";
    default: return "?";
  }
}

// words of a segment of `bytes` bytes (the last one zero-extended); false: more than 2^31, no digest
ABFT_DIGEST_HD bool digest_word_count(uint64_t bytes, uint64_t *n) {
  *n = (bytes + 3u) >> 2;
  return *n <= ABFT_DIGEST_MAX_WORDS;
}

// one word's share: i < 2^31, so the weight fits 32 bits and the product is one 32 x 32 -> 64 multiply-add
ABFT_DIGEST_HD uint64_t digest_term(uint64_t acc, uint32_t w, uint32_t i) {
  return acc + (uint64_t)w * (uint64_t)(2u * i + 1u);
}

// the bytes [4 i, 4 i + count) of a segment as one zero-extended little-endian word, count 1..4
ABFT_DIGEST_HD uint32_t digest_tail_word(const unsigned char *p, uint32_t count) {
  uint32_t w = 0u;
  for (uint32_t k = 0; k < count; k++) w |= (uint32_t)p[k] << (8u * k);
  return w;
}

// the whole digest, serially: the definition (0 OK, -4 = ABFT_ERR_RANGE: more than 2^31 words, *out untouched)
ABFT_DIGEST_HD int digest_segment(const void *base, uint64_t bytes, uint64_t *out) {
  uint64_t n;
  if (!digest_word_count(bytes, &n)) return -4;
  const unsigned char *p = static_cast<const unsigned char *>(base);
  const uint64_t full = bytes >> 2;
  uint64_t acc = 0u;
  for (uint64_t i = 0; i < full; i++) acc = digest_term(acc, digest_tail_word(p + 4u * i, 4u), (uint32_t)i);
  if (n > full) acc = digest_term(acc, digest_tail_word(p + 4u * full, (uint32_t)(bytes & 3u)), (uint32_t)full);
  *out = acc;
  return 0;
}

// One row of the segment table matrix_digest_kernel walks (device memory; built when a matrix is armed).  The kernel
// reads `quads` 16-byte groups with one load per lane each, and the `tail` bytes behind them (0..15) apart.
struct DigestSeg {
  const void *base;  // the allocation (16-byte aligned: every allocation of the device runtime is)
  uint32_t quads;    // bytes / 16; <= 2^29
  uint32_t tail;     // bytes % 16
  uint32_t kind;     // ABFT_SEG_*
  uint32_t pad;
};
#define ABFT_DIGEST_MAX_SEGS 32u  // rows of a table: more than any matrix has (ABFT_SEG_COUNT kinds, each at most once)
