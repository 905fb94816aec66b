/*
 * abft_hip.h -- C ABI of the MI355X (gfx950) ABFT sparse-CG engine.
 *
 * This is the drop-in boundary for the `-t hip` target of abft-sparse-cg: one
 * entry point per virtual method of the reference plugin interface
 * (reference CGContext.h:13-36), plus the few additive calls a device backend
 * needs (stream hand-over, event drain, shard creation, profiling).  Plain
 * pointers and sizes only: no C++ types, no torch types.
 *
 * Conventions
 *   - every call returns ABFT_OK (0) or a negative ABFT_ERR_* code; the text of
 *     the last failure on the calling thread is abft_hip_last_error();
 *   - handles are opaque and owned by the library until the matching destroy;
 *   - host arrays passed to *_create_* are copied before the call returns
 *     (reference cg.cpp:418-422 frees them right after create_matrix);
 *   - spmv / calc_p / copy are asynchronous on the context's HIP stream;
 *     dot / calc_xr / map / drain_events synchronise it (reference semantics:
 *     CGContext.h:27-30 return the scalar by value);
 *   - nothing here prints or exits: ECC / constraint events are queued on the
 *     device and handed to the caller by abft_hip_drain_events(), which the
 *     host-side HIPContext turns into the reference's exact printf lines and
 *     exit(1) (reference CSR/CPUContext.cpp:175-400).
 */
#ifndef ABFT_HIP_H
#define ABFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ABFT_OK 0
#define ABFT_ERR_INVALID (-1)  /* bad argument / shape mismatch              */
#define ABFT_ERR_HIP (-2)      /* a HIP runtime call failed                  */
#define ABFT_ERR_NOMEM (-3)    /* host or device allocation failed           */
#define ABFT_ERR_RANGE (-4)    /* column index does not fit the ECC layout   */
#define ABFT_ERR_NODEVICE (-5) /* no usable gfx950 device                    */

/* -m modes: reference CSR/CPUContext.cpp:415-420, COO/CPUContext.cpp:383-388 */
typedef enum {
  ABFT_MODE_NONE = 0,
  ABFT_MODE_CONSTRAINTS = 1,
  ABFT_MODE_SED = 2,
  ABFT_MODE_SEC7 = 3,
  ABFT_MODE_SEC8 = 4,
  ABFT_MODE_SECDED = 5
} abft_mode;

/* storage format: cg-csr links CSR/, cg-coo links COO/ (reference Makefile:22-52) */
typedef enum { ABFT_FMT_CSR = 0, ABFT_FMT_COO = 1 } abft_format;

/* reference CGContext.h:11 */
typedef enum { ABFT_FLIP_ANY = 0, ABFT_FLIP_VALUE = 1, ABFT_FLIP_INDEX = 2 } abft_flip_kind;

/* One queued event == one printf line of the reference backend. */
typedef enum {
  ABFT_EV_SED_DETECTED = 1,     /* "[ECC] error detected at index %d"               fatal */
  ABFT_EV_CORRECTED_BIT = 2,    /* "[ECC] corrected bit %u at index %d"                   */
  ABFT_EV_CORRECTED_PARITY = 3, /* "[ECC] corrected overall parity bit at index %d"       */
  ABFT_EV_DOUBLE_BIT = 4,       /* "[ECC] double-bit error detected"                fatal */
  ABFT_EV_ROW_SIZE = 5,         /* "row size constraint violated for ..."           fatal */
  ABFT_EV_ROW_ORDER = 6,        /* "row order constraint violated ..."              fatal */
  ABFT_EV_COL_SIZE = 7,         /* "column size constraint violated ..."            fatal */
  ABFT_EV_COL_ORDER = 8,        /* "column order constraint violated ..."           fatal */
  /* not a reference line: more COO elements carry a silently corrupted column than the
   * engine's list holds (index = its capacity); results past this point are not the
   * reference's, so the event is fatal */
  ABFT_EV_MOVED_OVERFLOW = 9,
  /* protected vectors (the abft_hip_*_vecc entries; fmt = ABFT_FMT_VECTOR): `index` is the element
   * inside the operand, `bit` holds the word bit in bits 0..7 and the operand's ordinal among the
   * entry's vector arguments, from 0, in bits 8..15 */
  ABFT_EV_VEC_CORRECTED = 10, /* "[ECC] corrected bit %u of vector operand %u at index %d"            */
  ABFT_EV_VEC_DOUBLE = 11,    /* "[ECC] double-bit error detected in vector operand %u at index %d" fatal */
  /* the protected row structure (abft_hip_matrix_create_csr_protected; fmt = ABFT_FMT_CSR): `bit` holds the
   * word bit in bits 0..7 (a row block's numbered as a COO element's 128) and the kind of word in bits 8..15
   * -- ABFT_STRUCT_ROW_EXTENT or ABFT_STRUCT_ROW_BLOCK --, `index` is the row or the block number */
  ABFT_EV_STRUCT_CORRECTED = 12, /* "[ECC] corrected bit %u of row extent %d" / "... of row block %d"              */
  ABFT_EV_STRUCT_DOUBLE = 13,    /* "[ECC] double-bit error detected in row extent %d" / "... in row block %d" fatal */
  /* the protected scalar trail (the abft_hip_*_trail_iteration_until_dev entries; fmt = ABFT_FMT_CSR): `index` is
   * the word's ordinal in its record, `bit` holds the slot's bit in bits 0..7 (numbered as a COO element's 128, the
   * parity bit 24) and the record in bits 8..15 -- ABFT_TRAIL_START, ABFT_TRAIL_PW or ABFT_TRAIL_NEXT */
  ABFT_EV_TRAIL_CORRECTED = 14, /* "[ECC] corrected bit %u of trail word %d (start record|p.w pair|next record)"        */
  ABFT_EV_TRAIL_DOUBLE = 15,    /* "[ECC] double-bit error detected in trail word %d (...)"                        fatal */
  /* matrix digests (abft_hip_matrix_verify, abft_hip_matrix_verify_dev; fmt = the matrix's): a stored array of the
   * matrix no longer has the digest it was armed with.  `index` is the segment kind (abft_hip_segment_name), `bit` 0.
   * A drain hands these over behind every other event of the same drain, and where the first fatal event of a drain
   * is one of them, all of them: one line per differing segment. */
  ABFT_EV_MATRIX_DIGEST = 16    /* "[ABFT] matrix digest mismatch in segment NAME"                                fatal */
} abft_event_kind;
#define ABFT_STRUCT_ROW_EXTENT 0
#define ABFT_STRUCT_ROW_BLOCK 1
#define ABFT_FMT_VECTOR 2 /* abft_event.fmt of the two vector events */

typedef struct {
  uint32_t kind;  /* abft_event_kind                                             */
  uint32_t index; /* element index i (or row, for the CSR row events), global    */
  uint32_t bit;   /* corrected bit for ABFT_EV_CORRECTED_BIT, else 0             */
  uint32_t fmt;   /* abft_format of the matrix that raised it (ABFT_FMT_VECTOR: a vector) */
} abft_event;

typedef struct abft_hip_ctx abft_hip_ctx;
typedef struct abft_hip_matrix abft_hip_matrix;
typedef struct abft_hip_vector abft_hip_vector;

/* ---- library / context ------------------------------------------------- */

const char *abft_hip_last_error(void);
int abft_hip_device_count(int *count);

/* Replaces `new HIPContext` (reference CGContext::create, CGContext.cpp:9-25).
 * Binds the context to `device` and creates its stream and scratch buffers.
 * abft_hip_shutdown releases everything the context owns except its stream, which is left
 * idle in a process-wide pool for the next abft_hip_init on that device (DESIGN.md section 5,
 * "a context's stream is pooled": hipStreamDestroy per context corrupted the host heap). */
int abft_hip_init(int device, abft_hip_ctx **ctx);
int abft_hip_shutdown(abft_hip_ctx *ctx);

/* Run on a caller-owned hipStream_t (e.g. torch's current stream) instead of
 * the context's own stream; NULL restores the own stream. */
int abft_hip_set_stream(abft_hip_ctx *ctx, void *hip_stream);
void *abft_hip_get_stream(abft_hip_ctx *ctx);
int abft_hip_synchronize(abft_hip_ctx *ctx);
/* The same, giving up after `seconds` (ABFT_ERR_HIP, "timed out"): for the first replay of a
 * captured graph that holds collectives, so that a stack on which they cannot run from a graph
 * ends the job with a message instead of hanging it. */
int abft_hip_synchronize_timeout(abft_hip_ctx *ctx, double seconds);

/* ---- matrix ------------------------------------------------------------ */

/* reference CSR/CPUContext.cpp:11-44 (create_matrix + generate_ecc_bits).
 * columns/rows/values are COO triplets sorted by (row, col), 0-based.
 * ECC modes need every column < 2^24 (reference CSR/CPUContext.cpp:238). */
int abft_hip_matrix_create_csr(abft_hip_ctx *ctx, int mode, const uint32_t *columns,
                               const uint32_t *rows, const double *values, int N, int nnz,
                               abft_hip_matrix **mat);
/* reference COO/CPUContext.cpp:11-36 */
int abft_hip_matrix_create_coo(abft_hip_ctx *ctx, int mode, const uint32_t *columns,
                               const uint32_t *rows, const double *values, int N, int nnz,
                               abft_hip_matrix **mat);
/* Row-block shard of a larger matrix (multi-GPU): the result vector
 * has `n_out` entries (CSR: local rows, COO: local cols, 0-based), the input
 * vector `n_in` entries (CSR: columns index it, COO: rows do); event indices
 * are reported as index_base + local element index. */
int abft_hip_matrix_create_shard(abft_hip_ctx *ctx, int format, int mode,
                                 const uint32_t *columns, const uint32_t *rows,
                                 const double *values, int n_out, int n_in, int nnz,
                                 uint32_t index_base, abft_hip_matrix **mat);
/* The same for a shard whose elements are not one contiguous run of the caller's element
 * order (COO split by column blocks: the reference's input is row-major): event indices are
 * reported as global_index[local element index] (nnz entries, ascending; NULL = as above
 * with index_base 0). */
int abft_hip_matrix_create_shard_indexed(abft_hip_ctx *ctx, int format, int mode,
                                         const uint32_t *columns, const uint32_t *rows,
                                         const double *values, int n_out, int n_in, int nnz,
                                         const uint32_t *global_index, abft_hip_matrix **mat);
/* reference CSR/CPUContext.cpp:46-52 */
int abft_hip_matrix_destroy(abft_hip_matrix *mat);
/* How the matrix is stored and run (measurement only): *layout = 0 streaming row blocks,
 * 1 column panels (chunked launches), 2 sweep (one persistent launch); *launches_per_spmv = kernel launches one abft_hip_spmv enqueues (what
 * ABFT_K_SPMV's bracket spans), without the fold of a fused product. */
int abft_hip_matrix_info(abft_hip_matrix *mat, int *layout, int *launches_per_spmv);
/* Mode none, streaming row-block CSR layout (measurement and tests only): *tiles = row blocks of the
 * layout (0 for any other layout or format), *compact_tiles = those whose columns the SpMV reads as
 * 16-bit offsets from a per-block base, *mismatches = elements of compact blocks whose base + offset
 * differs from the stored column (0 unless the copies have come apart).  Any pointer may be NULL. */
int abft_hip_matrix_compact_stats(abft_hip_matrix *mat, uint32_t *compact_tiles, uint32_t *tiles,
                                  uint32_t *mismatches);
/* Mode none, streaming row-block CSR layout (measurement and tests only): *tiles as above, *packed_tiles =
 * row blocks whose elements the SpMV reads as one 16-bit code each (column offset and value palette index),
 * *mismatches = elements of packed blocks whose decoded (column, value) differs bitwise from the stored
 * (cols, vals) (0 unless the copies have come apart).  Any pointer may be NULL. */
int abft_hip_matrix_packed_stats(abft_hip_matrix *mat, uint32_t *packed_tiles, uint32_t *tiles,
                                 uint32_t *mismatches);
/* The same layout (measurement and tests only): *packed = packed row blocks, *stage_fast = those the SpMV stages
 * without per-element bound tests (the planner has proven every code's column inside the vector and the tile's
 * window of codes inside the allocation), *row_fast = those of them whose equal-length rows (1..8 elements) it
 * also sums without row pointers or clamps.  0, 0 with ABFT_HIP_PACKED_FAST=0.  Any pointer may be NULL. */
int abft_hip_packed_stats(abft_hip_matrix *mat, uint32_t *packed, uint32_t *stage_fast, uint32_t *row_fast);

/* Read back the stored (ECC-encoded) arrays in the caller's element order.
 * CSR: cols[nnz], rowptr[nrows+1], values[nnz].  Any pointer may be NULL. */
int abft_hip_matrix_read_csr(abft_hip_matrix *mat, uint32_t *cols, uint32_t *rowptr,
                             double *values);
/* COO: 16-byte elements {col,row,value} (reference COO/ecc.h:11-16), nnz of them. */
int abft_hip_matrix_read_coo(abft_hip_matrix *mat, void *elements);

/* The stored words of ONE element by the caller's index: 3 for CSR {value low, value high, column word},
 * 4 for COO {column word, row, value low, value high} -- what inject flips bits of (a shard's host layer
 * reads the re-based index before it flips it in global terms). */
int abft_hip_matrix_read_element(abft_hip_matrix *mat, uint32_t index, uint32_t *words);

/* reference CSR/CPUContext.cpp:135-159 / COO/CPUContext.cpp:123-140, minus the
 * rand() draws: the host picks `index` and the bits (so the libc sequence stays
 * the reference's) and the device XORs them into element `index`.  Bit
 * numbering is the reference's: CSR 0-63 value, 64-95 column; COO 0-31 col,
 * 32-63 row, 64-127 value. */
int abft_hip_inject(abft_hip_matrix *mat, uint32_t index, const int *bits, int nbits);

/* XOR `mask` into row pointer `row` (0..N) of a CSR matrix: the array constraints mode checks
 * at reference CSR/CPUContext.cpp:173-182 and the reference's own injector never touches. */
int abft_hip_inject_rowptr(abft_hip_matrix *mat, uint32_t row, uint32_t mask);

/* ---- the protected row structure -----------------
 * Like abft_hip_matrix_create_csr_stream, but the matrix stores no plain row pointers and no plain
 * row-block descriptors: one 64-bit row extent word per row {code, rowptr[r], rowptr[r + 1]} under the
 * (64, 57) code of the protected vectors, and the descriptors under the 128-bit COO element code in
 * secded form -- both SECDED whatever `mode` is.  Every SpMV checks each word it reads: one flipped bit
 * is repaired, stored back and reported (ABFT_EV_STRUCT_CORRECTED), two are ABFT_EV_STRUCT_DOUBLE, fatal,
 * and the rows the word owns are not written.  Limits (ABFT_ERR_RANGE): nnz < 2^28, N <= 2^24.
 * abft_hip_spmv, _spmv_part, _spmv_dot_dev, _spmv_vecc, the residual and restart entries, cg_iteration_dev
 * and the four single guarded iterations run on such a matrix as on any other; read_csr and diag_inverse
 * strip the codes.  abft_hip_inject_rowptr, the block entries (spmm, spmm_dot, spmm_dot_vecc, both block
 * guarded iterations, block_loop_reserve) and abft_hip_spmv_dot_range_dev refuse it (ABFT_ERR_INVALID). */
int abft_hip_matrix_create_csr_protected(abft_hip_ctx *ctx, int mode, const uint32_t *columns,
                                         const uint32_t *rows, const double *values, int N, int nnz,
                                         abft_hip_matrix **mat);
/* is_protected: 0 / 1; row_words and blocks: how many words of each kind it stores (0 when not protected) */
int abft_hip_matrix_structure_info(abft_hip_matrix *mat, int *is_protected, uint32_t *row_words, uint32_t *blocks);
/* the stored codewords as they are: row_words 64-bit words, 4 * blocks 32-bit words.  Either may be NULL. */
int abft_hip_matrix_read_structure(abft_hip_matrix *mat, uint64_t *rowext, uint32_t *blk4);
/* the inverse: store the given words as they are, codewords or not (a fault injector for whole sweeps: one
 * copy instead of one abft_hip_inject_structure per word).  Either may be NULL. */
int abft_hip_matrix_write_structure(abft_hip_matrix *mat, const uint64_t *rowext, const uint32_t *blk4);
/* XOR bits into ONE stored word: kind ABFT_STRUCT_ROW_EXTENT (bits 0..63 of row `index`'s word) or
 * ABFT_STRUCT_ROW_BLOCK (bits 0..127 of descriptor `index`, numbered as a COO element's) */
int abft_hip_inject_structure(abft_hip_matrix *mat, int kind, uint32_t index, const int *bits, int nbits);
/* walk every row word and every descriptor -- those of uniform blocks too, which no SpMV reads --, repair
 * single flips in place and report like the SpMV; the counts of this call (either may be NULL) */
int abft_hip_matrix_scrub_structure(abft_hip_ctx *ctx, abft_hip_matrix *mat, uint32_t *corrected,
                                    uint32_t *uncorrectable);

/* ---- vectors ----------------------------------------------------------- */

/* reference CSR/CPUContext.cpp:54-75: contents are uninitialised */
int abft_hip_vector_create(abft_hip_ctx *ctx, int N, abft_hip_vector **vec);
/* A window [offset, offset+N) of `parent` (the local slice of a gathered
 * vector); does not own memory. */
int abft_hip_vector_view(abft_hip_vector *parent, int offset, int N, abft_hip_vector **vec);
int abft_hip_vector_destroy(abft_hip_vector *vec);
/* map: device -> pinned host staging, returns the host pointer (valid until
 * unmap); unmap: host staging -> device.  reference CSR/CPUContext.cpp:68-75 */
int abft_hip_vector_map(abft_hip_vector *vec, double **host);
int abft_hip_vector_unmap(abft_hip_vector *vec, double *host);
/* reference CSR/CPUContext.cpp:77-80: copies dst->N doubles */
int abft_hip_vector_copy(abft_hip_vector *dst, const abft_hip_vector *src);
/* The raw device address (stable for the life of the vector), for callers that
 * alias library memory, e.g. to hand it to a collective.  Work the caller
 * enqueues on it must be ordered against the context's stream.  A vector whose
 * address has been handed out is excluded from the deferred x update described
 * at abft_hip_calc_xr; ask once and keep the value. */
void *abft_hip_vector_device_ptr(abft_hip_vector *vec);
int abft_hip_vector_length(abft_hip_vector *vec);

/* ---- the CG kernels ---------------------------------------------------- */

/* reference CSR/CPUContext.cpp:82-90 */
int abft_hip_dot(abft_hip_ctx *ctx, const abft_hip_vector *a, const abft_hip_vector *b,
                 double *result);
/* reference CSR/CPUContext.cpp:92-105: x += alpha p; r -= alpha w; returns r.r.
 * The x half may be carried out by the abft_hip_calc_p that follows (it reads the
 * same p: one pass over p less per iteration); any other call on the context
 * applies it first, so callers observe exactly the reference's sequence.
 * ABFT_HIP_FUSE_X=0 turns this off. */
int abft_hip_calc_xr(abft_hip_ctx *ctx, abft_hip_vector *x, abft_hip_vector *r,
                     const abft_hip_vector *p, const abft_hip_vector *w, double alpha,
                     double *result);
/* reference CSR/CPUContext.cpp:107-113: p = r + beta p */
int abft_hip_calc_p(abft_hip_ctx *ctx, abft_hip_vector *p, const abft_hip_vector *r,
                    double beta);
/* reference CSR/CPUContext.cpp:115-133 and the five ABFT variants :162-411;
 * COO/CPUContext.cpp:104-121 and :142-379.  The mode is the matrix's.
 * On a square matrix the kernel also forms sum vec[row]*result[row]; an
 * abft_hip_dot(vec, result) issued before either vector changes is answered
 * from it (same API, one pass over the vectors less; ABFT_HIP_FUSE_DOT=0 turns
 * it off).  Large matrices with scattered columns are stored in a column-panel
 * layout chosen at create time (ABFT_HIP_LAYOUT=stream|panels|auto); element
 * indices seen by the caller (events, inject, read-back) are unaffected. */
int abft_hip_spmv(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec,
                  abft_hip_vector *result);

/* ---- block right-hand sides: K solves share one pass over the matrix ------
 * A block vector is an ordinary vector of N*K entries, row-major: entry (i, j)
 * at i*K + j (1 <= K <= 8, N*K < 2^31; with an even K it must start 16-byte
 * aligned, which every vector from abft_hip_vector_create does).  Every block
 * call takes k and checks the lengths (ABFT_ERR_INVALID on a mismatch).  Column
 * j of every result is, bit for bit, what the single call gives for column j,
 * except the reductions (dot_block, calc_xr_block's r.r), which are tree sums of
 * one shape for every column.  The block calls start like the single ones (a
 * pending x update is applied) and forget what the single calls cached (the
 * fused product, a learned iteration). */

/* CSR only: like abft_hip_matrix_create_csr, but always in the streaming
 * row-block layout (ignores ABFT_HIP_LAYOUT) -- the layout abft_hip_spmm runs on. */
int abft_hip_matrix_create_csr_stream(abft_hip_ctx *ctx, int mode, const uint32_t *columns,
                                      const uint32_t *rows, const double *values, int N, int nnz,
                                      abft_hip_matrix **mat);
/* Y = A X for k columns: the matrix is streamed, and every element ECC-checked
 * (and repaired or given up) once per call whatever k is -- one spmm queues the
 * events one spmv on the same matrix state would.  k == 1 is abft_hip_spmv.
 * Refused (ABFT_ERR_INVALID): COO matrices, CSR matrices in the panel, sweep or
 * slice layout, shards. */
int abft_hip_spmm(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *X,
                  abft_hip_vector *Y, int k);
/* out[j] = a[:, j] . b[:, j]; one synchronisation for all k */
int abft_hip_dot_block(abft_hip_ctx *ctx, const abft_hip_vector *a, const abft_hip_vector *b,
                       int k, double *out);
/* for every column j whose bit is set in `active`: x[:, j] += alpha[j] p[:, j],
 * r[:, j] -= alpha[j] w[:, j]; other columns of x and r are left untouched.
 * rr_out[j] = r[:, j] . r[:, j] for every column (active or not). */
int abft_hip_calc_xr_block(abft_hip_ctx *ctx, abft_hip_vector *x, abft_hip_vector *r,
                           const abft_hip_vector *p, const abft_hip_vector *w, int k,
                           const double *alpha, uint32_t active, double *rr_out);
/* p[:, j] = r[:, j] + beta[j] p[:, j] for the columns active in `active` */
int abft_hip_calc_p_block(abft_hip_ctx *ctx, abft_hip_vector *p, const abft_hip_vector *r, int k,
                          const double *beta, uint32_t active);

/* ---- residual checks: silent corruption of the CG vectors --------------
 * The matrix is protected element by element; x, r, p and w are not.  A
 * periodic check compares the recurrence's r with the true residual b - A x
 * (one SpMV into a scratch vector -- w is dead between calc_p and the next
 * SpMV -- and one pass over b, A x and r); a failed check lets the caller
 * restore x from a checkpoint and restart the recurrence from it.  Every entry
 * starts like the block calls (a pending x update applied, cached results
 * forgotten); the SpMV is abft_hip_spmv (abft_hip_spmm for the block forms)
 * with its events.  Sums are tree sums. */

/* XOR bits[0..nbits) (each in [0, 64)) into the double v[index]: fault injection */
int abft_hip_vector_flip(abft_hip_vector *v, int index, const int *bits, int nbits);
/* scratch = A x; out[0] = sum ((b - scratch) - r)^2, out[1] = sum (b - scratch)^2 */
int abft_hip_residual_gap(abft_hip_ctx *ctx, abft_hip_matrix *A, const abft_hip_vector *b,
                          const abft_hip_vector *x, const abft_hip_vector *r,
                          abft_hip_vector *scratch, double out[2]);
/* scratch = A x; r = b - scratch; p = r; *rr = r . r, bit for bit what abft_hip_dot(r, r)
 * returns -- from x = 0 this is the start of the CG loop (copy r <- b, copy p <- r, dot) */
int abft_hip_residual_restart(abft_hip_ctx *ctx, abft_hip_matrix *A, const abft_hip_vector *b,
                              const abft_hip_vector *x, abft_hip_vector *r, abft_hip_vector *p,
                              abft_hip_vector *scratch, double *rr);
/* block form (abft_hip_spmm's matrices): out[2j], out[2j + 1] = the two sums of column j,
 * 0.0 for a column whose bit is clear in `active` */
int abft_hip_residual_gap_block(abft_hip_ctx *ctx, abft_hip_matrix *A, const abft_hip_vector *B,
                                const abft_hip_vector *X, const abft_hip_vector *R,
                                abft_hip_vector *scratch, int k, uint32_t active, double *out);
/* block form: R and P are rewritten in the columns set in `mask` only (the others keep their
 * bits); rr[j] = R[:, j] . R[:, j] for every column, bit for bit abft_hip_dot_block(R, R) */
int abft_hip_residual_restart_block(abft_hip_ctx *ctx, abft_hip_matrix *A, const abft_hip_vector *B,
                                    const abft_hip_vector *X, abft_hip_vector *R, abft_hip_vector *P,
                                    abft_hip_vector *scratch, int k, uint32_t mask, double *rr);
/* dst[:, j] = src[:, j] for the columns set in `mask` (checkpoints of block vectors) */
int abft_hip_copy_block(abft_hip_ctx *ctx, abft_hip_vector *dst, const abft_hip_vector *src, int k,
                        uint32_t mask);

/* ---- protected vectors: a SECDED code in each double's low mantissa bits ----
 * Opt-in.  A protected element is one 64-bit word: bits 7..63 are the double's sign, exponent
 * and top 45 mantissa bits, bits 1..6 the check bits of the (64, 57) extended Hamming code
 * (check bit k at bit 1 + k, Hamming position 2^k; data bit 7, 8, ... at positions 3, 5, 6, 7,
 * 9, ...), bit 0 the overall parity.  Every *_vecc entry decodes each operand element it loads
 * -- a single flipped bit is repaired in registers and reported (ABFT_EV_VEC_CORRECTED), two are
 * fatal (ABFT_EV_VEC_DOUBLE) -- computes in full fp64 with separate multiply and add on the
 * words without their code bits, and encodes every element it stores (truncation toward zero).
 * Sums are taken over the values as stored.  Vectors a call only reads are not written back.
 * Each entry walks its vectors and folds its sum as its plain counterpart does, starts like
 * every other entry (a pending x update applied, a speculation voided) and checks every length
 * and overlap before it enqueues anything.  abft_hip_vector_copy / _map / _unmap / _flip move
 * stored words as they are: a copy of a codeword is a codeword.  The loop:
 *   encode b, x;  copy r <- b;  copy p <- r;  rr = dot_vecc(r, r)
 *   while rr > threshold:  spmv_vecc(A, p, w);  alpha = rr / dot_vecc(p, w)
 *                          rr_new = calc_xr_vecc(x, r, p, w, alpha);  calc_p_vecc(p, r, rr_new / rr)
 *   scrub x (and b) before downloading them. */

/* v[i] <- the codeword of the double v[i] (a NaN whose payload lay in bits 0..6 keeps bit 51) */
int abft_hip_vector_encode(abft_hip_ctx *ctx, abft_hip_vector *v);
/* check every word of v, write repaired words back, queue the events (operand 0); the counts of
 * repaired and of uncorrectable (left as they are) words go to *corrected / *uncorrectable */
int abft_hip_vector_scrub(abft_hip_ctx *ctx, abft_hip_vector *v, int *corrected, int *uncorrectable);
/* result = A vec on protected vectors (operands 0, 1): every gathered vec entry decoded, result
 * stored encoded.  CSR matrices in the streaming row-block layout only, all six modes; anything
 * else: ABFT_ERR_INVALID.  On a square matrix the product vec . result (decoded vec, truncated
 * result) is formed in the same pass and serves the abft_hip_dot_vecc(vec, result) that
 * follows; a plain abft_hip_dot is never served from it, nor a protected dot from abft_hip_spmv. */
int abft_hip_spmv_vecc(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec,
                       abft_hip_vector *result);
/* *out = a . b (operands 0, 1) */
int abft_hip_dot_vecc(abft_hip_ctx *ctx, const abft_hip_vector *a, const abft_hip_vector *b, double *out);
/* x += alpha p; r -= alpha w (operands 0..3); *rr = abft_hip_dot_vecc(r, r) of the r it leaves.
 * Both halves run in this call (no deferred x update).  x and r may overlap no other operand. */
int abft_hip_calc_xr_vecc(abft_hip_ctx *ctx, abft_hip_vector *x, abft_hip_vector *r, const abft_hip_vector *p,
                          const abft_hip_vector *w, double alpha, double *rr);
/* p = r + beta p (operands 0, 1); p may not overlap r */
int abft_hip_calc_p_vecc(abft_hip_ctx *ctx, abft_hip_vector *p, const abft_hip_vector *r, double beta);
/* The same two updates as two kernels that read p once (the cut abft_hip_calc_xr / _calc_p's deferred x update
 * makes on plain vectors, as calls of their own):
 *   rr_new = calc_r_vecc(r, w, alpha);  calc_px_vecc(x, p, r, alpha, rr_new / rr)
 * For the same alpha and beta x, r and *rr are bit for bit what abft_hip_calc_xr_vecc leaves and returns and p what
 * abft_hip_calc_p_vecc leaves, where both walk alike: each call chooses its walk (pairs or single elements) by the
 * 16-byte alignment of ITS operands, so vectors that are all whole, or all views at an odd offset, always agree.
 * Both start like abft_hip_calc_xr_vecc (the prologue, the learned iteration and the fused product forgotten) and
 * check every length and overlap before anything is enqueued.
 * r -= alpha w (operands 0: r, 1: w; w is not written back); *rr = abft_hip_dot_vecc(r, r) of the r it leaves */
int abft_hip_calc_r_vecc(abft_hip_ctx *ctx, abft_hip_vector *r, const abft_hip_vector *w, double alpha, double *rr);
/* x += alpha p; p = r + beta p, both from the p the call finds (operands 0: x, 1: p, 2: r; r is not written back).
 * No two of x, p, r may overlap. */
int abft_hip_calc_px_vecc(abft_hip_ctx *ctx, abft_hip_vector *x, abft_hip_vector *p, const abft_hip_vector *r,
                          double alpha, double beta);

/* ---- Jacobi (diagonal) preconditioning ------------------------------------
 * M^-1 = diag(dinv) is one more N-vector; z = dinv * r is one rounded product formed
 * inside the kernels that already stream r and never stored.  The loop:
 *   copy r <- b;  {rz, rr} = precond_start(r, dinv, p)
 *   while rr > threshold:  spmv(A, p, w);  alpha = rz / dot(p, w)
 *                          {rz_new, rr} = calc_xr_precond(x, r, p, w, dinv, alpha)
 *                          calc_p_precond(p, r, dinv, rz_new / rz);  rz = rz_new
 * Every multiply and add is separate.  Each entry walks the vectors and folds its sums
 * exactly as its plain counterpart (dot, calc_xr, calc_p and their block forms), so with
 * dinv == 1.0 everywhere it leaves and returns the plain call's bits.  Every length is
 * checked, and a dinv that overlaps a vector the call writes is refused
 * (ABFT_ERR_INVALID) before anything is enqueued.  In these entries dinv carries no ECC
 * words: damage to it changes M, hence the rate of convergence, never the consistency of r
 * with b - A x that the residual checks verify (the protected forms below keep dinv under
 * the vectors' code). */

/* dinv[i] = 1.0 / d[i], d[i] = the sum, in the caller's element order, of the values of the
 * elements whose row and column are both i (the column as that mode's SpMV decodes it: ECC
 * bits masked off; no ECC check, no repair, no event -- the SpMV checks the matrix).  A row
 * with no diagonal element, or whose d[i] is not finite or <= 0, gets 1.0 and is counted in
 * *bad.  CSR and COO, every one-GPU layout (a device kernel over the stored arrays for the
 * streaming CSR and the grouped COO layout -- there a COO element whose stored column no
 * longer names the group it is stored in is not on any diagonal --, the caller-order read-back
 * for the permuted layouts); shards: ABFT_ERR_INVALID. */
int abft_hip_matrix_diag_inverse(abft_hip_ctx *ctx, abft_hip_matrix *mat, abft_hip_vector *dinv,
                                 uint32_t *bad);
/* p = z; out = {sum r z, sum r r}; out[1] is abft_hip_dot(r, r) bit for bit */
int abft_hip_precond_start(abft_hip_ctx *ctx, const abft_hip_vector *r, const abft_hip_vector *dinv,
                           abft_hip_vector *p, double out[2]);
/* x += alpha p; r -= alpha w; out = {sum r z, sum r r} of the new r.  The x half may be
 * carried out by the abft_hip_calc_p_precond that follows, under abft_hip_calc_xr's rules
 * (any other call applies it first; ABFT_HIP_FUSE_X=0 turns it off). */
int abft_hip_calc_xr_precond(abft_hip_ctx *ctx, abft_hip_vector *x, abft_hip_vector *r,
                             const abft_hip_vector *p, const abft_hip_vector *w,
                             const abft_hip_vector *dinv, double alpha, double out[2]);
/* p = z + beta p, z formed again from the same operands (the same bits) */
int abft_hip_calc_p_precond(abft_hip_ctx *ctx, abft_hip_vector *p, const abft_hip_vector *r,
                            const abft_hip_vector *dinv, double beta);
/* The same preconditioning on PROTECTED vectors (the *_vecc entries above): r, p, x, w AND dinv hold codewords
 * (abft_hip_vector_encode dinv once).  val(w): the repaired word without its 7 code bits; enc(v): v truncated toward
 * zero plus the code bits; z = val(dinv[i]) * (value of r[i]) is one rounded fp64 product, never stored and never
 * truncated; every multiply and add is separate; sums are over the values as stored.  The loop:
 *   copy r <- b;  {rz, rr} = precond_start_vecc(r, dinv, p)
 *   while rr > threshold:  spmv_vecc(A, p, w);  alpha = rz / dot_vecc(p, w)
 *                          {rz_new, rr} = calc_r_precond_vecc(r, w, dinv, alpha)
 *                          calc_px_precond_vecc(x, p, r, dinv, alpha, rz_new / rz);  rz = rz_new
 * -- the r / px cut of abft_hip_calc_r_vecc / _calc_px_vecc: one set of walks, 80 N bytes of vectors behind the SpMV.
 * Each walks and sums as its plain protected counterpart (abft_hip_dot_vecc for the start), pairs only when ALL its
 * operands, dinv included, are 16-byte aligned, the two sums through the K-wide slot as abft_hip_precond_start's.
 * With dinv == enc(1.0) everywhere, on whole vectors: calc_r_precond_vecc leaves abft_hip_calc_r_vecc's r and returns
 * its r.r in out[1], out[0] the same bits; calc_px_precond_vecc leaves abft_hip_calc_px_vecc's x and p;
 * precond_start_vecc leaves a copy of r in p.
 * A flipped bit in any operand is repaired in registers and reported (ABFT_EV_VEC_CORRECTED, the operand's ordinal
 * as listed); a vector a call only reads is not written back -- EXCEPT dinv, which no call of the loop ever rewrites:
 * the repaired dinv word is stored back, so a flip in dinv is reported once and gone afterwards.  Two flips in one
 * word are ABFT_EV_VEC_DOUBLE, fatal, the word left as it is.  Hence dinv is not const here.
 * Each starts like abft_hip_calc_r_vecc (the prologue, the learned iteration and the fused product forgotten) and
 * refuses (ABFT_ERR_INVALID) a null pointer, differing lengths and ANY two operands that overlap, dinv included, before
 * anything is enqueued, every operand untouched.
 * p = enc(z), z from val(r) (operands 0: r, 1: dinv, 2: p; p is only written, r not written back);
 * out = {sum val(r) z, sum val(r) val(r)}; out[1] is abft_hip_dot_vecc(r, r) bit for bit */
int abft_hip_precond_start_vecc(abft_hip_ctx *ctx, const abft_hip_vector *r, abft_hip_vector *dinv,
                                abft_hip_vector *p, double out[2]);
/* r = enc(val(r) - alpha val(w)) (operands 0: r, 1: w, 2: dinv; w is not written back);
 * out = {sum r' z', sum r' r'}, r' the stored r without its code bits, z' = val(dinv) r' */
int abft_hip_calc_r_precond_vecc(abft_hip_ctx *ctx, abft_hip_vector *r, const abft_hip_vector *w,
                                 abft_hip_vector *dinv, double alpha, double out[2]);
/* x = enc(val(x) + alpha val(p)); p = enc(val(dinv) val(r) + beta val(p)), both from the p the call finds, read once
 * (operands 0: x, 1: p, 2: r, 3: dinv; r is not written back) */
int abft_hip_calc_px_precond_vecc(abft_hip_ctx *ctx, abft_hip_vector *x, abft_hip_vector *p,
                                  const abft_hip_vector *r, abft_hip_vector *dinv, double alpha, double beta);
/* Block forms (k <= 8 columns, row-major as above; ONE dinv of N entries for all columns: one
 * operator).  out[2j], out[2j + 1] = column j's two sums, for every column.  P is rewritten in
 * the columns set in `mask` only; `active` as in abft_hip_calc_xr_block / _calc_p_block: a
 * column whose bit is clear keeps its bits. */
int abft_hip_precond_start_block(abft_hip_ctx *ctx, const abft_hip_vector *R, const abft_hip_vector *dinv,
                                 abft_hip_vector *P, int k, uint32_t mask, double *out);
int abft_hip_calc_xr_precond_block(abft_hip_ctx *ctx, abft_hip_vector *X, abft_hip_vector *R,
                                   const abft_hip_vector *P, const abft_hip_vector *W,
                                   const abft_hip_vector *dinv, int k, const double *alpha, uint32_t active,
                                   double *out);
int abft_hip_calc_p_precond_block(abft_hip_ctx *ctx, abft_hip_vector *P, const abft_hip_vector *R,
                                  const abft_hip_vector *dinv, int k, const double *beta, uint32_t active);

/* ---- the fused block iteration ------------------------------------------
 * The block CG loop in three calls instead of four, 64 N k bytes of vectors behind the SpMM
 * instead of 88 N k.  Nothing is carried between calls: every sum comes back through the call
 * that forms it.  Each entry starts like the other block calls, checks every length, k and
 * overlap before anything is queued, and leaves every operand untouched when it refuses. */

/* W = A P as abft_hip_spmm (k in [1, 8]; the same bits, the same events), and
 * out[j] = P[:, j] . W[:, j], formed from W's rows while they are in registers: per row block
 * a tree sum of one shape, the row blocks' partials folded in a fixed order (so two calls give
 * the same bits, and a column scaled by a power of two gives the scaled sum).  Refused: what
 * abft_hip_spmm refuses, and a matrix that is not square. */
int abft_hip_spmm_dot(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *P,
                      abft_hip_vector *W, int k, double *out);
/* the r half of abft_hip_calc_xr_block: r[:, j] -= alpha[j] w[:, j] for the active columns;
 * rr_out[j] = r[:, j] . r[:, j] for every column.  R and the sums are, bit for bit, those of
 * abft_hip_calc_xr_block with the same alpha and mask. */
int abft_hip_calc_r_block(abft_hip_ctx *ctx, abft_hip_vector *R, const abft_hip_vector *W, int k,
                          const double *alpha, uint32_t active, double *rr_out);
/* for the active columns x[:, j] += alpha[j] p[:, j], then p[:, j] = r[:, j] + beta[j] p[:, j],
 * p read once: the bits the x half of abft_hip_calc_xr_block and abft_hip_calc_p_block give */
int abft_hip_calc_px_block(abft_hip_ctx *ctx, abft_hip_vector *X, abft_hip_vector *P,
                           const abft_hip_vector *R, int k, const double *alpha, const double *beta,
                           uint32_t active);
/* the Jacobi forms (one dinv of N entries): out[2j], out[2j + 1] = column j's r.z and r.r, as
 * abft_hip_calc_xr_precond_block; p[:, j] = dinv * r[:, j] + beta[j] p[:, j] */
int abft_hip_calc_r_precond_block(abft_hip_ctx *ctx, abft_hip_vector *R, const abft_hip_vector *W,
                                  const abft_hip_vector *dinv, int k, const double *alpha, uint32_t active,
                                  double *out);
int abft_hip_calc_px_precond_block(abft_hip_ctx *ctx, abft_hip_vector *X, abft_hip_vector *P,
                                   const abft_hip_vector *R, const abft_hip_vector *dinv, int k,
                                   const double *alpha, const double *beta, uint32_t active);

/* The fused block iteration on PROTECTED block vectors: every double of the N x k
 * blocks is a (64, 57) codeword, as in the abft_hip_*_vecc entries above; abft_hip_vector_encode, _scrub,
 * _flip and _copy treat a block as N * k words (a scrub's event index is row * k + column).  Each entry is
 * its plain twin on codewords -- same checks and refusals, same grid, walk and reductions -- that decodes
 * every word it loads (inactive columns included), computes with the values in full fp64 and encodes every
 * word it stores.  A word with one flipped bit is repaired in registers and reported once
 * (ABFT_EV_VEC_CORRECTED, index row * k + column, bit | operand << 8); two flipped bits are
 * ABFT_EV_VEC_DOUBLE (fatal).  With the same scalars and mask, column j of every vector is word for word
 * what abft_hip_spmv_vecc, abft_hip_calc_r_vecc and abft_hip_calc_px_vecc leave for column j alone.
 * A column whose bit is clear in `active` is never computed with; in a vector the call writes its words are
 * stored back repaired (a clean word keeps every bit).
 *
 * W = enc(A val(P)), out[j] = sum over rows of val(P[row, j]) * strip(stored W[row, j]); P is operand 0 and is
 * not written back.  Matrix elements are checked as in abft_hip_spmm_dot. */
int abft_hip_spmm_dot_vecc(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *P,
                           abft_hip_vector *W, int k, double *out);
/* out[j] = sum val(a[:, j]) * val(b[:, j]) (operands 0: a, 1: b; nothing is written) */
int abft_hip_dot_block_vecc(abft_hip_ctx *ctx, const abft_hip_vector *a, const abft_hip_vector *b, int k,
                            double *out);
/* R[:, j] = enc(val(R[:, j]) - alpha[j] val(W[:, j])) in the active columns; rr_out[j] = the sum of the squares
 * of the stored R's values for EVERY column: the bits abft_hip_dot_block_vecc(R, R) then gives (operands 0: R,
 * 1: W; W is not written back) */
int abft_hip_calc_r_block_vecc(abft_hip_ctx *ctx, abft_hip_vector *R, const abft_hip_vector *W, int k,
                               const double *alpha, uint32_t active, double *rr_out);
/* in the active columns X[:, j] = enc(val(X) + alpha[j] val(P)) and P[:, j] = enc(val(R) + beta[j] val(P)), both
 * from the P the call finds (operands 0: X, 1: P, 2: R; R is not written back) */
int abft_hip_calc_px_block_vecc(abft_hip_ctx *ctx, abft_hip_vector *X, abft_hip_vector *P,
                                const abft_hip_vector *R, int k, const double *alpha, const double *beta,
                                uint32_t active);

/* Shard-local forms for the row-partitioned solver: same kernels, but the
 * result stays on the device so a collective can sum it across ranks before
 * the host reads it.  `dev_result` is a device pointer to TWO doubles:
 * [0] = the shard's partial sum, [1] = this context's queued-event count
 * (so one all-reduce also tells every rank whether any rank has events). */
int abft_hip_dot_dev(abft_hip_ctx *ctx, const abft_hip_vector *a, const abft_hip_vector *b,
                     double *dev_result);
int abft_hip_calc_xr_dev(abft_hip_ctx *ctx, abft_hip_vector *x, abft_hip_vector *r,
                         const abft_hip_vector *p, const abft_hip_vector *w, double alpha,
                         double *dev_result);
/* ... and back: the two doubles at `dev_pair` (after the collective summed them on
 * the context's stream) delivered to the host through the pinned slot it polls. */
int abft_hip_read_pair(abft_hip_ctx *ctx, const double *dev_pair, double *value, double *events);
/* ... and the other way (a sum formed on the host, e.g. by host-staged collectives). */
int abft_hip_write_pair(abft_hip_ctx *ctx, double *dev_pair, double value, double events);

/* All-reduce of such a pair across the processes of ONE node without a collective
 * library (no counterpart in the reference, which is single-process; SURVEY 8e names the
 * two scalar all-reduces per iteration).  `shared` is a page-aligned region of at least
 * abft_hip_peer_board_bytes() that every process of the job has mapped (POSIX shared
 * memory, zero-filled when created); attach registers it with the GPU.  The all-reduce is
 * one small kernel on the context's stream -- capturable -- in which each rank publishes
 * its pair on the board and adds all ranks' pairs in rank order (identical bits everywhere).
 * Every rank must enqueue the same sequence of all-reduces.  A rank that waits longer than
 * `timeout_seconds` (<= 0: 120) for a peer leaves NaN and abft_hip_peer_board_failed() = 1. */
size_t abft_hip_peer_board_bytes(void);
int abft_hip_peer_board_attach(abft_hip_ctx *ctx, void *shared, size_t bytes, int rank, int size,
                               double timeout_seconds);
int abft_hip_peer_board_detach(abft_hip_ctx *ctx);
int abft_hip_allreduce_pair_peers(abft_hip_ctx *ctx, double *dev_pair);
/* on != 0: every device-scalar reduction of the context from now on (abft_hip_dot_dev,
 * abft_hip_calc_xr_dev, abft_hip_calc_xr_ratio_dev, the product of abft_hip_spmv_dot_*_dev)
 * delivers its pair already summed over the ranks: the all-reduce runs in the tail of the
 * block that finishes the shard's sum, no kernel of its own.  All ranks switch together. */
int abft_hip_peer_board_fuse(abft_hip_ctx *ctx, int on);
int abft_hip_peer_board_failed(abft_hip_ctx *ctx);
/* The same board in DEVICE memory, one copy per rank: a rank pushes its slot into every copy (stores over
 * xGMI between the GPUs of a node) and polls only its own -- no host memory, no PCIe crossing.  Across
 * processes: every rank calls _ipc_export (allocates its copy, hands out an IPC handle of
 * abft_hip_peer_board_ipc_handle_bytes() bytes), the handles are gathered by the caller's own means, then
 * _ipc_attach maps the peers' copies (fails, leaving nothing attached, when a peer's memory cannot be reached:
 * the caller then falls back to the host-memory board above).  Inside one process (two contexts standing in
 * for two ranks): _device_alloc per rank + _attach_device with the plain pointers.  Everything else --
 * abft_hip_allreduce_pair_peers, _fuse, _failed, _detach, identical bits on every rank -- as above. */
size_t abft_hip_peer_board_ipc_handle_bytes(void);
int abft_hip_peer_board_ipc_export(abft_hip_ctx *ctx, void *handle);
int abft_hip_peer_board_ipc_attach(abft_hip_ctx *ctx, const void *handles, int rank, int size, double timeout_seconds);
int abft_hip_peer_board_device_alloc(abft_hip_ctx *ctx, void **board);
int abft_hip_peer_board_device_free(abft_hip_ctx *ctx, void *board);
int abft_hip_peer_board_attach_device(abft_hip_ctx *ctx, void *const *boards, int rank, int size, double timeout_seconds);

/* The windows of the gathered vector that a rank's peers read (the halo of a banded matrix)
 * exchanged between the processes of ONE node through shared host memory, in one capturable
 * kernel on the context's stream ("a neighbour exchange would beat an all-gather"
 * for banded matrices).  `shared`: a page-aligned, zero-filled region of at least
 * abft_hip_peer_exchange_bytes(size, outbox_bytes) mapped by every process; every rank lays
 * the windows it sends out in its outbox (`box_offset`, 8-byte aligned, the same
 * outbox_bytes on every rank; behind each window 8 more bytes belong to the library: a
 * check word) and lists the windows it receives with the offsets their senders chose.
 * `vector_offset` / `count` are in doubles from the start of the gathered vector passed to
 * abft_hip_peer_exchange.  Every rank must enqueue the same sequence of
 * exchanges.  Give-up after `timeout_seconds` (<= 0: 120): NaN in the first received window
 * and abft_hip_peer_exchange_failed() = 1. */
typedef struct {
  int peer;                 /* out: the rank that reads it; in: the rank that sends it */
  uint32_t vector_offset;   /* doubles */
  uint32_t count;           /* doubles */
  uint64_t box_offset;      /* bytes from the start of the SENDER's outbox */
} abft_peer_piece;
size_t abft_hip_peer_exchange_bytes(int size, size_t outbox_bytes);
int abft_hip_peer_exchange_attach(abft_hip_ctx *ctx, void *shared, size_t bytes, int rank, int size,
                                  size_t outbox_bytes, const abft_peer_piece *out, int nout,
                                  const abft_peer_piece *in, int nin, double timeout_seconds);
int abft_hip_peer_exchange_detach(abft_hip_ctx *ctx);
int abft_hip_peer_exchange(abft_hip_ctx *ctx, abft_hip_vector *full);
/* ... or, with beside != 0, on a side stream behind everything enqueued so far: what the caller
 * enqueues on the context's stream until _finish runs next to the exchange (an SpMV's rows that
 * read no window: abft_hip_spmv_dot_part_dev, ABFT_PART_INTERIOR); _finish makes the context's
 * stream wait for it.  (Two stream hand-offs, also when replayed from a graph: worth it only
 * for exchanges longer than those; the C++ host leaves it off) */
int abft_hip_peer_exchange_begin(abft_hip_ctx *ctx, abft_hip_vector *full, int beside);
int abft_hip_peer_exchange_finish(abft_hip_ctx *ctx);
int abft_hip_peer_exchange_failed(abft_hip_ctx *ctx);
/* The same exchange through DEVICE memory (round 3): every rank owns a region of
 * abft_hip_peer_exchange_bytes(size, outbox_bytes) in its GPU's memory, laid out like the shared one, and a rank
 * PUSHES each window -- and its sequence words -- into the reader's region (stores over xGMI between the GPUs of
 * a node); all waiting and reading is on the rank's own memory.  Across processes: _ipc_export (allocates the
 * region, hands out an IPC handle of abft_hip_peer_board_ipc_handle_bytes() bytes), the handles gathered by the
 * caller's own means, _ipc_attach (fails, leaving nothing attached, when a peer's region cannot be mapped).
 * Inside one process: _device_alloc per rank + _attach_device with the plain pointers.  Window lists, outbox
 * layout, abft_hip_peer_exchange[_begin/_finish], _failed, _detach: as above. */
int abft_hip_peer_exchange_ipc_export(abft_hip_ctx *ctx, int size, size_t outbox_bytes, void *handle);
int abft_hip_peer_exchange_ipc_attach(abft_hip_ctx *ctx, const void *handles, int rank, int size, size_t outbox_bytes,
                                      const abft_peer_piece *out, int nout, const abft_peer_piece *in, int nin,
                                      double timeout_seconds);
int abft_hip_peer_exchange_device_alloc(abft_hip_ctx *ctx, int size, size_t outbox_bytes, void **region);
int abft_hip_peer_exchange_device_free(abft_hip_ctx *ctx, void *region);
int abft_hip_peer_exchange_attach_device(abft_hip_ctx *ctx, void *const *regions, int rank, int size, size_t outbox_bytes,
                                         const abft_peer_piece *out, int nout, const abft_peer_piece *in, int nin,
                                         double timeout_seconds);

/* Device-scalar forms, for loops that keep alpha and beta on the device (no host
 * round trip per iteration; the row-partitioned solver's fixed-iteration loop):
 *   spmv_dot_dev        result = A vec, and dev_result = {sum_row vec[vec_offset+row]
 *                       * result[row], queued events}  (vec_offset: the shard's slot
 *                       in the gathered vector; 0 on one GPU)
 *   calc_xr_ratio_dev   calc_xr with alpha = *dev_num / *dev_den  (cg.cpp:102)
 *   calc_p_ratio_dev    calc_p  with beta  = *dev_num / *dev_den  (cg.cpp:109)
 * All three are asynchronous; every pointer is device memory.
 * calc_xr_ratio_dev's r.r (like calc_xr's, and abft_hip_cg_iteration_dev's) is summed in the order of
 * the call's walk: by pairs of entries when x, r, p and w are ALL 16-byte aligned, entry by entry when
 * any of them is not (a view at an odd offset) -- whichever kernels run the call.  It therefore equals
 * abft_hip_dot(r, r) on the resulting r bit for bit when r's alignment matches the call's (all four
 * aligned, or r itself unaligned); with r aligned beside an unaligned x, p or w, abft_hip_dot(r, r)
 * adds the same products in the other order. */
int abft_hip_spmv_dot_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec,
                          abft_hip_vector *result, int vec_offset, double *dev_result);
int abft_hip_calc_xr_ratio_dev(abft_hip_ctx *ctx, abft_hip_vector *x, abft_hip_vector *r,
                               const abft_hip_vector *p, const abft_hip_vector *w,
                               const double *dev_num, const double *dev_den, double *dev_result);
int abft_hip_calc_p_ratio_dev(abft_hip_ctx *ctx, abft_hip_vector *p, const abft_hip_vector *r,
                              const double *dev_num, const double *dev_den);

/* SpMV in two parts, so a shard can multiply the rows that need nothing from its
 * peers while the exchange of the input vector is still in flight.
 * abft_hip_matrix_set_interior declares rows [row_lo, row_hi) of the matrix
 * "interior": every input entry they read is in place before the exchange.  Then
 *   part = ABFT_PART_INTERIOR   multiplies (whole row blocks of) those rows only,
 *   part = ABFT_PART_BOUNDARY   all the others, and completes the fused product;
 * issued in that order on unchanged vectors, the two calls together equal one
 * ABFT_PART_ALL call bit for bit, events included.  Row sums are never split
 * (an output's additions keep the reference's order), so this is a split by
 * rows, not by columns.  Layouts without row-block launches (panels, COO) keep
 * the interior part empty: INTERIOR returns at once and BOUNDARY does the work. */
typedef enum { ABFT_PART_ALL = 0, ABFT_PART_INTERIOR = 1, ABFT_PART_BOUNDARY = 2 } abft_part;
int abft_hip_matrix_set_interior(abft_hip_matrix *mat, int row_lo, int row_hi);
int abft_hip_spmv_part(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec,
                       abft_hip_vector *result, int part);
int abft_hip_spmv_dot_part_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec,
                               abft_hip_vector *result, int vec_offset, double *dev_result, int part);

/* SpMV by ranges of column panels, for a shard whose input vector arrives slot by slot (an
 * exchange pipelined with the multiplication).  A matrix in the sweep layout is stored in
 * *npanels panels of *width input entries each (abft_hip_matrix_panels; any other layout:
 * one panel) and its rows are summed panel by panel in ascending order, so
 *   spmv_dot_range_dev(.., 0, k), spmv_dot_range_dev(.., k, npanels)
 * on unchanged vectors equal one abft_hip_spmv_dot_dev bit for bit: the first range starts
 * the row sums, a later one continues from what `result` holds, the one that ends at
 * npanels completes the fused product in dev_result (NULL: plain SpMV).  Panels [c0, c1)
 * read input entries [c0 * width, c1 * width) only. */
int abft_hip_matrix_panels(abft_hip_matrix *mat, int *npanels, int *width);
int abft_hip_spmv_dot_range_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec,
                                abft_hip_vector *result, int vec_offset, double *dev_result, int c0, int c1);

/* Speculation (round 4, opt-in: ABFT_HIP_SPECULATE=1; cross-call fusion behind the unchanged host-scalar API,
 * reference loop cg.cpp:97-112): once the library has seen one iteration of the CG loop -- spmv(A,p,w), [dot(p,w)],
 * calc_xr(x,r,p,w,alpha), calc_p(p,r,beta) on vectors it alone can see -- it enqueues, right behind the next
 * spmv(A,p,w), that iteration's r half with alpha = r.r / p.w formed on the device, into a shadow buffer; a calc_xr
 * that arrives with the same vectors and a bit-identical alpha takes it over (r's buffer and the shadow are swapped, no
 * launch, the GPU did not wait for the scalar's round trip) and at once enqueues the x / p half (x in place -- it is
 * due --, p with beta = r.r_new / r.r into a shadow), which calc_p takes over likewise; anything else drops the
 * shadows and runs the call as written.  A view made of r or p while a half is in flight (abft_hip_vector_view drops
 * nothing itself) makes the call that would have swapped that vector's buffer drop the half instead: no buffer changes
 * places behind a view.  The results are the same bits either way.  This reports how often a speculated iteration was
 * taken over / dropped. */
int abft_hip_speculation_stats(abft_hip_ctx *ctx, long *taken, long *dropped);

/* `processes` processes drive this library on the context's device at the same time (ranks sharing one GPU:
 * tests).  Launches whose workgroups wait for each other inside the kernel (abft_hip_cg_iteration_dev's one-launch
 * tail) then size their grids for that share of the device, so that every process's workgroups are resident
 * together.  Default 1: one process per GPU. */
int abft_hip_set_sharers(abft_hip_ctx *ctx, int processes);

/* One CG iteration behind its exchange, scalars on the device (reference loop cg.cpp:97-112):
 *   w = A vec [part: ABFT_PART_ALL, or ABFT_PART_BOUNDARY after an ABFT_PART_INTERIOR call],
 *   dev_pw = {vec[vec_offset..] . w, events};  alpha = dev_rr[0] / dev_pw[0];
 *   r -= alpha w;  dev_rr_new = {r . r, events};  beta = dev_rr_new[0] / dev_rr[0];
 *   x += alpha p;  p = r + beta p.
 * Bit for bit what abft_hip_spmv_dot_part_dev + abft_hip_calc_xr_ratio_dev + abft_hip_calc_p_ratio_dev
 * leave behind (with abft_hip_peer_board_fuse the two scalars arrive summed over the ranks, as there),
 * but everything behind the SpMV -- the fold of the fused product, the r half, the x / p half and the
 * two board all-reduces -- is ONE launch of co-resident workgroups where that applies (vectors of at most
 * 2^22 entries -- beyond that the three kernels are faster --, x private to the library and no operand
 * aliasing another; ABFT_HIP_TAIL=0 keeps the three kernels).  p is the
 * caller's view of vec's slot (the vector the SpMV read).  Enqueue-only: capturable.
 * The order in which r.r is summed: see abft_hip_calc_xr_ratio_dev above.
 * abft_hip_tail_stats tells which form a call took.  x, r, p or w missing or of different lengths:
 * ABFT_ERR_INVALID before anything is launched (w and dev_pw keep what they held). */
int abft_hip_cg_iteration_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec, int vec_offset,
                              int part, abft_hip_vector *x, abft_hip_vector *r, abft_hip_vector *p,
                              abft_hip_vector *w, const double *dev_rr, double *dev_pw, double *dev_rr_new);
/* What the last abft_hip_cg_iteration_dev on the context ran behind its SpMV (tests; host counters, nothing
 * on the device): *path = 0 the three kernels, 1 the one launch in its form for operands that are not all
 * 16-byte aligned (cg_tail_kernel<1, false>), 2 the aligned form that walks the vector in rounds (<2, false>),
 * 3 the register-resident form (<2, true>); *grid = the workgroups launched and *want = the number the
 * vector's length asks for before the resident cap (both 0 on path 0); counts[k] = calls that took path k
 * since the context was created.  Any pointer may be null. */
int abft_hip_tail_stats(abft_hip_ctx *ctx, int *path, int *grid, int *want, long counts[4]);

/* The x update inside the next SpMV (host-scalar loop; DESIGN.md section 4, "Fourth cross-call fusion").  Once
 * abft_hip_spmv(A, p, w) has been seen directly behind an abft_hip_calc_p(p, r, beta) that took the x += alpha p of
 * the preceding abft_hip_calc_xr along, the following abft_hip_calc_p writes the new p into a buffer of the
 * context's, swaps it with p's and leaves x += alpha p_old pending; the abft_hip_spmv(A, p, w) that follows -- a
 * CSR matrix in the streaming layout, with the fused product -- applies it row by row, and any other call applies
 * it first, as a kernel of its own.  Every x, r, p, w, scalar and event keeps its bits; only when x[i] is written
 * changes.  p must be a whole vector whose device pointer was never handed out and that has no views.
 * By default the prediction is armed on matrices of mode ABFT_MODE_NONE only (the one mode it was measured to pay on);
 * ABFT_HIP_X_IN_SPMV=1 (read when the context is created) arms it in every mode, =0 in none; it is also off with
 * ABFT_HIP_FUSE_X=0, ABFT_HIP_FUSE_DOT=0 or ABFT_HIP_SPECULATE=1, and from the context's first
 * abft_hip_graph_begin on.  *absorbed = pending updates taken over by the predicted SpMV -- applied by that launch
 * or, with ABFT_HIP_LAZY_X above 1, queued by it for a later one -- *flushed = pending updates applied on their own
 * before their SpMV came, since the context was created (host counters; either pointer may be null). */
int abft_hip_x_in_spmv_stats(abft_hip_ctx *ctx, long *absorbed, long *flushed);

/* The queue of x updates ("Sixth cross-call fusion"; ABFT_HIP_LAZY_X=1|2|4, read when the context
 * is created; 1 wherever the x update inside the next SpMV is off).  Nobody reads x before the solve ends or the
 * caller looks at it, so with depth d > 1 the predicted SpMV only queues the update it takes over, and every d-th one
 * applies d of them in one pass: x read and written once, the d multiply-adds per element in arrival order -- the
 * same bits.  The loop's own calls keep the queue (that abft_hip_spmv(A, p, w), the abft_hip_dot(p, w) served from its
 * fused product, the abft_hip_calc_xr on the same x and the abft_hip_calc_p behind it); every other call applies it
 * first, in order, with one kernel.  The context holds d buffers of p's length for it (d + 1 with the one behind p's
 * handle); where they do not fit, the depth falls to 2 or 1.  *bursts = SpMV launches that applied d updates,
 * *applied_in_bursts = updates those applied, *applied_by_flush = queued updates applied on their own, since the
 * context was created (host counters; any pointer may be null). */
int abft_hip_lazy_x_stats(abft_hip_ctx *ctx, long *bursts, long *applied_in_bursts, long *applied_by_flush);

/* Run-ahead of the host-scalar loop ("Fifth cross-call fusion"; ABFT_HIP_AHEAD=0|1|2, read when
 * the context is created).  The loop hands two scalars to the host per iteration, and the GPU runs nothing while the
 * host forms alpha and beta from them.  Level 1: abft_hip_calc_xr launches, behind its own kernel and before it waits
 * for r.r, the p = r + beta p of the abft_hip_calc_p that will follow, with beta = r.r_new / r.r formed on the device,
 * into the buffer the x-in-SpMV path swaps p's with.  Level 2: abft_hip_spmv also launches, behind its fold, the
 * r -= alpha w of the coming abft_hip_calc_xr with alpha = r.r / p.w formed on the device, into a buffer of the
 * context's, and the level-1 kernel behind that.  The call that arrives with the same vectors and an alpha (beta) that
 * is bit for bit the quotient of the scalars handed back -- and no NaN -- commits: the buffers change places and no
 * kernel is launched.  Any other call drops what was launched, unread, and runs as written; the results are the same
 * bits either way.  Armed by one complete iteration (abft_hip_spmv, abft_hip_dot(p, w), abft_hip_calc_xr,
 * abft_hip_calc_p, nothing in between) on whole vectors that were never exposed and have no views, run as written,
 * whose alpha and beta were the two quotients; a drop, or an iteration with other scalars, disarms until the next such
 * iteration.  Only where the x-in-SpMV path is armed (above), and off with ABFT_HIP_SPECULATE=1.
 * Default: level 1 (the level that was measured to pay; level 2 did not beat it: DESIGN.md section 4); ABFT_HIP_AHEAD=0 turns it off.
 * ABFT_HIP_DEFER_FINISH=0|1 (read when the context is created; default 1; no effect where the run-ahead is off): a
 * reduction whose consumer kernel is launched behind it in the same call -- the r -= alpha w in front of the level-1
 * kernel, at level 2 also the multi-workgroup fold of p.w in front of that -- ends with its block partials, and every
 * workgroup of the consumer folds them at its head, in the order the reduction's own last workgroup would have; its
 * first workgroup publishes the scalar.  The same bits, the same counters, one serial tail less per hand-off.
 * *committed_p / *committed_r = calls of abft_hip_calc_p / abft_hip_calc_xr that took over a kernel run ahead,
 * *dropped = run-aheads thrown away, since the context was created (host counters; any pointer may be null). */
int abft_hip_ahead_stats(abft_hip_ctx *ctx, long *committed_p, long *committed_r, long *dropped);

/* The guarded iteration: abft_hip_cg_iteration_dev behind the stop test of the reference loop (cg.cpp:94,
 * `while (rr > conv)`), evaluated ON THE DEVICE, so that a loop with a convergence threshold can enqueue
 * (or replay from a graph) several iterations and look at the scalars once per batch: iterations enqueued
 * past convergence do nothing.
 *   LIVE   when dev_rr[0] > threshold (false for NaN, as the reference's test is): bit for bit what
 *          abft_hip_cg_iteration_dev leaves for the same arguments -- x, r, p, w, both pairs, the events words.
 *   FROZEN otherwise: x, r and p keep every bit; dev_rr_new[0] gets the bits of dev_rr[0] (so the next guarded
 *          iteration, reading that pair, is frozen too) and dev_rr_new[1] the queued-event count, as a live
 *          iteration writes it; w and dev_pw are unspecified -- the SpMV still runs, with its ECC checks, its
 *          repairs and its events (the guard is in the vector kernels alone).  Replaying a frozen iteration any
 *          number of times changes nothing.
 * `threshold` is a kernel argument: a captured graph keeps the threshold it was captured with.
 * Enqueue-only and capturable; starts like every other entry (a pending x update applied, a speculation
 * voided) and leaves nothing pending: the x half runs inside the call.  abft_hip_tail_stats is left as it was.
 * What follows the SpMV is ALWAYS three kernels -- the fold of the fused product, the guarded r half, the
 * guarded x / p half -- never abft_hip_cg_iteration_dev's one launch: that kernel's hand-off counters must grow by
 * every launch's amounts, and a launch that returned early would break the bases its successor starts from.
 * The guarded kernels decide by one word that neither writes, uniformly over the grid; a frozen launch returns
 * before the reduction's ticket; no workgroup waits for another.
 * Before anything is enqueued the call checks that x, r, p and w have the matrix's row count, that no two of
 * them overlap, that vec overlaps none of x, r, w, and that p is vec's window [vec_offset, vec_offset + n) or
 * apart from vec; that the three scalar pairs are non-null and apart; it refuses ABFT_PART_INTERIOR and a context
 * with a peer board attached (one rank only: a frozen rank must never be the subject of a cross-rank wait).
 * Every matrix abft_hip_cg_iteration_dev takes is accepted. */
int abft_hip_cg_iteration_until_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec,
                                    int vec_offset, int part, abft_hip_vector *x, abft_hip_vector *r,
                                    abft_hip_vector *p, abft_hip_vector *w, const double *dev_rr,
                                    double *dev_pw, double *dev_rr_new, double threshold);

/* The guarded iteration with Jacobi preconditioning (dinv: abft_hip_jacobi): one iteration of the preconditioned
 * loop -- spmv(A, vec, w) with p.w, r -= alpha w, z = dinv r, x += alpha p, p = z + beta p -- behind the same stop
 * test on r.r, alpha = r.z / p.w and beta = r.z' / r.z formed on the device.
 * The scalars travel as device RECORDS of four doubles {r.r, queued events, r.z, 0.0}; the first two doubles of a
 * record are an ordinary pair (abft_hip_read_pair reads it).  dev_in: the record the iteration starts from (read
 * only), dev_out: the record it leaves, dev_pw: the pair {p.w, events} of the SpMV.
 *   LIVE   when dev_in[0] > threshold (false for NaN): bit for bit what abft_hip_spmv_dot_dev(A, vec, w, vec_offset,
 *          dev_pw), abft_hip_calc_xr_precond(x, r, p, w, dinv, dev_in[2] / dev_pw[0]) and
 *          abft_hip_calc_p_precond(p, r, dinv, r.z' / dev_in[2]) leave in x, r, p and w, with
 *          dev_out = {r.r', queued events, r.z', 0.0} the two sums abft_hip_calc_xr_precond returns.
 *   FROZEN otherwise: x, r and p keep every bit; dev_out[0] and dev_out[2] get the bits of dev_in[0] and dev_in[2]
 *          (moved as integers: a NaN keeps its payload), dev_out[1] the queued-event count, dev_out[3] 0.0; w and
 *          dev_pw are unspecified -- the SpMV still runs, with its ECC checks and events.  Replaying a frozen
 *          iteration changes nothing.
 * Always three kernels behind the SpMV (the fold of the fused product, the guarded r half, the guarded x / p half),
 * never abft_hip_cg_iteration_dev's one launch; abft_hip_tail_stats is left as it was.  Enqueue-only and capturable;
 * starts like every other entry (a pending x update applied, a speculation voided) and leaves nothing pending.
 * Refused before anything is enqueued: everything abft_hip_cg_iteration_until_dev refuses -- with the two records
 * of four doubles and the pair dev_pw apart from each other --, a null dinv, a dinv that does not have the vectors' length,
 * and a dinv that overlaps x, r, p, w or vec.
 * Under graph capture (abft_hip_graph_begin) the call needs the context's block partials, which the first
 * preconditioned (or block) call allocates and a capturing stream cannot: on a context that has made no such call
 * it returns ABFT_ERR_INVALID.  Make one eager preconditioned call first -- abft_hip_precond_start, which the loop
 * needs for its first record anyway.
 * Every matrix abft_hip_cg_iteration_until_dev takes is accepted. */
int abft_hip_pcg_iteration_until_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec,
                                     int vec_offset, int part, abft_hip_vector *x, abft_hip_vector *r,
                                     abft_hip_vector *p, abft_hip_vector *w, const abft_hip_vector *dinv,
                                     const double *dev_in, double *dev_pw, double *dev_out, double threshold);

/* The guarded iteration on PROTECTED vectors (the *_vecc entries above): x, r, p, w and vec hold codewords; the scalar
 * pairs are plain doubles in device memory, outside any code, as abft_hip_cg_iteration_until_dev keeps them.
 *   LIVE   when dev_rr[0] > threshold (false for NaN): bit for bit -- x, r, p, w, both pairs -- what
 *          abft_hip_spmv_vecc(A, vec, w), abft_hip_dot_vecc(p, w) served from its fused product,
 *          abft_hip_calc_r_vecc(r, w, rr / pw) and abft_hip_calc_px_vecc(x, p, r, rr / pw, rr_new / rr) leave, the
 *          quotients formed on the device.
 *   FROZEN otherwise: x, r and p keep every bit -- a word with a flipped bit included: a frozen launch of the two
 *          vector kernels repairs nothing and reports nothing --; dev_rr_new[0] gets the bits of dev_rr[0] (moved as
 *          an integer), dev_rr_new[1] the queued-event count; w and dev_pw are unspecified.  The SpMV still runs,
 *          with its matrix checks, its gather checks on vec and their events.  Replaying changes nothing.
 * Vector events (ABFT_EV_VEC_CORRECTED, ABFT_EV_VEC_DOUBLE) name their operand by its place among this entry's vector
 * arguments vec, x, r, p, w = 0 .. 4: the SpMV reports the gathered vector as 0, the r half r as 2 and w as 4, the
 * x / p half x as 1, r as 2 and p as 3.
 * Always three kernels behind the SpMV (the fold of the fused product, the guarded r half, the guarded x / p half);
 * enqueue-only and capturable -- every buffer it uses exists from abft_hip_init on, so also on a fresh context --;
 * starts like abft_hip_cg_iteration_until_dev and leaves nothing pending; abft_hip_tail_stats is left as it was.
 * Refused before anything is enqueued: everything abft_hip_cg_iteration_until_dev refuses, a COO matrix, and every
 * CSR layout abft_hip_spmv_vecc refuses (the message names the layout). */
int abft_hip_cg_vecc_iteration_until_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec,
                                         int vec_offset, int part, abft_hip_vector *x, abft_hip_vector *r,
                                         abft_hip_vector *p, abft_hip_vector *w, const double *dev_rr,
                                         double *dev_pw, double *dev_rr_new, double threshold);

/* The guarded Jacobi iteration on PROTECTED vectors: abft_hip_pcg_iteration_until_dev's protocol on codewords, dinv's
 * included.  Records of four plain doubles {r.r, queued events, r.z, 0.0}; dev_pw is the SpMV's pair.
 *   LIVE   when dev_in[0] > threshold (false for NaN): bit for bit -- x, r, p, w, dev_pw, dev_out -- what
 *          abft_hip_spmv_vecc(A, vec, w) with its fused product,
 *          abft_hip_calc_r_precond_vecc(r, w, dinv, dev_in[2] / dev_pw[0]) and
 *          abft_hip_calc_px_precond_vecc(x, p, r, dinv, that alpha, r.z' / dev_in[2]) leave, the quotients formed on
 *          the device.
 *   FROZEN otherwise: x, r, p and dinv keep every bit -- a word with a flipped bit included: a frozen launch of the two
 *          vector kernels repairs nothing and reports nothing --; dev_out[0] and dev_out[2] get dev_in's bits (moved
 *          as integers), dev_out[1] the queued-event count, dev_out[3] 0.0; w and dev_pw are unspecified.  The SpMV
 *          still runs, with its checks.
 * Vector events name their operand by its place among vec, x, r, p, w, dinv = 0 .. 5.
 * Always three kernels behind the SpMV (the fold, the guarded r half, the guarded x / p half); both guards decide on
 * dev_in[0], which neither kernel writes; a frozen launch returns before the reduction's ticket; no workgroup waits
 * for another.  Enqueue-only and capturable once the context holds its block partials: under graph capture on a
 * context that does not, ABFT_ERR_INVALID, and the message names the remedy -- one eager abft_hip_precond_start_vecc,
 * which allocates them and which the loop needs for its first record anyway.
 * Refused before anything is enqueued: everything abft_hip_cg_vecc_iteration_until_dev refuses, and everything
 * abft_hip_pcg_iteration_until_dev refuses about dinv and the records. */
int abft_hip_pcg_vecc_iteration_until_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec,
                                          int vec_offset, int part, abft_hip_vector *x, abft_hip_vector *r,
                                          abft_hip_vector *p, abft_hip_vector *w, abft_hip_vector *dinv,
                                          const double *dev_in, double *dev_pw, double *dev_out, double threshold);

/* ---- the guarded iterations on a PROTECTED TRAIL ----
 * The four single guarded entries above with their scalars under a SECDED code.  A trail word is a SLOT of 128 bits,
 * two doubles: the COO element {word 0, word 1, value = words 2, 3} of the reference's code in secded form, word 0
 * holding the word's ordinal in its record in bits 0..23 (record: 0 r.r, 1 events, 2 r.z, 3 the trailing 0.0; the
 * SpMV's pair: 0 p.w, 1 events) and the check byte in bits 24..31, word 1 zero, words 2 and 3 the double, every bit.
 * So the records are 4 doubles (the plain loops) or 8 (the preconditioned ones) and the pair is 4; all three must be
 * 16-byte aligned.  abft_hip_trail_encode / abft_hip_trail_decode are the host's view of them.
 *
 * Contracts as the unprotected twin's -- live / frozen on r.r, three kernels behind the SpMV, every refusal before
 * anything is enqueued, capturable under the same conditions, every matrix the twin accepts -- with these rules:
 *   - every launch checks every slot it reads, the ordinal under the code against the word's place included (a clean
 *     codeword in the wrong place, or with word 1 set, counts as two flips).  One flipped bit is repaired in registers by every thread; thread 0 of
 *     workgroup 0 stores the clean slot back and queues ABFT_EV_TRAIL_CORRECTED.  Hence dev_in is not const.
 *   - every slot written is a fresh encode of a value moved as an integer (the frozen hand-on included: it hands on
 *     the repaired bits, re-encoded).  For slots that decode clean the values are the unprotected twin's bits.
 *   - two flips in a slot the decision depends on (r.r; of a live record r.z; p.w; in the x / p half also the new
 *     record's r.z) queue ABFT_EV_TRAIL_DOUBLE, fatal, and the launch returns before it touches a vector, a partial or
 *     the ticket; the r half then hands the record on word for word, unrepaired.  x, r and p keep every bit.
 *   - no alpha scratch word: the x / p half forms alpha from the same two checked slots as the r half.
 * The events word and the trailing word of a record are not read on the device; abft_hip_trail_decode checks them.
 * Reduction partials and tickets stay plain: they live inside one iteration.  A peer board is refused. */
#define ABFT_TRAIL_START 0u /* the record the iteration starts from */
#define ABFT_TRAIL_PW 1u    /* the SpMV's pair */
#define ABFT_TRAIL_NEXT 2u  /* the record the iteration leaves */
int abft_hip_cg_trail_iteration_until_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec,
                                          int vec_offset, int part, abft_hip_vector *x, abft_hip_vector *r,
                                          abft_hip_vector *p, abft_hip_vector *w, double *dev_rr, double *dev_pw,
                                          double *dev_rr_new, double threshold);
int abft_hip_pcg_trail_iteration_until_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec,
                                           int vec_offset, int part, abft_hip_vector *x, abft_hip_vector *r,
                                           abft_hip_vector *p, abft_hip_vector *w, const abft_hip_vector *dinv,
                                           double *dev_in, double *dev_pw, double *dev_out, double threshold);
int abft_hip_cg_vecc_trail_iteration_until_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec,
                                               int vec_offset, int part, abft_hip_vector *x, abft_hip_vector *r,
                                               abft_hip_vector *p, abft_hip_vector *w, double *dev_rr, double *dev_pw,
                                               double *dev_rr_new, double threshold);
int abft_hip_pcg_vecc_trail_iteration_until_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, const abft_hip_vector *vec,
                                                int vec_offset, int part, abft_hip_vector *x, abft_hip_vector *r,
                                                abft_hip_vector *p, abft_hip_vector *w, abft_hip_vector *dinv,
                                                double *dev_in, double *dev_pw, double *dev_out, double threshold);

/* Host functions: n values -> n slots (2 n doubles), value i with ordinal first_ordinal + i; and back.
 * decode: values[i] the value (repaired when one bit was flipped), status[i] 0 clean, 1 one flip repaired, -1 two
 * flips (the value as stored), bits[i] the flipped bit (0..127) when status[i] == 1.  status and bits may be NULL. */
int abft_hip_trail_encode(const double *values, int n, int first_ordinal, double *slots);
int abft_hip_trail_decode(const double *slots, int n, double *values, int *status, int *bits);
/* enqueue an XOR of the given bits (0..127, numbered as the COO element's) into slot `slot` of the device slots at
 * dev_slots (16-byte aligned), like abft_hip_vector_flip */
int abft_hip_trail_flip(abft_hip_ctx *ctx, double *dev_slots, int slot, const int *bits, int nbits);
/* Reach a slot that lives only inside an iteration.  One shot: the next eager protected guarded call enqueues the XOR
 * of the given bits into slot `ordinal` of `record` (ABFT_TRAIL_START, ABFT_TRAIL_PW, ABFT_TRAIL_NEXT) behind the fold
 * (stage 1) or behind the r half (stage 2).  A capturing call with an injection armed returns ABFT_ERR_INVALID (and
 * leaves it armed), and so does a call whose record does not have that ordinal -- the pair has two words, a record of
 * the plain loops two, of the preconditioned ones four --, before anything is enqueued.  nbits == 0 disarms. */
int abft_hip_trail_inject_at(abft_hip_ctx *ctx, int stage, int record, int ordinal, const int *bits, int nbits);

/* The guarded iteration for k right-hand sides (block vectors, 1 <= k <= ABFT_MAX_RHS): one iteration of the fused
 * block loop -- W = A P with the k products P . W, then per column r -= alpha w, x += alpha p, p = r + beta p (with
 * dinv: p = dinv r + beta p) -- with the k alphas, the k betas and the COLUMN MASK formed on the device: column j runs
 * while ITS r.r is above the threshold.  dinv == NULL: the plain form.
 * The scalars travel as device RECORDS of 2k + 2 doubles: [j] = r.r of column j, [k + j] = its r.z (the plain form:
 * the bits of [j]), [2k] = the queued-event count, [2k + 1] = 0.0.  dev_in: the record the iteration starts from
 * (read only), dev_out: the record it leaves, dev_pw: k + 1 doubles, the k products and the queued-event count.
 *   Column j is LIVE when dev_in[j] > threshold (false for NaN): its column of X, R and P, dev_pw[j], dev_out[j] and
 *          dev_out[k + j] are bit for bit what abft_hip_spmm_dot, abft_hip_calc_r_block (abft_hip_calc_r_precond_block)
 *          and abft_hip_calc_px_block (abft_hip_calc_px_precond_block) leave when called with the mask of the live
 *          columns, alpha[j] = dev_in[k + j] / P.W[j] and beta[j] = r.z'[j] / dev_in[k + j] as IEEE quotients.
 *   FROZEN otherwise: its column of X, R and P keeps every bit; dev_out[j] and dev_out[k + j] get the bits of
 *          dev_in[j] and dev_in[k + j] (moved as integers: a NaN keeps its payload).
 * The SpMM always runs, with its ECC checks and events: W = A P in every column, as abft_hip_spmm_dot leaves it.
 * With no column live nothing else is touched but dev_pw and dev_out; replaying such an iteration changes nothing.
 * Four kernels in a line: the SpMM with its row-block partials, their fold, the guarded r half, the guarded x / p
 * half.  Every thread of both halves forms the mask from the same words of dev_in, which neither writes; no workgroup
 * waits for another.  Enqueue-only and capturable; starts like every other entry (a pending x update applied, a
 * speculation voided) and leaves nothing pending.
 * Refused before anything is enqueued, every operand left as it was: whatever abft_hip_spmm_dot refuses for (mat, P,
 * W, k); X, R, P, W that are not blocks of the matrix's rows, or overlap each other; a dinv that does not have the
 * matrix's row count or overlaps one of the four; null records or records that overlap each other (2k + 2, k + 1
 * and 2k + 2 doubles); a context with a peer board attached.
 * Under graph capture the call needs what a capturing stream cannot allocate -- the block partials, the SpMM's
 * partials for this matrix, the alpha scratch: on a context that does not hold them it returns ABFT_ERR_INVALID.
 * Call abft_hip_block_loop_reserve first; an eager call allocates them itself. */
int abft_hip_cg_block_iteration_until_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, abft_hip_vector *X,
                                          abft_hip_vector *R, abft_hip_vector *P, abft_hip_vector *W,
                                          const abft_hip_vector *dinv, int k, const double *dev_in, double *dev_pw,
                                          double *dev_out, double threshold);

/* The guarded block iteration on PROTECTED vectors: abft_hip_cg_block_iteration_until_dev with dinv == NULL, on
 * codewords.  X, R, P and W hold codewords; the records (2k + 2 doubles) and dev_pw (k + 1 doubles) are the plain
 * entry's: plain doubles in device memory, outside any code.
 *   Column j LIVE (dev_in[j] > threshold, false for NaN): its column of X, R and P, dev_pw[j], dev_out[j] and
 *          dev_out[k + j] are bit for bit what abft_hip_spmm_dot_vecc, abft_hip_calc_r_block_vecc and
 *          abft_hip_calc_px_block_vecc leave when called with the mask of the live columns, alpha[j] = dev_in[k + j] /
 *          P.W[j] and beta[j] = r.r'[j] / dev_in[k + j] as IEEE quotients.
 *   Column j FROZEN in a launch with a live column: dev_out[j] and dev_out[k + j] get the bits of dev_in[j] and
 *          dev_in[k + j] (moved as integers: a NaN keeps its payload); its words of R, X and P are checked and stored
 *          back repaired -- a clean word keeps every bit --, as those calls do with that mask.
 *   NO column live: X, R and P keep every bit, a word with a flipped bit included: such a launch of the two vector
 *          kernels repairs nothing and reports nothing; the record is handed on as integers with the queued-event
 *          count and 0.0; replaying changes nothing.  The SpMM still runs, with its matrix checks, its gather checks
 *          on P and their events.
 * Vector events (ABFT_EV_VEC_CORRECTED, ABFT_EV_VEC_DOUBLE) use the single guarded entries' numbering: 0 the P that
 * the SpMM gathers, 1 X, 2 R, 3 P, 4 W -- the r half reports R as 2 and W as 4, the x / p half X as 1, R as 2 and P
 * as 3 --, with index row * k + column.
 * Four kernels in a line: the protected SpMM with its row-block partials, their fold into dev_pw, the guarded r half,
 * the guarded x / p half; no workgroup waits for another.  Enqueue-only and capturable; leaves nothing pending.
 * Refused before anything is enqueued, every operand and record left as it was: everything
 * abft_hip_cg_block_iteration_until_dev refuses (overlaps, records, a peer board, k), and everything
 * abft_hip_spmm_dot_vecc refuses about the matrix (the message names the layout, or COO).
 * Under graph capture the call needs what abft_hip_block_loop_reserve allocates and returns ABFT_ERR_INVALID naming
 * it otherwise; an eager call allocates it itself. */
int abft_hip_cg_block_vecc_iteration_until_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, abft_hip_vector *X,
                                               abft_hip_vector *R, abft_hip_vector *P, abft_hip_vector *W, int k,
                                               const double *dev_in, double *dev_pw, double *dev_out, double threshold);

/* Allocate what abft_hip_cg_block_iteration_until_dev needs for this matrix and k (any k up to ABFT_MAX_RHS is then
 * covered), so that the iteration can be captured on a fresh context.  Eager only: refused under graph capture. */
int abft_hip_block_loop_reserve(abft_hip_ctx *ctx, abft_hip_matrix *mat, int k);

/* The two guarded block iterations on a PROTECTED TRAIL: abft_hip_cg_block_iteration_until_dev
 * and abft_hip_cg_block_vecc_iteration_until_dev with every scalar word a SECDED slot of two doubles, as in the single
 * trail entries above.  A slot holds the word's ordinal in its record -- r.r of column j: j, its r.z: k + j, the
 * events word 2k, the trailing word 2k + 1; in dev_pw P.W of column j: j, the events word k -- so a record is
 * 2 (2k + 2) doubles and dev_pw 2 (k + 1); all three must be 16-byte aligned (ABFT_ERR_INVALID otherwise) and apart.
 * Every launch of both halves checks all 2k value slots of the start record; a launch with a live column also P.W of
 * the LIVE columns and, in the x / p half, the next record's r.z of the live columns.  A frozen column's P.W slot is
 * not read.  One flipped bit: repaired by every thread in registers, stored back by one, one ABFT_EV_TRAIL_CORRECTED
 * event (index the ordinal, bit | record << 8); outputs are the clean call's.  Two flips in a slot read (a codeword
 * under the wrong ordinal counts as two): one ABFT_EV_TRAIL_DOUBLE event, the launch returns before it touches a
 * vector, a partial or the ticket, the r half hands the start record on word for word.  No column live: the record is
 * handed on repaired and re-encoded, nothing else is touched.  dev_in is repaired in place, hence not const.  The
 * context's alpha scratch is not used: the x / p half forms alpha_j from the same two checked slots.
 * Refusals are those of the plain entries, all before anything is enqueued; under capture
 * abft_hip_block_loop_reserve comes first. */
int abft_hip_cg_block_trail_iteration_until_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, abft_hip_vector *X,
                                                abft_hip_vector *R, abft_hip_vector *P, abft_hip_vector *W,
                                                const abft_hip_vector *dinv, int k, double *dev_in, double *dev_pw,
                                                double *dev_out, double threshold);
int abft_hip_cg_block_vecc_trail_iteration_until_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat, abft_hip_vector *X,
                                                     abft_hip_vector *R, abft_hip_vector *P, abft_hip_vector *W, int k,
                                                     double *dev_in, double *dev_pw, double *dev_out, double threshold);
/* abft_hip_trail_inject_at for the two entries above, with state of its own: armed for the next eager block trail
 * call, stage 1 behind the fold, stage 2 behind the r half.  ordinal in [0, 2 ABFT_MAX_RHS + 2); the iteration entry
 * refuses an ordinal its records do not have for its k (record 2k + 2 words, dev_pw k + 1), naming the word and the
 * record length, and any armed injection under capture; it stays armed then.  nbits == 0 disarms.  An injection
 * armed through abft_hip_trail_inject_at does not fire in a block call, nor this one in a single call. */
int abft_hip_block_trail_inject_at(abft_hip_ctx *ctx, int stage, int record, int ordinal, const int *bits, int nbits);

/* ---- a residual check whose verdict is formed and acted on on the device ----
 * abft_hip_residual_gap for the device-scalar loop: enqueue-only and capturable, nothing comes back to the host but
 * what it downloads from dev_chk later.  Three things in a line on the context's stream:
 *   1. scratch = A x, the SpMV of abft_hip_residual_gap (every format, layout and mode; its checks, repairs, events);
 *   2. dev_chk[0..3] = {gap2, tt2, verdict, queued events}: gap2 = sum ((b - scratch) - r)^2 and tt2 =
 *      sum (b - scratch)^2 are bit for bit what abft_hip_residual_gap returns for the same operands; verdict = 1.0
 *      (passed) when gap2 <= limit and both sums are finite, else 2.0 (a NaN fails the comparison);
 *   3. every thread of a third kernel reads the verdict: passed, x_ckpt <- x; failed, x <- x_ckpt (plain copies: an
 *      inf or NaN moves as it is).  No workgroup waits for another.
 * b and r are only read.  Starts like abft_hip_residual_gap (a pending x update applied, cached results forgotten).
 * Refused before anything is enqueued: a null argument, what abft_hip_residual_gap refuses about the lengths and the
 * scratch vector, an x_ckpt that has not x's length or overlaps b, x, r or scratch, and dev_chk within one of the
 * vectors.  Under graph capture the context must hold the partials of a K-wide reduction: ABFT_ERR_INVALID naming
 * abft_hip_residual_check_reserve otherwise; an eager call allocates them itself. */
int abft_hip_residual_check_dev(abft_hip_ctx *ctx, abft_hip_matrix *A, const abft_hip_vector *b,
                                abft_hip_vector *x, const abft_hip_vector *r, abft_hip_vector *scratch,
                                abft_hip_vector *x_ckpt, double *dev_chk, double limit);
/* Allocate what abft_hip_residual_check_dev needs, so that it can be captured on a fresh context.  Idempotent.
 * Eager only: ABFT_ERR_INVALID under graph capture. */
int abft_hip_residual_check_reserve(abft_hip_ctx *ctx);

/* ---- graph replay ------------------------------------------------------ */

/* Capture everything enqueued on the context's stream between begin and end -- the
 * asynchronous calls of this library (spmv*, *_dev forms, calc_p*, copy) and whatever the
 * caller enqueues on abft_hip_get_stream() meanwhile (RCCL collectives) -- into a hipGraph
 * and replay it with one launch.  Nothing that synchronises may be called in between
 * (dot / calc_xr with host results, map, drain_events), kernel brackets must be off, and a
 * calc_xr must be followed by its calc_p inside the same capture.  The fixed-iteration CG
 * loop of the drivers (-c 0: cg.cpp:94-118 with alpha and beta kept on the device) is
 * captured this way. */
typedef struct abft_hip_graph abft_hip_graph;
int abft_hip_graph_begin(abft_hip_ctx *ctx);
int abft_hip_graph_end(abft_hip_ctx *ctx, abft_hip_graph **graph);
int abft_hip_graph_launch(abft_hip_graph *graph);
int abft_hip_graph_destroy(abft_hip_graph *graph);

/* ---- matrix digests ---------------------------------------------------- */

/* Once abft_hip_matrix_create_* returns, the arrays of a matrix that kernels read are constant for its life: the only
 * legitimate writes are ECC repairs, which store the original word back.  A SEGMENT is one such device allocation,
 * viewed as little-endian 32-bit words w[0..n) over the whole allocation, padding included (the last word
 * zero-extended when the byte length is no multiple of 4), n <= 2^31, and its digest is
 *     D = sum of w[i] * (2 i + 1)  mod 2^64,
 * which every single and every double bit flip inside the segment changes (csrc/matrix_digest.h has the argument;
 * three or more flips can cancel).  A digest taken once (arm) and recomputed now and then (verify) therefore detects
 * corruption of any stored array, in every mode, format and layout, for one streaming read of the matrix per
 * verification.  It detects, it does not repair: after a mismatch the caller re-creates the matrix.  Not covered:
 * compute faults, the vectors, a flip that an ECC mode repairs between two verifications.  The reference digests
 * sit unprotected in device memory: a flip there is a false alarm, never a miss.
 *
 * The segment kinds are a fixed list (csrc/matrix_digest.h, ABFT_SEG_*); abft_hip_segment_name gives a kind's name
 * ("cols", "pal", "wbase", ...; NULL past the end of the list).  The progress boards, debug buffers, the moved list
 * and the fused product's partials are written by kernels and are no segments.  The entries that rewrite matrix
 * arrays on purpose (abft_hip_inject and the re-planning behind it, abft_hip_inject_rowptr, abft_hip_inject_structure,
 * abft_hip_matrix_write_structure, abft_hip_matrix_flip_segment) leave the armed digests alone: an injected flip is
 * the fault to be found. */
const char *abft_hip_segment_name(uint32_t kind);
/* Which segments this matrix has, in the order every other entry here uses: kinds[k], bytes[k] for k < min(cap, *count);
 * *count = how many there are (kinds / bytes may be NULL with cap 0). */
int abft_hip_matrix_segments(abft_hip_matrix *mat, uint32_t *kinds, uint64_t *bytes, int cap, int *count);
/* The current digests, out[k] for segment k (cap >= the segment count, else ABFT_ERR_INVALID).  Synchronous; not under
 * graph capture.  The first digest call on a matrix allocates its segment table and accumulators. */
int abft_hip_matrix_digest(abft_hip_ctx *ctx, abft_hip_matrix *mat, uint64_t *out, int cap);
/* Compute the digests and keep them as the reference, on the host and in device memory.  Arming again takes a new
 * reference.  Nothing is armed at create: a matrix that is never armed makes exactly the launches and allocations
 * it made before these entries existed.  Synchronous; not under graph capture. */
int abft_hip_matrix_digest_arm(abft_hip_ctx *ctx, abft_hip_matrix *mat);
/* Recompute and compare: *bad_count segments differ, bad_kinds[0 .. min(cap, *bad_count)) name them in segment
 * order.  Synchronous; queues no event.  ABFT_ERR_INVALID on a matrix that is not armed (the message names
 * abft_hip_matrix_digest_arm). */
int abft_hip_matrix_verify(abft_hip_ctx *ctx, abft_hip_matrix *mat, int *bad_count, uint32_t *bad_kinds, int cap);
/* The same as two launches enqueued on the context's stream, nothing else: matrix_digest_kernel over all segments, and
 * behind it one workgroup that compares, queues one ABFT_EV_MATRIX_DIGEST event per differing segment and zeroes the
 * accumulators.  It allocates nothing and waits for nothing, so it can be captured into a graph; the verdict arrives
 * with the next drain.  ABFT_ERR_INVALID on a matrix that is not armed. */
int abft_hip_matrix_verify_dev(abft_hip_ctx *ctx, abft_hip_matrix *mat);
/* The tests' and the command line's injector for arrays no other injector reaches.  read_segment copies the first
 * `bytes` bytes of the segment of that kind to buf (bytes <= the segment's).  flip_segment XORs the listed bits
 * (0..31, nbits <= 32) into stored word `word` of the segment, as the digest numbers the words; in a zero-extended
 * last word only the bits of stored bytes may be named.  Raw writes: no copy of the array anywhere else follows. */
int abft_hip_matrix_read_segment(abft_hip_ctx *ctx, abft_hip_matrix *mat, uint32_t kind, void *buf, uint64_t bytes);
int abft_hip_matrix_flip_segment(abft_hip_ctx *ctx, abft_hip_matrix *mat, uint32_t kind, uint64_t word, const int *bits,
                                 int nbits);

/* ---- events ------------------------------------------------------------ */

/* Synchronise, then move the queued events to `buf` (at most `cap`), sorted
 * by (index, kind) and cut after the first fatal one -- the order a
 * single-threaded reference run prints them in.  *count = events returned,
 * *fatal = 1 if the last one is fatal (the reference would have exit(1)ed).
 * Vector events (ABFT_FMT_VECTOR) equal in all four fields are reported once per
 * drain: every gatherer of one vector entry sees the same flip.  The duplicates
 * are already suppressed on the device -- the first thread to meet a flipped word
 * queues it, the others find its key in a table that this call clears --, so a
 * flipped entry of a dense column costs one slot of the queue, not one per row
 * that gathers it, and cannot overflow it. */
int abft_hip_drain_events(abft_hip_ctx *ctx, abft_event *buf, int cap, int *count, int *fatal);
/* Capacity of the device event queue = the `cap` with which drain never truncates.
 * drain returns ABFT_ERR_RANGE (after filling buf / count / fatal) if the device queued
 * more events than that, or if `cap` is smaller than the events due. */
int abft_hip_event_capacity(void);
/* Number of events queued as of the last synchronising call (no sync). */
int abft_hip_pending_events(abft_hip_ctx *ctx);
/* The reference's exact printf line for an event, including the newline. */
int abft_format_event(const abft_event *ev, char *buf, size_t cap);
int abft_event_is_fatal(uint32_t kind);

/* ---- measurement ------------------------------------------------------- */

typedef enum {
  ABFT_K_SPMV = 0,
  ABFT_K_DOT = 1,
  ABFT_K_CALC_XR = 2,
  ABFT_K_CALC_P = 3,
  ABFT_K_COUNT = 4
} abft_kernel_id;

/* `mask` bit k (1 << abft_kernel_id) brackets every launch of kernel k with HIP
 * events on the context's stream; 0 switches profiling off.  A bracket costs
 * two event records per launch, so measure throughput with only the kernel of
 * interest enabled.  abft_hip_profile_read synchronises and returns the summed
 * device time (ms) and launch count since the last reset.  With the fused dot
 * (spmv on a square matrix), ABFT_K_DOT times the small fold kernel that is left
 * of dot(p, w).  abft_hip_profile_stride(n) brackets only every n-th launch of an
 * enabled kernel (default 1): a sampled average at 1/n of the cost. */
int abft_hip_profile_enable(abft_hip_ctx *ctx, int mask);
int abft_hip_profile_stride(abft_hip_ctx *ctx, int stride);
int abft_hip_profile_reset(abft_hip_ctx *ctx);
int abft_hip_profile_read(abft_hip_ctx *ctx, int kernel, double *total_ms, long *launches);

/* Device streaming-copy bandwidth probe (bytes moved = 2*bytes per rep):
 * the measured-peak denominator SURVEY 8(d) asks for beside the 8 TB/s spec. */
int abft_hip_stream_probe(abft_hip_ctx *ctx, size_t bytes, int reps, double *gbps_copy,
                          double *gbps_read);

#ifdef __cplusplus
}
#endif
#endif /* ABFT_HIP_H */
