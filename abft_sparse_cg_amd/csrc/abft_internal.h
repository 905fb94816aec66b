// abft_internal.h -- shared between kernels.hip (device code + launchers) and
// abft_hip.hip (the C ABI).  Not part of the public boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/abft_hip.h"

// Device-side event queue: one entry per printf line of the reference backend.
struct EventRing {
  abft_event *buf;
  uint32_t *count;  // total pushed (may exceed cap; extra events are dropped)
  uint32_t cap;
};

// Behind the `cap` events of EventRing::buf, in the same allocation: the table of vector events already
// queued since the last drain (kernels.hip vecc_cold), ABFT_VECC_SEEN_SLOTS 64-bit keys, 0 = free.  It is
// cleared wherever EventRing::count is reset.
#define ABFT_VECC_SEEN_SLOTS 4096u
#define ABFT_VECC_SEEN_PROBES 8u

// CSR matrix as the kernels see it.  cols/vals keep the reference's SoA layout
// (CSR/CPUContext.h:11-18) so element i is {vals[i], cols[i]}; both arrays are
// over-allocated by 2 elements so the paired loads never leave the buffer.
struct CsrDev {
  uint32_t *cols;
  double *vals;
  const uint32_t *rowptr;   // n_out + 1
  const uint4 *blk;         // nblk : {first row, end row, first element, end element} of each row block
  uint32_t nblk, n_out, n_in, nnz, index_base;
  // Panel layout only (see CsrPanels): elements are stored grouped by
  // (row group, column panel); these map storage position <-> caller's index.
  const uint32_t *orig_index;   // cold path: event messages carry the caller's element index
  const uint32_t *pos_of_orig;  // inject
  const uint32_t *gidx;         // shards whose elements are not one run of the caller's: global index of local element k
};

// Mode none, streaming row-block layout: the columns a second time, as 16-bit offsets from a
// per-block base, for the blocks the SpMV stages as one tile and whose columns span at most
// 65536 values (banded matrices: all of them).  The SpMV then streams 2 bytes per column
// instead of 4.  `cols` stays the authoritative copy (read back, inject, every other kernel and
// mode); every writer of a column keeps cbase[b] + cols16[i] == cols[i] for the elements of a
// compact block b, or marks the block wide.  Kept out of CsrDev, which every CSR kernel takes
// by value: there two more pointers would move the argument offsets of all of them.
#define ABFT_CBASE_WIDE 0xFFFFFFFFu
struct CsrCompact {
  const uint16_t *cols16;  // cols' padded length + 2 (8-byte loads at every even index), or NULL: none compact
  const uint32_t *cbase;   // nblk: the block's smallest column, or ABFT_CBASE_WIDE (read through cols)
};

// Mode none, streaming row-block layout: *packed* blocks, whose elements the SpMV reads as one
// u16 code each -- column and value together, 2 bytes instead of 10 -- for the blocks it stages
// as one tile that hold at most 16 distinct values (by 64-bit pattern) and whose columns fit the
// bits the palette index leaves: k = ceil(log2(#values)), shift = 16 - k, max - min col < 2^shift.
//   col = cbase + (code & ((1 << shift) - 1)),   val = pal[pbase + (code >> shift)]
// Palettes are padded to 16 entries (any index a code can hold stays inside its own palette) and
// shared by every block with the same value set (config 2: one palette of {-1, 4}).  `vals` and
// `cols` stay authoritative; abft_hip_inject re-plans a packed block it flips (packed anew, or the
// compact / wide path).  Kept apart from CsrDev and CsrCompact for the same reason as CsrCompact.
#define ABFT_PAL_ENTRIES 16u
struct CsrPacked {
  const uint16_t *code16;  // cols' padded length + 2, or NULL: none packed
  const uint2 *pdesc;      // nblk: {cbase, (pbase / 16) << 5 | shift}; .y == 0: not packed (shift is 12..16)
  const double *pal;       // the palette pool, ABFT_PAL_ENTRIES per palette
};
// ... and what the SpMV may skip on a packed block (layout_plan.h, packed_fast_word, which proves it at plan time): one
// word per row block, 0: the general path.  Bit 0: staged with unclamped code loads and unchecked gathers
// (csr_stage_packed_fast); bits 8..11: besides, rows of that one length, summed without row pointers or clamps.
// The word travels in a 16-byte record {cbase, descriptor's second word, fast word, 0} per block, an array of its own
// beside pdesc (which keeps every bit): the kernels that read the word -- spmv_csr_kernel<MODE_NONE, ..., VECC = false,
// ...> -- load the record INSTEAD of the descriptor, one scalar load as before.  A struct of its own, the LAST kernel
// argument: a fourth pointer in CsrPacked would move XUpd's argument offsets in every instantiation.
// (layout_plan.h, which a CPU build includes without this header, has the same three lines)
#define ABFT_FAST_STAGE 1u
#define ABFT_FAST_LEN_SHIFT 8u
#define ABFT_FAST_LEN_MAX 8u
struct CsrPackedFast {
  const uint4 *rec;  // nblk records, or NULL: nothing packed
};

// A structure-protected matrix (struct_ecc.h; abft_hip_matrix_create_csr_protected): the row structure as codewords.
// CsrDev::rowptr and CsrDev::blk are NULL on such a matrix -- no plain copy exists --, and only the kernels that take
// this struct run on it.  Not const: a cold path stores a repaired word back.
struct CsrStruct {
  uint64_t *rowext;  // n_out row extent words
  uint4 *blk;        // nblk stored descriptors
};

// Panel ("column-blocked") layout for matrices whose columns are scattered over
// a vector much larger than an XCD's 4 MB L2 (random / unstructured).  Rows are
// cut into groups of ABFT_PANEL_ROWS, columns into panels of `width` entries
// (2 MB of x); the elements of one (row group, panel) segment are contiguous and
// keep their (row, col) order.  A workgroup owns a row group, keeps the running
// row sums in registers and sweeps the panels in ascending order -- the same
// order of additions as the row-by-row sum, so y stays bit-identical -- while all
// resident workgroups gather from the same 2 MB window of x at a time, which the
// L2 then serves (the streaming layout misses L2 on 7 of 8 gathers here).
struct CsrPanels {
  const uint32_t *seg_base;  // ngroups * npanels + 1 : first element of each segment
  const uint16_t *seg_ptr;   // per segment ABFT_PANEL_ROWS + 1 row offsets relative to seg_base
  uint32_t ngroups, npanels;
  unsigned long long *debug;  // optional (ABFT_HIP_PANEL_DEBUG, -DABFT_DBG_STAMPS builds): 2 x 8 phase clocks, first / later launches
  uint32_t *pace;             // COO panel kernel run as ONE launch over all panels: a progress board per XCD (as SweepLayout), else NULL
  uint32_t lag;               // workgroups of an XCD stay within `lag` panels of its slowest; 0: no pacing
  uint32_t width;             // gather indices per panel
  uint32_t xpf;               // COO panel kernel: entering a panel, the workgroups of an XCD touch the NEXT panel's lines of x (into that XCD's L2)
};
// Sweep layout: the panel layout's successor (same idea: (output group, gather-index panel)
// segments, outputs' additions in the caller's order) run as ONE persistent launch:
//   * a workgroup owns a group of 256 * RPT outputs for the whole sweep; thread (wave w,
//     lane l) keeps the running sums of outputs w*64*RPT + j*64 + l (j < RPT) in
//     registers from the first panel to the last -- y is written once (the chunked panel
//     launches carried the sums through y: 7 extra round trips of y on config 4);
//   * per (segment, row) only a COUNT is stored (1 byte; a matrix with more than 255 elements
//     of one row in one panel keeps the panel layout), laid out so that a thread loads its
//     RPT counts with one access; the element offsets come from
//     a DPP prefix scan over the wave plus one stored base per (segment, wave)
//     (the 16-bit offset tables of the panel layout were 134 MB on config 4);
//   * what keeps every workgroup of an XCD inside the same window of the gathered vector is
//     not a kernel boundary but pacing through a per-XCD progress board (kernels.hip,
//     board_load): speed only, never correctness; every wait is bounded.
struct SweepLayout {
  const uint32_t *wbase;   // nseg * 4 + 1 : first element of (segment, wave); segment s = [wbase[4s], wbase[4s+4])
  const uint8_t *counts;   // [segment][thread 0..255][j 0..RPT-1], one byte each
  uint32_t ngroups, npanels;
  uint32_t *pace;          // exit ticket, registrations per XCD, a progress board per XCD (kernels.hip: PACE_*)
  uint32_t lag;            // workgroups of an XCD stay within `lag` panels of its slowest; 0: no pacing
  uint32_t *debug;         // optional (ABFT_HIP_SWEEP_DEBUG): {polls that waited, waits, workgroup exits}, never reset
  unsigned long long *debug_wg;  // optional, -DABFT_DBG_STAMPS builds: per workgroup {clocks in all, at the pacing check, staging, hardware id}
};

// Slice layout (round 3; opt-in, ABFT_HIP_LAYOUT=slice: built to test whether the sweep kernel's bookkeeping
// is what keeps it from the gather path's floor -- it is not, DESIGN.md section 4 "Round 3" -- and measured
// slower).  What the sweep kernel pays per (row, panel) CELL -- a count byte, a share of a prefix scan, a
// range test, a branch, and a workgroup barrier per tile -- is as much as it pays per element (config 4:
// 26 panels x 16 rows = 416 cells for 400 elements per thread).  Here nothing is per cell:
//   * rows are cut into SLICES of 2^rows_log2 consecutive rows; a slice belongs to ONE WAVE, which
//     keeps the slice's running row sums in its own piece of LDS -- no other wave ever touches them,
//     so the kernel has no barrier and no atomics at all;
//   * a slice's elements are stored as one run ordered by (panel of the gather index, row, caller's
//     order), each with its row inside the slice as a 16-bit id: the wave streams the run 64 elements
//     per instruction -- chunks run straight across panel boundaries, every chunk but a slice's last
//     is full -- and each element is added onto its row's sum in LDS, in storage order (the lanes
//     of one chunk that share a row are folded in lane order by the first of them, over DPP);
//     a row's elements therefore meet its sum in the caller's order (panels ascend; inside a panel a
//     row's elements keep their order): y stays bit-identical to the reference;
//   * `sub` (first element of every (slice, panel)) is only read for panel ranges and pacing.
struct SliceLayout {
  const uint32_t *sub;   // nslices * (npanels + 1): first stored element of (slice, panel); [.. + npanels] = the slice's end
  const uint16_t *rid;   // per stored element: row - (slice << rows_log2) + 1 (0: no element -- a load past the end)
  uint32_t nslices, npanels, rows_log2;
  uint32_t *pace;        // a progress board per XCD (as SweepLayout::pace)
  uint32_t lag;          // 0: no pacing
};

#ifndef ABFT_CFG_SLICE_K
#define ABFT_CFG_SLICE_K 2  // chunks of 64 elements a wave of the slice kernel keeps in flight
#endif
#ifndef ABFT_CFG_SLICE_WAVES
#define ABFT_CFG_SLICE_WAVES 8  // waves per SIMD the slice kernel is compiled for (register budget)
#endif

#ifndef ABFT_CFG_PANEL_RPT
#define ABFT_CFG_PANEL_RPT 8  // outputs per thread of the panel kernels (4: equal on config 4, -14% on config 5)
#endif
constexpr int ABFT_PANEL_ROWS_PER_THREAD = ABFT_CFG_PANEL_RPT;
constexpr int ABFT_PANEL_ROWS = 256 * ABFT_PANEL_ROWS_PER_THREAD;

// COO only: elements whose stored column no longer names the output group they are
// stored in (a silently corrupted column: modes none/constraints, or multi-bit damage
// an ECC mode cannot see).  The reference scatters such a product into
// result[corrupted col] (COO/CPUContext.cpp:120); the SpMV kernels leave it out of the
// group's sum and queue it here, and coo_fixup_kernel, launched behind every COO SpMV,
// rebuilds each receiving output in the caller's element order.  Empty on clean data.
struct MovedEntry {
  uint32_t orig;  // caller's (local) element index: the position in the reference's serial loop
  uint32_t col;   // the output the reference adds this product to (< n_out)
  double prod;    // value * vec[row], as the SpMV formed it
};
struct MovedList {
  MovedEntry *buf;     // 2 * cap entries: [0, cap) filled by the SpMV, [cap, 2 cap) sorted by the fix-up
  uint32_t *count;     // entries pushed by the SpMV in flight (reset by the fix-up)
  uint32_t cap;
};

// COO matrix: 16-byte elements {col,row,value} (COO/ecc.h:11-16) stored grouped
// by output index (col) and, inside a group, in the caller's order -- so each
// output is still summed in the reference's storage order.
struct CooDev {
  uint4 *elems;
  const uint32_t *grp_ptr;      // n_out + 1
  const uint4 *blk;             // nblk : {first group, end group, first element, end element}
  const uint32_t *orig_index;   // stored position -> caller's element index (cold path)
  const uint32_t *pos_of_orig;  // caller's element index -> stored position
  const uint2 *as_created;      // constraints mode: {col,row} of every stored element as create_matrix left it (or its complement: see kernels.hip)
  uint32_t nblk, n_out, n_in, nnz, index_base;
  MovedList moved;
  const uint32_t *gidx;         // column-block shards: global (caller's) index of local element k; else index_base + k
};

#define ABFT_COLMASK_HOST 0x00FFFFFFu

// Tuning knobs (overridable with -D for A/B builds; defaults are the measured best)
#ifndef ABFT_CFG_CSR_EPT
#define ABFT_CFG_CSR_EPT 4
#endif
#ifndef ABFT_CFG_PACKED_PAL
#define ABFT_CFG_PACKED_PAL 0  // packed tiles' palette lookup: 0 ds_bpermute, 1 scalar-loaded + selects, 2 vector load
#endif
#ifndef ABFT_CFG_COO_EPT
#define ABFT_CFG_COO_EPT 4
#endif
#ifndef ABFT_CFG_PANEL_EPT
#define ABFT_CFG_PANEL_EPT 8  // elements per thread per tile of the panel-layout kernel (4: -9%)
#endif
#ifndef ABFT_CFG_SWEEP_EPT
#define ABFT_CFG_SWEEP_EPT 8  // CSR elements per thread per tile of the sweep kernel
#endif
#ifndef ABFT_CFG_COO_PANEL_EPT
#define ABFT_CFG_COO_PANEL_EPT 4  // 16-byte elements per thread per tile of the COO panel kernel
#endif
#ifndef ABFT_CFG_DEAD_NT
#define ABFT_CFG_DEAD_NT 0  // non-temporal loads of values read for the last time this iteration: bit 0 w in calc_r, 1 r in calc_px, 2 p in calc_px
#endif
#ifndef ABFT_CFG_SWEEP_COUNTS_NT
#define ABFT_CFG_SWEEP_COUNTS_NT 0  // sweep kernel: the per-(segment, row) counts by non-temporal loads
#endif
#ifndef ABFT_CFG_PX_OUT_NT
#define ABFT_CFG_PX_OUT_NT 0  // calc_px writing into shadow buffers (speculation): non-temporal stores, bit 0 x, bit 1 p
#endif
#ifndef ABFT_X_IN_SPMV_MODES
#define ABFT_X_IN_SPMV_MODES 0x01u  // the x update inside the next SpMV (abft_hip.hip, xpend): bit m = armed by default on matrices of ECC mode m -- `none` only: in the five other modes the alternated series showed no gain, in sed a loss (profiles/r11/mode_*)
#endif
#ifndef ABFT_CFG_XUPD_NT
#define ABFT_CFG_XUPD_NT 7  // spmv_csr_kernel<..., NUPD>: non-temporal access to the update's streams, bit 0 the p_old load, 1 the x load, 2 the x store (0: 2-3 % slower than without the update; 7 with P_OUT_NT: 5 % faster, profiles/r11)
#endif
#ifndef ABFT_CFG_P_OUT_NT
#define ABFT_CFG_P_OUT_NT 1  // calc_p writing the new p into the buffer its handle swaps to (xpend): non-temporal stores
#endif
#ifndef ABFT_CFG_R_NT
#define ABFT_CFG_R_NT 0  // calc_r_kernel's r store, non-temporal: bit 0 into the shadow of a run-ahead (r_out != r), bit 1 in place (profiles/r12/variants_ab.md)
#endif
#ifndef ABFT_CFG_Y_NT
#define ABFT_CFG_Y_NT 0  // spmv_csr_kernel<MODE_NONE, ..., NUPD>: the y[row] store non-temporal (profiles/r12/variants_ab.md)
#endif
#ifndef ABFT_PACKED_FAST_DEFAULT
#define ABFT_PACKED_FAST_DEFAULT 1  // the predicate-free path on packed blocks proven safe (CsrPackedFast) without ABFT_HIP_PACKED_FAST: 0 off, 1 on (profiles/r15)
#endif
#ifndef ABFT_AHEAD_DEFAULT
#define ABFT_AHEAD_DEFAULT 1  // run-ahead of the host-scalar loop (abft_hip.hip, spec.ahead) without ABFT_HIP_AHEAD: 0 off, 1 calc_p, 2 calc_r and calc_p -- 1: level 1 passed the rule against level 0 and the parent, level 2 did not pass it against level 1 (profiles/r12/variants_ab.md), nor with the deferred finishes (profiles/r13/bench_ab.md)
#endif
#ifndef ABFT_LAZY_X_DEFAULT
#define ABFT_LAZY_X_DEFAULT 2  // queue depth of the x updates without ABFT_HIP_LAZY_X (loop_state.h, LazyUpdates): 1 no queue, 2 or 4: every 2nd / 4th predicted SpMV applies that many in one pass -- 2: its slowest run lay above the fastest of depth 1 and of the parent, depth 4's did not lie above depth 2's fastest (profiles/r14/bench_ab.md)
#endif
#ifndef ABFT_DEFER_FINISH_DEFAULT
#define ABFT_DEFER_FINISH_DEFAULT 1  // without ABFT_HIP_DEFER_FINISH: the reductions in front of a run-ahead kernel leave their finish to its head (loop_state.h, RunAhead::defer_finish) -- 1: at level 1 its slowest run lay above the parent's fastest (profiles/r13/bench_ab.md)
#endif
#ifndef ABFT_CFG_X_NT
#define ABFT_CFG_X_NT 0 // calc_px: x (touched once per iteration) by non-temporal loads and stores
#endif
#ifndef ABFT_CFG_COO_LEAN_WAVES
#define ABFT_CFG_COO_LEAN_WAVES 8  // register budget of spmv_coo_lean_kernel, in waves per SIMD (8: 64 VGPRs)
#endif
#ifndef ABFT_CFG_COO_PANEL_XPF_AHEAD
#define ABFT_CFG_COO_PANEL_XPF_AHEAD 1  // the x prefetch of the COO panel kernel runs this many panels ahead
#endif
#ifndef ABFT_CFG_COO_PANEL_PREFETCH
#define ABFT_CFG_COO_PANEL_PREFETCH 0  // COO panel kernel: the next tile's streaming loads issued behind this tile's gathers
#endif
#ifndef ABFT_CFG_COO_SCHED_BARRIER
#define ABFT_CFG_COO_SCHED_BARRIER 1  // bit m: COO kernels of mode m keep their streaming loads together (kernels.hip)
#endif
#ifndef ABFT_CFG_COO_PANEL_SHORT_SUMS
#define ABFT_CFG_COO_PANEL_SHORT_SUMS 1  // COO panel kernel's ordered sums two-wide instead of four-wide
#endif
#ifndef ABFT_CFG_SWEEP_SHORT_SUMS
#define ABFT_CFG_SWEEP_SHORT_SUMS 1  // sweep kernel's row sums: two LDS reads in flight per step instead of four
#endif
#ifndef ABFT_CFG_SWEEP_PREFETCH
#define ABFT_CFG_SWEEP_PREFETCH 0  // bit 0: 8 rows per thread, bit 1: 16 (see spmv_sweep_kernel)
#endif
#ifndef ABFT_CFG_SCHED_BARRIER
#define ABFT_CFG_SCHED_BARRIER 1
#endif
#ifndef ABFT_CFG_UNIFORM_ROWS
#define ABFT_CFG_UNIFORM_ROWS 1  // row blocks of equal-length rows are flagged and skip the row-pointer loads
#endif
#ifndef ABFT_CFG_NT
#define ABFT_CFG_NT 1  // stream cols/vals with the non-temporal hint
#endif
#ifndef ABFT_CFG_XCD
#define ABFT_CFG_XCD 1  // tile order: 0 dispatch order, 1 contiguous range per XCD, 2 chunked
#endif
#ifndef ABFT_CFG_XCD_CHUNK
#define ABFT_CFG_XCD_CHUNK 32
#endif

constexpr int ABFT_BLOCK = 256;
constexpr int ABFT_CSR_EPT = ABFT_CFG_CSR_EPT;           // elements per thread per tile
constexpr int ABFT_CSR_TILE = ABFT_BLOCK * ABFT_CSR_EPT;  // nnz staged per block
constexpr int ABFT_COO_EPT = ABFT_CFG_COO_EPT;
constexpr int ABFT_COO_TILE = ABFT_BLOCK * ABFT_COO_EPT;
#ifndef ABFT_CFG_MAX_PARTIALS
#define ABFT_CFG_MAX_PARTIALS 2048  // 256 CUs x 8 (1024: calc_px 7 % slower; 4096: calc_r 10 % slower)
#endif
constexpr int ABFT_MAX_PARTIALS = ABFT_CFG_MAX_PARTIALS;  // reduction blocks
constexpr int ABFT_TICKET_GROUP = 32;    // blocks per first-level arrival counter
constexpr int ABFT_TICKET_WORDS = 1 + ABFT_MAX_PARTIALS / ABFT_TICKET_GROUP;  // [0] top, [1..] groups

hipError_t launch_encode_csr(int mode, uint32_t *cols, double *vals, uint32_t nnz, hipStream_t s);
hipError_t launch_encode_coo(int mode, uint4 *elems, uint32_t nnz, hipStream_t s);
hipError_t launch_inject_csr(double *vals, uint32_t *cols, const uint32_t *pos_of_orig, uint32_t index,
                             const int *bits_dev, int nbits, hipStream_t s);
hipError_t launch_inject_coo(uint4 *elems, const uint32_t *pos_of_orig, uint32_t index,
                             const int *bits_dev, int nbits, hipStream_t s);

// Pinned, device-visible result slot: the reduction's last block writes the
// scalar and the queued-event count, then publishes `seq` with a system-scope
// release store; the host spins on `seq` instead of synchronising the stream.
struct HostSlot {
  double value;
  uint32_t evcount;
  uint32_t seq;
};

// peer board (all-reduce of a pair across the processes of one node, see kernels.hip):
// [2 rows][ABFT_PEER_MAX_RANKS] slots, then one failure flag per rank
#define ABFT_PEER_MAX_RANKS 64
struct PeerSlot {
  unsigned long long v0, v1, seq, pad;
};
#define ABFT_PEER_BOARD_BYTES (2 * ABFT_PEER_MAX_RANKS * sizeof(PeerSlot) + ABFT_PEER_MAX_RANKS * sizeof(uint32_t))
// ... as the tail of a reduction: the block that finishes the shard's sum also takes it over the
// board (size == 0: no)
struct PeerArgs {
  PeerSlot *const *boards;  // replicated board (device memory): every rank's copy, by rank (device table); else NULL
  PeerSlot *board;
  unsigned long long *counter;
  uint32_t *fail;
  int rank, size;
  unsigned long long timeout_ticks;
};

// Where a reduction delivers its result.  Every block writes one partial, takes
// a ticket (agent-scope release before, acquire after for the last arriver), and
// the block that draws the last ticket adds the partials in a fixed order, so the
// value does not depend on which block that is.
struct ReduceOut {
  double *partials;          // ABFT_MAX_PARTIALS doubles
  uint32_t *ticket;          // ABFT_TICKET_WORDS counters, zero between launches (last arrivers reset them)
  double *dev_out;           // optional: {sum, queued events} as two doubles
  HostSlot *host;            // optional: device alias of the pinned slot
  const uint32_t *ev_count;  // the context's device event counter
  uint32_t seq;              // value to publish in host->seq
  PeerArgs peers;            // dev_out form: {sum, events} summed over the ranks of the board before it is stored
};

// Cross-call fusion: an SpMV on a square matrix also forms
// sum_row vec[row] * result[row], so the dot(p, w) the CG loop asks for right
// after spmv(A, p, w) needs no pass over the vectors.  Each block leaves one
// partial; a small kernel behind the SpMV (one workgroup, or several for many partials:
// launch_fuse_finalize) folds them in a fixed order and
// publishes the scalar like a reduction does.  `partials` belongs to the matrix.
struct FuseOut {
  double *partials;  // one per SpMV workgroup
  HostSlot *host;    // publish to the pinned slot (host-scalar form) ...
  double *dev_out;   // ... or {sum, queued events} to device memory (device-scalar form)
  const uint32_t *ev_count;
  uint32_t seq;
  uint32_t x_off;    // the product uses vec[x_off + row] (a shard's slot in the gathered vector)
  PeerArgs peers;    // as in ReduceOut
};

// Which row blocks (tiles) of a streaming-layout CSR matrix one launch covers:
// workgroup b takes tile first + b, plus `skip` once b >= cut.  Whole matrix:
// {0, nblk, 0, nblk}; interior rows of a shard: {t_lo, n, 0, n}; the rest:
// {0, t_lo, t_hi - t_lo, nblk - (t_hi - t_lo)}.
struct TileSpan {
  uint32_t first, cut, skip, count;
};

// spmv_csr_kernel<..., NUPD>: the n (1, 2 or 4) updates x += u[k].alpha * u[k].p_old the launch applies row by row, k = 0 first
// (abft_hip.hip "xpend", and the queue of loop_state.h's LazyUpdates); axpy_chain_kernel: 1 to 4 of them
struct XUpd {
  double *xs;
  struct { const double *p_old; double alpha; } u[4];  // (pairs: one update's arguments lie where they lay before there were four)
  int n;
};

// sweep-layout SpMV (modes other than constraints): panels [c0, c1) in one persistent launch of
// `grid` workgroups (all resident); c0 > 0 resumes from the sums a previous launch left in y
hipError_t launch_spmv_sweep(int mode, int rpt, const CsrDev &A, const SweepLayout &L, const double *x, double *y,
                             EventRing ev, const FuseOut *fuse, uint32_t grid, uint32_t c0, uint32_t c1, hipStream_t s);
int spmv_sweep_blocks_per_cu(int mode, int rpt);  // rpt: 2, 4, 8 or 16
// slice-layout SpMV (modes other than constraints): panels [c0, c1), `grid` workgroups of 4 waves
hipError_t launch_spmv_slice(int mode, const CsrDev &A, const SliceLayout &L, const double *x, double *y, EventRing ev,
                             const FuseOut *fuse, uint32_t grid, uint32_t c0, uint32_t c1, hipStream_t s);
int spmv_slice_blocks_per_cu(int mode, uint32_t rows_log2);

// panel-layout SpMV (modes other than constraints); `grid` = resident workgroups
hipError_t launch_spmv_csr_panels(int mode, const CsrDev &A, const CsrPanels &P, const double *x, double *y,
                                  EventRing ev, const FuseOut *fuse, uint32_t grid, uint32_t chunk,
                                  hipStream_t s);
int spmv_csr_panels_blocks_per_cu(int mode, bool fuse);
hipError_t launch_spmv_coo_panels(int mode, const CooDev &A, const CsrPanels &P, const double *x, double *y,
                                  EventRing ev, const FuseOut *fuse, uint32_t grid, uint32_t chunk,
                                  hipStream_t s);
// fuse == nullptr: plain SpMV; otherwise follow with launch_fuse_finalize
// (`big`: where a multi-workgroup fold of many partials meets; see fold_partials_kernel)
struct FixArgs;
hipError_t launch_fuse_finalize(const FuseOut &f, uint32_t nblk, const ReduceOut &big, const FixArgs *fix, hipStream_t s);
// the grid of a multi-workgroup fold of nblk partials (-> workgroups, *chunk partials each): launch_fuse_finalize's
// many-partials path, launch_spmm_fold and launch_spmm_fold_dev all use it
uint32_t fold_grid(uint32_t nblk, uint32_t *chunk);
// vecc: x and y hold protected elements (abft_hip_spmv_vecc)
hipError_t launch_spmv_csr(int mode, const CsrDev &A, const CsrCompact &cc, const CsrPacked &cp, const TileSpan &span,
                           const double *x, double *y, EventRing ev, const FuseOut *fuse, hipStream_t s,
                           bool vecc = false, const XUpd *xu = nullptr, CsrPackedFast pf = CsrPackedFast{nullptr});
// the same on a structure-protected matrix (never with compact or packed blocks, never with an x update)
hipError_t launch_spmv_csr_struct(int mode, const CsrDev &A, const CsrStruct &S, const TileSpan &span, const double *x,
                                  double *y, EventRing ev, const FuseOut *fuse, hipStream_t s, bool vecc);
// S as uploaded (packed row words, plain descriptors) -> the stored codewords, in place
hipError_t launch_struct_encode(const CsrStruct &S, uint32_t n, uint32_t nblk, hipStream_t s);
// counts[0] += repaired words, counts[1] += uncorrectable ones
hipError_t launch_struct_scrub(const CsrStruct &S, uint32_t n, uint32_t nblk, uint32_t *counts, EventRing ev, hipStream_t s);
hipError_t launch_spmv_coo(int mode, const CooDev &A, const double *x, double *y, EventRing ev,
                           const FuseOut *fuse, hipStream_t s);
// behind every COO SpMV: see MovedList.  With a fused product the fix-up runs inside the fold
// (launch_fuse_finalize's `fix`), else as its own one-workgroup launch.
// where output c's own elements sit: the one group (streaming layout), or its slice of
// segment (group, panel rg) in the panel layout
struct FixLayout {
  int kind;  // 0 streaming, 1 panels
  CsrPanels P;
};
struct FixArgs {
  CooDev A;
  FixLayout F;
  const double *x;
  double *y;
  double *partial0;  // the fused product's partial 0 (corrected in place), or nullptr
  uint32_t x_off;
  int ecc;           // the stored column carries ECC bits (mask them)
  int on;            // 0: nothing to do (not a COO matrix)
};
FixArgs make_fix_args(int mode, const CooDev &A, const CsrPanels *P, const double *x, double *y, const FuseOut *fuse);
hipError_t launch_coo_fixup(const FixArgs &fx, hipStream_t s);

// cg_tail_kernel (kernels.hip): fold of the SpMV's fused partials + calc_r + calc_px in one launch
struct TailArgs {
  FuseOut f;            // the SpMV's partials, dev_out = the {p.w, events} pair, peers for its all-reduce
  uint32_t nparts;      // how many partials
  uint32_t fold_nb, fold_chunk;  // many partials (> 8192): folded in fold_nb chunks first (launch_fuse_finalize's rule); else 0
  FixArgs fx;           // COO fix-up (on = 0: none)
  ReduceOut o;          // partials = the context's block partials, dev_out = the {r.r, events} pair, peers
  const double *rr;     // this iteration's r.r (device)
  double *x, *r, *p;
  const double *w;
  int n;
  uint32_t nbv;         // reduce_blocks(n): the grid calc_r_kernel / calc_px_kernel would run on
  unsigned long long *sync;  // 32 words that never go back: counters, flags and the bases a launch leaves for the next (kernels.hip)
  unsigned long long timeout_ticks;  // wall_clock64 ticks (100 MHz) a workgroup waits at a hand-off at most
};
int spmv_coo_panels_blocks_per_cu(int mode);
int spmv_coo_pc_blocks_per_cu(int mode);
int spmv_coo_lean_blocks_per_cu(int mode);
hipError_t launch_spmv_coo_lean(int mode, const CooDev &A, const CsrPanels &P, const double *x, double *y, EventRing ev,
                                const FuseOut *fuse, uint32_t grid, uint32_t chunk, hipStream_t s);
hipError_t launch_spmv_coo_pc(int mode, const CooDev &A, const CsrPanels &P, const double *x, double *y, EventRing ev,
                              const FuseOut *fuse, uint32_t grid, uint32_t chunk, hipStream_t s);
int cg_tail_blocks_per_cu(bool vec2, bool fast, int q);  // q: virtual 256-thread blocks per workgroup (4, 2, 1)
hipError_t launch_cg_tail(const TailArgs &a, bool vec2, bool fast, int q, uint32_t grid, hipStream_t s);

int reduce_blocks(int n);
hipError_t launch_dot(const double *a, const double *b, int n, const ReduceOut &out, hipStream_t s);
// alpha = num ? *num / *den : alpha (device-resident scalars: no host round trip)
hipError_t launch_calc_xr(double *x, double *r, const double *p, const double *w, double alpha,
                          const double *num, const double *den, int n, const ReduceOut &out, hipStream_t s);
hipError_t launch_calc_p(double *p, const double *r, double beta, const double *num, const double *den, int n,
                         hipStream_t s, double *p_out = nullptr);
hipError_t launch_calc_r(double *r, const double *w, double alpha, const double *num, const double *den,
                         double *alpha_out, int n, const ReduceOut &out, hipStream_t s, double *r_out = nullptr,
                         const double *x = nullptr, const double *p = nullptr);
hipError_t launch_calc_px(double *p, const double *r, double *x, double beta, const double *num, const double *den,
                          double alpha, const double *alpha_ptr, int n, hipStream_t s, double *p_out = nullptr,
                          double *x_out = nullptr);
// ---- reductions finished by the launch behind them (kernels.hip, deferred_head) ----
// The producer leaves its block partials and ends; every block of the consumer folds them at its head as the last
// arriver of the ticket form would have (the same bits), and its block 0 publishes {sum, queued events} as `head`
// says (partials: where the producer left them; dev_out, host, ev_count, seq as in the ticket form; no ticket, no peers).
// Only for a pair enqueued back to back in one call; the partials' area is the reduction's until the consumer has ended.
// launch_calc_r without its finish -> reduce_blocks(n) partials at block_partials.  head: it is also the consumer of
// the deferred fold in front of it (head_nb chunk sums): alpha = *num / that p.w
hipError_t launch_calc_r_defer(double *r, const double *w, double alpha, const double *num, const double *den,
                               double *alpha_out, int n, double *block_partials, hipStream_t s, double *r_out,
                               const double *x, const double *p, const ReduceOut *head, uint32_t head_nb);
// launch_calc_p with beta = (the r.r of `head`, nb partials) / *den
hipError_t launch_calc_p_head(const double *p, const double *r, const double *den, int n, hipStream_t s, double *p_out,
                              const ReduceOut &head, uint32_t nb);
// does launch_fuse_finalize take the multi-workgroup form (the one with a finish to defer) for nblk partials?
bool fuse_finalize_folds(uint32_t nblk);
// that form without its finish -> *nb_out chunk sums at chunk_sums
hipError_t launch_fuse_finalize_defer(const FuseOut &f, uint32_t nblk, double *chunk_sums, const FixArgs *fix,
                                      uint32_t *nb_out, hipStream_t s);
// the head alone, in one block: behind a deferred producer whose consumer could not be launched
hipError_t launch_deferred_finish(const ReduceOut &head, uint32_t nb, hipStream_t s);
hipError_t launch_axpy(double *x, const double *p, double alpha, const double *alpha_ptr, int n, hipStream_t s);
// x += u.u[0].alpha * u.u[0].p_old, then u.u[1], ... u.u[u.n - 1] (1 <= u.n <= 4) over n elements: launch_axpy u.n times, x read and written once
hipError_t launch_axpy_chain(const XUpd &u, int n, hipStream_t s);
// the two halves of a guarded iteration (abft_hip_cg_iteration_until_dev): live when *rr > threshold -- then what
// launch_calc_r (alpha = *rr / *pw, left in alpha_out) and launch_calc_px (beta = *rr_new / *rr) do --, else nothing
// but the new pair out.dev_out = {the bits of *rr, queued events}
hipError_t launch_calc_r_until(double *r, const double *w, const double *rr, const double *pw, double threshold,
                               double *alpha_out, int n, const ReduceOut &out, hipStream_t s, const double *x,
                               const double *p);
hipError_t launch_calc_px_until(double *p, const double *r, double *x, const double *rr, const double *rr_new,
                                double threshold, const double *alpha_ptr, int n, hipStream_t s);

// ---- the guarded iteration on a protected trail (trail_ecc.h; abft_hip_*_trail_iteration_until_dev) ----
// the scalars of one iteration: records and pair as SECDED slots, 16-byte aligned; `in` is repaired in place
struct TrailIter {
  double *in, *pw, *out;
  double threshold;
  EventRing ev;
};
struct ReduceOutD;
// launch_fuse_finalize with {p.w, events} published as slots (no peers, no pinned slot)
hipError_t launch_fuse_finalize_trail(const FuseOut &f, uint32_t nblk, const ReduceOut &big, const FixArgs *fix,
                                      hipStream_t s);
// the two halves of the four loops (vecc: codewords; precond: dinv and records of four slots, reduced through od, else
// pairs through o); x, p of the r half: for the plain loop's choice of walk only
hipError_t launch_trail_r_until(bool vecc, bool precond, double *r, const double *w, double *dinv, const double *x,
                                const double *p, const TrailIter &t, int n, const ReduceOut &o, const ReduceOutD &od,
                                hipStream_t s);
hipError_t launch_trail_px_until(bool vecc, bool precond, double *x, double *p, const double *r, double *dinv,
                                 const TrailIter &t, int n, hipStream_t s);
// XOR mask[4] into the slot at `slot`
hipError_t launch_flip_trail(double *slot, const uint32_t mask[4], hipStream_t s);

// ---- block right-hand sides (abft_hip_spmm and the *_block vector calls; 1 <= K <= 8) ----
#define ABFT_MAX_RHS 8
// the K-wide form of HostSlot: K results of one reduction, published by `seq`
struct HostSlotK {
  double value[ABFT_MAX_RHS];
  uint32_t evcount;
  uint32_t seq;
};
struct ReduceOutK {
  double *partials;          // ABFT_MAX_RHS * ABFT_MAX_PARTIALS doubles: column j's block partials at j * ABFT_MAX_PARTIALS
  uint32_t *ticket;          // as ReduceOut::ticket
  HostSlotK *host;           // device alias of the pinned slot
  const uint32_t *ev_count;
  uint32_t seq;
};
struct BlockScalars {
  double v[ABFT_MAX_RHS];
};
// Y = A X on the streaming row-block CSR layout, k in [2, 8] (k = 1 is launch_spmv_csr)
hipError_t launch_spmm_csr(int mode, int k, const CsrDev &A, const double *x, double *y, EventRing ev, hipStream_t s);
// n = rows of the block vectors (n * k doubles each)
hipError_t launch_dot_block(const double *a, const double *b, int n, int k, const ReduceOutK &out, hipStream_t s);
hipError_t launch_calc_xr_block(double *x, double *r, const double *p, const double *w, int n, int k,
                                const BlockScalars &alpha, uint32_t active, const ReduceOutK &out, hipStream_t s);
hipError_t launch_calc_p_block(double *p, const double *r, int n, int k, const BlockScalars &beta, uint32_t active,
                               hipStream_t s);
// as launch_spmm_csr, k in [1, 8], on a square matrix; and column j's product x[:, j] . y[:, j] as A.nblk
// partials at dotp + j * A.nblk (plain stores), which launch_spmm_fold sums and publishes in the K-wide slot
hipError_t launch_spmm_dot_csr(int mode, int k, const CsrDev &A, const double *x, double *y, EventRing ev,
                               double *dotp, hipStream_t s);
hipError_t launch_spmm_fold(const double *parts, uint32_t nblk, int k, const ReduceOutK &out, hipStream_t s);
// r -= alpha w alone (the r half of launch_calc_xr_block, its sums)
hipError_t launch_calc_r_block(double *r, const double *w, int n, int k, const BlockScalars &alpha, uint32_t active,
                               const ReduceOutK &out, hipStream_t s);
// x += alpha p; p = r + beta p, or with dinv p = dinv * r + beta p
hipError_t launch_calc_px_block(double *x, double *p, const double *r, const double *dinv, int n, int k,
                                const BlockScalars &alpha, const BlockScalars &beta, uint32_t active, hipStream_t s);
// residual checks (abft_hip_residual_*): 2k sums of a block check come back in one wide slot
struct HostSlotW {
  double value[2 * ABFT_MAX_RHS];
  uint32_t evcount;
  uint32_t seq;
};
struct ReduceOutW {
  double *partials;          // 2 * ABFT_MAX_RHS * ABFT_MAX_PARTIALS doubles, value j's at j * ABFT_MAX_PARTIALS
  uint32_t *ticket;          // as ReduceOut::ticket
  HostSlotW *host;           // device alias of the pinned slot
  const uint32_t *ev_count;
  uint32_t seq;
};
hipError_t launch_flip_vector(double *v, unsigned long long mask, hipStream_t s);
// ---- protected vectors (abft_hip_*_vecc): the words of ecc_device.h's (64, 57) code ----
hipError_t launch_vector_encode(double *v, int n, hipStream_t s);
// counts[0] += repaired words, counts[1] += uncorrectable ones
hipError_t launch_vector_scrub(double *v, int n, uint32_t *counts, EventRing ev, hipStream_t s);
hipError_t launch_dot_vecc(const double *a, const double *b, int n, const ReduceOut &out, EventRing ev, hipStream_t s);
hipError_t launch_calc_xr_vecc(double *x, double *r, const double *p, const double *w, double alpha, int n,
                               const ReduceOut &out, EventRing ev, hipStream_t s);
hipError_t launch_calc_p_vecc(double *p, const double *r, double beta, int n, EventRing ev, hipStream_t s);
// the two-kernel tail on protected vectors: calc_xr_vecc's r half, and its x half inside
// calc_p_vecc's pass over p; each chooses its walk by the alignment of its own operands
hipError_t launch_calc_r_vecc(double *r, const double *w, double alpha, int n, const ReduceOut &out, EventRing ev,
                              hipStream_t s);
hipError_t launch_calc_px_vecc(double *x, double *p, const double *r, double alpha, double beta, int n, EventRing ev,
                               hipStream_t s);
// the fused block iteration on protected block vectors: launch_spmm_dot_csr,
// launch_dot_block, launch_calc_r_block and launch_calc_px_block on codewords
hipError_t launch_spmm_dot_vecc_csr(int mode, int k, const CsrDev &A, const double *x, double *y, EventRing ev,
                                    double *dotp, hipStream_t s);
hipError_t launch_dot_block_vecc(const double *a, const double *b, int n, int k, const ReduceOutK &out, EventRing ev,
                                 hipStream_t s);
hipError_t launch_calc_r_block_vecc(double *r, const double *w, int n, int k, const BlockScalars &alpha,
                                    uint32_t active, const ReduceOutK &out, EventRing ev, hipStream_t s);
hipError_t launch_calc_px_block_vecc(double *x, double *p, const double *r, int n, int k, const BlockScalars &alpha,
                                     const BlockScalars &beta, uint32_t active, EventRing ev, hipStream_t s);
// their guarded forms (abft_hip_cg_vecc_iteration_until_dev): launch_calc_r_until's / launch_calc_px_until's protocol
hipError_t launch_calc_r_vecc_until(double *r, const double *w, const double *rr, const double *pw, double threshold,
                                    double *alpha_out, int n, const ReduceOut &out, EventRing ev, hipStream_t s);
hipError_t launch_calc_px_vecc_until(double *x, double *p, const double *r, const double *rr, const double *rr_new,
                                     double threshold, const double *alpha_ptr, int n, EventRing ev, hipStream_t s);
// {gap2, tt2} = {sum ((b - y) - r)^2, sum (b - y)^2} through the K-wide slot (values 0, 1)
hipError_t launch_residual_gap(const double *b, const double *y, const double *r, int n, const ReduceOutK &out,
                               hipStream_t s);
// r = b - y, p = r; r.r as launch_dot(r, r) forms it
hipError_t launch_residual_restart(const double *b, const double *y, double *r, double *p, int n, const ReduceOut &out,
                                   hipStream_t s);
// n = rows of the block vectors; out value 2j: gap2 of column j, 2j + 1: tt2 (0 for columns not in `active`)
hipError_t launch_residual_gap_block(const double *b, const double *y, const double *r, int n, int k, uint32_t active,
                                     const ReduceOutW &out, hipStream_t s);
hipError_t launch_residual_restart_block(const double *b, const double *y, double *r, double *p, int n, int k,
                                         uint32_t mask, const ReduceOutK &out, hipStream_t s);
hipError_t launch_copy_block(double *dst, const double *src, int n, int k, uint32_t mask, hipStream_t s);
// Jacobi preconditioning (abft_hip_*_precond*): z = dinv * r formed in registers; {r.z, r.r} through the K-wide
// slot (values 0, 1), the block forms' 2k sums (2j: r.z, 2j + 1: r.r of column j) through the wide one
hipError_t launch_precond_start(const double *r, const double *dinv, double *p, int n, const ReduceOutK &out,
                                hipStream_t s);
// x == nullptr: r -= alpha w alone (x += alpha p is deferred to launch_calc_p_precond)
hipError_t launch_calc_xr_precond(double *x, double *r, const double *p, const double *w, const double *dinv,
                                  double alpha, int n, const ReduceOutK &out, hipStream_t s);
// p = z + beta p; x != nullptr: and x += alpha p with p as it was
hipError_t launch_calc_p_precond(double *p, const double *r, const double *dinv, double *x, double beta, double alpha,
                                 int n, hipStream_t s);
// the two halves of a guarded preconditioned iteration (abft_hip_pcg_iteration_until_dev).  Scalars travel as device
// records of four doubles {r.r, queued events, r.z, 0.0}; live when in[0] > threshold -- then what
// launch_calc_xr_precond(x == nullptr) (alpha = in[2] / *pw, left in alpha_out) and launch_calc_p_precond(x != nullptr)
// (beta = out[2] / in[2]) do --, else nothing but the record handed on: out = {bits of in[0], events, bits of in[2], 0.0}
struct ReduceOutD {
  double *partials;          // 2 * ABFT_MAX_PARTIALS doubles at least: r.z's block partials at 0, r.r's at ABFT_MAX_PARTIALS
  uint32_t *ticket;          // as ReduceOut::ticket
  double *dev_out;           // the record (device memory)
  const uint32_t *ev_count;
};
hipError_t launch_calc_r_precond_until(double *r, const double *w, const double *dinv, const double *in,
                                       const double *pw, double threshold, double *alpha_out, int n,
                                       const ReduceOutD &out, hipStream_t s);
hipError_t launch_calc_px_precond_until(double *p, const double *r, const double *dinv, double *x, const double *in,
                                        const double *out, double threshold, const double *alpha_ptr, int n,
                                        hipStream_t s);
// Jacobi preconditioning on protected vectors: the r / px cut of launch_calc_r_vecc /
// launch_calc_px_vecc with z = dec(dinv) * r formed in registers, {r.z, r.r} as launch_precond_start returns them; each
// chooses its walk by the alignment of ALL its operands.  dinv is not const: the cold path stores a repaired word back.
hipError_t launch_precond_start_vecc(const double *r, double *dinv, double *p, int n, const ReduceOutK &out,
                                     EventRing ev, hipStream_t s);
hipError_t launch_calc_r_precond_vecc(double *r, const double *w, double *dinv, double alpha, int n,
                                      const ReduceOutK &out, EventRing ev, hipStream_t s);
hipError_t launch_calc_px_precond_vecc(double *x, double *p, const double *r, double *dinv, double alpha, double beta,
                                       int n, EventRing ev, hipStream_t s);
// their guarded forms (abft_hip_pcg_vecc_iteration_until_dev): launch_calc_r_precond_until's / _px_precond_until's protocol
hipError_t launch_calc_r_precond_vecc_until(double *r, const double *w, double *dinv, const double *in,
                                            const double *pw, double threshold, double *alpha_out, int n,
                                            const ReduceOutD &out, EventRing ev, hipStream_t s);
hipError_t launch_calc_px_precond_vecc_until(double *x, double *p, const double *r, double *dinv, const double *in,
                                             const double *out, double threshold, const double *alpha_ptr, int n,
                                             EventRing ev, hipStream_t s);
// the guarded block iteration (abft_hip_cg_block_iteration_until_dev).  Scalars travel as device records of 2k + 2
// doubles {r.r of the k columns, their r.z (plain: the bits of r.r), queued events, 0.0}, the SpMM's products as
// k + 1 doubles {P.W of the k columns, queued events}.  Column j is live when in[j] > threshold, decided by every
// thread of both halves from the same words; a live column gets what launch_calc_r_block / launch_calc_r_precond_block
// (alpha[j] = in[k + j] / pw[j], left in alpha_out[0..k)) and launch_calc_px_block (beta[j] = out[k + j] / in[k + j])
// do with that mask, a frozen one keeps its bits and its record words; no column live: nothing but the record handed on
struct ReduceOutB {
  double *partials;          // 2 * ABFT_MAX_RHS * ABFT_MAX_PARTIALS doubles, value j's at j * ABFT_MAX_PARTIALS
  uint32_t *ticket;          // as ReduceOut::ticket
  double *dev_out;           // the record, or {P.W, events} (device memory)
  const uint32_t *ev_count;
};
// launch_spmm_fold with the k totals and the events word left in out.dev_out[0..k]
hipError_t launch_spmm_fold_dev(const double *parts, uint32_t nblk, int k, const ReduceOutB &out, hipStream_t s);
// dinv == nullptr: the plain forms
hipError_t launch_calc_r_block_until(double *r, const double *w, const double *dinv, const double *in,
                                     const double *pw, double threshold, double *alpha_out, int n, int k,
                                     const ReduceOutB &out, hipStream_t s);
hipError_t launch_calc_px_block_until(double *x, double *p, const double *r, const double *dinv, const double *in,
                                      const double *out, double threshold, const double *alpha_ptr, int n, int k,
                                      hipStream_t s);
// their protected twins (abft_hip_cg_block_vecc_iteration_until_dev): the plain forms' protocol in front of the walks
// of launch_calc_r_block_vecc / launch_calc_px_block_vecc; vector events count X, R, P, W as operands 1..4
hipError_t launch_calc_r_block_vecc_until(double *r, const double *w, const double *in, const double *pw,
                                          double threshold, double *alpha_out, int n, int k, const ReduceOutB &out,
                                          EventRing ev, hipStream_t s);
hipError_t launch_calc_px_block_vecc_until(double *x, double *p, const double *r, const double *in, const double *out,
                                           double threshold, const double *alpha_ptr, int n, int k, EventRing ev,
                                           hipStream_t s);
// the same four on a protected trail (trail_ecc.h, TrailBlock<K>; abft_hip_cg_block[_vecc]_trail_iteration_until_dev):
// records of 2 (2k + 2) doubles, the tail 2 (k + 1), 16-byte aligned; t.in is repaired in place; out.dev_out: the tail
// for the fold, t.out for the r half.  No alpha scratch.  vecc: codewords, no dinv
hipError_t launch_spmm_fold_trail(const double *parts, uint32_t nblk, int k, const ReduceOutB &out, hipStream_t s);
hipError_t launch_block_trail_r_until(bool vecc, double *r, const double *w, const double *dinv, const TrailIter &t,
                                      int n, int k, const ReduceOutB &out, hipStream_t s);
hipError_t launch_block_trail_px_until(bool vecc, double *x, double *p, const double *r, const double *dinv,
                                       const TrailIter &t, int n, int k, hipStream_t s);
// launch_residual_gap with its two sums, the verdict and the events word left in out.dev_out[0..3] (device memory):
// verdict 1.0 when gap2 <= limit and both sums are finite, else 2.0 (abft_hip_residual_check_dev)
hipError_t launch_residual_check(const double *b, const double *y, const double *r, int n, double limit,
                                 const ReduceOutB &out, hipStream_t s);
// behind it: chk[2] == 1.0: x_ckpt <- x, else x <- x_ckpt (n doubles each, disjoint)
hipError_t launch_residual_guard(double *x, double *x_ckpt, const double *chk, int n, hipStream_t s);
hipError_t launch_precond_start_block(const double *r, const double *dinv, double *p, int n, int k, uint32_t mask,
                                      const ReduceOutW &out, hipStream_t s);
hipError_t launch_calc_xr_precond_block(double *x, double *r, const double *p, const double *w, const double *dinv,
                                        int n, int k, const BlockScalars &alpha, uint32_t active, const ReduceOutW &out,
                                        hipStream_t s);
hipError_t launch_calc_p_precond_block(double *p, const double *r, const double *dinv, int n, int k,
                                       const BlockScalars &beta, uint32_t active, hipStream_t s);
hipError_t launch_calc_r_precond_block(double *r, const double *w, const double *dinv, int n, int k,
                                       const BlockScalars &alpha, uint32_t active, const ReduceOutW &out,
                                       hipStream_t s);
// dinv[i] = 1 / (sum of row i's diagonal elements) over the stored arrays of the streaming CSR / grouped COO
// layout; *bad (device) counts the rows left at 1.0
hipError_t launch_diag_csr(const CsrDev &A, uint32_t colmask, double *dinv, uint32_t *bad, hipStream_t s);
hipError_t launch_diag_coo(const CooDev &A, uint32_t colmask, double *dinv, uint32_t *bad, hipStream_t s);
hipError_t launch_publish_pair(const double *pair, HostSlot *host, uint32_t seq, hipStream_t s);

// window exchange over shared host memory (see kernels.hip, peer_exchange_kernel): a 4 KB header
// -- ready[rank], done[rank] sequence numbers, fail[rank] -- then per rank two outboxes (parity)
#define ABFT_PEER_MAX_PIECES 63
#define ABFT_PEER_XHDR_BYTES 4096
struct PeerPiece {
  unsigned long long box_off;  // bytes from the start of the SENDER's outbox
  unsigned int vec_off;        // doubles from the start of the gathered vector (this rank's copy)
  unsigned int count;          // doubles
  int peer;                    // out: who reads it; in: whose outbox it sits in
  int pad;
};
struct PeerExchange {  // lives in device memory
  unsigned char *const *regions;  // device-memory transport: every rank's region by rank (device table); else NULL
  unsigned char *shared;       // device alias of the mapping
  unsigned long long *counter; // sequence number of the last exchange
  int rank, size, nout, nin;
  unsigned long long box_bytes, timeout_ticks;
  PeerPiece out[ABFT_PEER_MAX_PIECES], in[ABFT_PEER_MAX_PIECES];
};
hipError_t launch_peer_exchange(const PeerExchange *X, double *full, hipStream_t s);
hipError_t launch_peer_allreduce(double *pair, const PeerArgs &P, hipStream_t s);
hipError_t launch_copy(double *dst, const double *src, int n, hipStream_t s);
hipError_t launch_stream_copy(double *dst, const double *src, size_t n, hipStream_t s);
hipError_t launch_stream_read(const double *src, size_t n, double *sink, hipStream_t s);

// ---- matrix digests (matrix_digest.h; abft_hip_matrix_digest / _arm / _verify / _verify_dev) ----
struct DigestSeg;
// acc[k] += D(segment k) for the nseg rows of `table` (device memory), one launch of `grid` workgroups over all of them
hipError_t launch_matrix_digest(const DigestSeg *table, uint32_t nseg, unsigned long long *acc, uint32_t grid, hipStream_t s);
// behind it, one workgroup: pairs[2k] = acc[k], pairs[2k + 1] = ref[k]; one ABFT_EV_MATRIX_DIGEST event per k where they
// differ (index = the segment's kind); acc[k] = 0
hipError_t launch_matrix_digest_finish(const DigestSeg *table, uint32_t nseg, unsigned long long *acc,
                                       const unsigned long long *ref, unsigned long long *pairs, EventRing ev, uint32_t fmt,
                                       hipStream_t s);
