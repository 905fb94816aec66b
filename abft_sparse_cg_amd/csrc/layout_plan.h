// layout_plan.h -- everything that decides how a matrix is stored: row blocks, compact columns, packed codes, the
// panel / sweep / slice layouts, the COO grouping, and the launch geometry that follows from them.
// Host code only, no HIP header, and the environment is never asked here: abft_hip.hip reads it once per create into a
// LayoutKnobs (read_knobs, given the lookup), fills a PlanGeometry from the constants of abft_internal.h, asks a plan
// here, and uploads what comes back; tests/host/layout_plan_play.cpp does the same with no GPU, also at a toy
// geometry.  Every array made here is a table a kernel indexes without a bounds check.  Nothing here allocates device
// memory, launches or fails.  Expects ABFT_PAL_ENTRIES and ABFT_CBASE_WIDE (abft_internal.h) and ABFT_PAL_SPARE
// (abft_hip.hip) defined before inclusion.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <optional>
#include <vector>

#if !defined(ABFT_PAL_ENTRIES) || !defined(ABFT_CBASE_WIDE) || !defined(ABFT_PAL_SPARE)
#error "layout_plan.h: define ABFT_PAL_ENTRIES, ABFT_CBASE_WIDE (abft_internal.h) and ABFT_PAL_SPARE (abft_hip.hip) first"
#endif

// a row block {first segment, end segment (bit 31: rows of equal length), first element, end element} and a pair of
// words, laid out as the uint4 / uint2 the kernels read (abft_hip.hip asserts it where it uploads them)
struct Blk { uint32_t x, y, z, w; };
struct Pair { uint32_t x, y; };

// the sizes the planners cut by (abft_internal.h: ABFT_BLOCK, ABFT_CSR_TILE, ABFT_COO_TILE, ABFT_PANEL_ROWS,
// ABFT_CFG_SWEEP_EPT, and the 4 * ABFT_BLOCK segments a block holds at most)
struct PlanGeometry {
  uint32_t block = 0, csr_tile = 0, coo_tile = 0, panel_rows = 0, sweep_ept = 0, max_segments = 0;
};

// ---- the knobs, as the environment gave them ------------------------------------------------------------------

// ABFT_HIP_LAYOUT as written (Other: any string that is none of the five); also, Stream .. Slice, the layout a matrix
// ended up in (COO: Stream is "grouped by output")
enum class Layout { Unset, Auto, Stream, Panels, Sweep, Slice, Other };
enum class CooPanelKernel { Panels, ProducerConsumer, Lean };

struct LayoutKnobs {
  Layout layout = Layout::Unset;
  std::optional<long> width;       // ABFT_HIP_PANEL_WIDTH: entries of the gathered vector per panel (every layout that has panels)
  std::optional<int> rpt;          // ABFT_HIP_SWEEP_RPT: 2, 4, 8, 16 (16 not in constraints mode); anything else is ignored
  std::optional<long> slice_rows;  // ABFT_HIP_SLICE_ROWS: a power of two 16 .. 2048; anything else is ignored
  std::optional<long> sweep_lag, slice_lag, panel_lag;  // ABFT_HIP_SWEEP_LAG / _SLICE_LAG / _PANEL_LAG
  std::optional<long> chunk, grid;                      // ABFT_HIP_PANEL_CHUNK / _PANEL_GRID
  long xpf = 0;                    // ABFT_HIP_PANEL_XPF
  bool compact = true, packed = true;       // ABFT_HIP_COMPACT_COLS=0 / ABFT_HIP_PACKED=0 turn them off
  std::optional<bool> packed_fast;          // ABFT_HIP_PACKED_FAST=0|1 (unset: the caller's default, ABFT_PACKED_FAST_DEFAULT)
  bool coo_pc = false, coo_lean = false;    // ABFT_HIP_COO_PC / ABFT_HIP_COO_LEAN set and not "0"
  bool panel_debug = false, sweep_debug = false;  // ABFT_HIP_PANEL_DEBUG / ABFT_HIP_SWEEP_DEBUG set
};

// the knobs as `get(name)` has them (a variable's text, or NULL: unset) -- the one place their names and spellings live
template <typename Lookup>
static inline LayoutKnobs read_knobs(Lookup get) {
  LayoutKnobs k;
  auto num = [&](const char *name) -> std::optional<long> {
    const char *e = get(name);
    return e ? std::optional<long>(atol(e)) : std::nullopt;
  };
  auto on = [&](const char *name) {  // set, and not "0"
    const char *e = get(name);
    return e && strcmp(e, "0") != 0;
  };
  auto off = [&](const char *name) {  // "0"
    const char *e = get(name);
    return e && !strcmp(e, "0");
  };
  if (const char *e = get("ABFT_HIP_LAYOUT"))
    k.layout = !strcmp(e, "auto") ? Layout::Auto : !strcmp(e, "stream") ? Layout::Stream : !strcmp(e, "panels") ? Layout::Panels
             : !strcmp(e, "sweep") ? Layout::Sweep : !strcmp(e, "slice") ? Layout::Slice : Layout::Other;
  k.width = num("ABFT_HIP_PANEL_WIDTH");
  if (const char *e = get("ABFT_HIP_SWEEP_RPT")) k.rpt = atoi(e);
  k.slice_rows = num("ABFT_HIP_SLICE_ROWS");
  k.sweep_lag = num("ABFT_HIP_SWEEP_LAG");
  k.slice_lag = num("ABFT_HIP_SLICE_LAG");
  k.panel_lag = num("ABFT_HIP_PANEL_LAG");
  k.chunk = num("ABFT_HIP_PANEL_CHUNK");
  k.grid = num("ABFT_HIP_PANEL_GRID");
  k.xpf = num("ABFT_HIP_PANEL_XPF").value_or(0L);
  k.compact = !off("ABFT_HIP_COMPACT_COLS");
  k.packed = !off("ABFT_HIP_PACKED");
  if (get("ABFT_HIP_PACKED_FAST")) k.packed_fast = !off("ABFT_HIP_PACKED_FAST");
  k.coo_pc = on("ABFT_HIP_COO_PC");
  k.coo_lean = on("ABFT_HIP_COO_LEAN");
  k.panel_debug = get("ABFT_HIP_PANEL_DEBUG") != nullptr;
  k.sweep_debug = get("ABFT_HIP_SWEEP_DEBUG") != nullptr;
  return k;
}

static inline uint32_t knob_u32(const std::optional<long> &v, long floor, uint32_t unset) {
  return v ? (uint32_t)std::max(floor, *v) : unset;
}

// Which layouts a create may try, and which of them it takes even where the size gates say it does not pay
// ("forced").  They are tried in the order slice, sweep, panels; the first that accepts the matrix wins; none: the
// streaming layout (COO: grouped by output).
//
//   ABFT_HIP_LAYOUT   | CSR, modes but constraints      | CSR, constraints       | COO, every mode
//   ------------------+---------------------------------+------------------------+-----------------
//   unset, auto       | sweep auto, panels auto         | sweep auto             | panels auto
//   stream            | -                               | -                      | -
//   panels            | panels forced                   | -                      | panels forced
//   sweep             | sweep forced, panels forced     | sweep forced           | panels forced
//   slice             | slice, panels auto              | -                      | panels auto
//   any other string  | panels auto                     | -                      | panels auto
//   (create_csr_stream: nothing is tried, whatever the variable says)
//
// So: `sweep` falls back to forced panels where the sweep planner declines (one-byte counts); `slice` is opt-in only,
// never in constraints mode, and leaves panels on auto; a CSR matrix in constraints mode never takes panels (that
// kernel has no check across a panel boundary); COO knows panels only, in constraints mode too (its checks go through
// a table of stored positions, whatever the layout).
struct LayoutTrial { bool tried = false, forced = false; };
struct LayoutPolicy { LayoutTrial slice, sweep, panels; };

static inline LayoutPolicy layout_policy(Layout choice, bool coo, bool constraints, bool force_stream) {
  LayoutPolicy p;
  if (force_stream || choice == Layout::Stream) return p;
  const bool csr = !coo;
  p.slice.tried = p.slice.forced = csr && choice == Layout::Slice && !constraints;
  p.sweep.tried = csr && (choice == Layout::Unset || choice == Layout::Auto || choice == Layout::Sweep);
  p.sweep.forced = p.sweep.tried && choice == Layout::Sweep;
  p.panels.tried = coo || !constraints;
  p.panels.forced = p.panels.tried && (choice == Layout::Panels || choice == Layout::Sweep);
  return p;
}

// what abft_hip_matrix_info reports
static inline int layout_number(Layout l) { return l == Layout::Slice ? 3 : l == Layout::Sweep ? 2 : l == Layout::Panels ? 1 : 0; }
static inline const char *layout_name(Layout l) {
  return l == Layout::Slice ? "slice" : l == Layout::Sweep ? "sweep" : l == Layout::Panels ? "panel" : "stream";
}

// ---- row pointers, row blocks ------------------------------------------------------------------------------------

// row pointers exactly as the reference builds them (CSR/CPUContext.cpp:24-41) from row indices that ascend;
// trailing empty rows get nnz (the reference leaves them uninitialised)
static inline std::vector<uint32_t> build_rowptr(const uint32_t *rows, int n_out, int nnz) {
  std::vector<uint32_t> rowptr((size_t)n_out + 1);
  uint32_t next = 0;
  for (int i = 0; i < nnz; i++)
    while (next <= rows[i]) rowptr[next++] = (uint32_t)i;
  while (next <= (uint32_t)n_out) rowptr[next++] = (uint32_t)nnz;
  return rowptr;
}

// Cut [0, n) into blocks of whole segments whose elements fit one LDS tile.
// `align2`: the tile starts at the even element at or below the block's first
// element (CSR pair loads), so that one counts against the capacity too.
static inline void cut_blocks(const PlanGeometry &geo, const uint32_t *ptr, uint32_t n, uint32_t tile, bool align2,
                              std::vector<Blk> &blk) {
  blk.clear();
  uint32_t s = 0;
  while (s < n) {
    const uint32_t base = align2 ? (ptr[s] & ~1u) : ptr[s];
    uint32_t e = s;
    while (e < n && e - s < geo.max_segments && ptr[e + 1] >= ptr[e] && ptr[e + 1] - base <= tile) e++;
    if (e == s) e = s + 1;  // a single segment longer than a tile: walked tile by tile
    blk.push_back(Blk{s, e, ptr[s], ptr[e]});
    s = e;
  }
}

// Flag the CSR row blocks whose rows all have the same length -- bit 31 of the end row:
// the kernel then derives each row's range from the block descriptor alone and never reads
// the row pointers (banded matrices: nearly every block; measured 151 -> 138 us on config
// 2's SpMV, 143 -> 134 us in secded; the same shortcut in the COO kernel was 4 % slower).
static inline void flag_uniform_blocks(const PlanGeometry &geo, const uint32_t *ptr, uint32_t tile, std::vector<Blk> &blk) {
  for (Blk &b : blk) {
    const uint32_t nseg = b.y - b.x;
    if (nseg < 2 || b.w - b.z > tile || nseg > geo.block) continue;
    const uint32_t len = ptr[b.x + 1] - ptr[b.x];
    bool same = len > 0 && (b.w - b.z) == len * nseg;
    for (uint32_t r = b.x; same && r < b.y; r++) same = ptr[r + 1] - ptr[r] == len;
    if (same) b.y |= 0x80000000u;
  }
}

// the block holding element `pos`: the last one starting at or before it (an empty block that starts at pos comes
// before the one holding pos); -1: none
static inline ptrdiff_t block_holding(const std::vector<Blk> &blk, uint32_t pos) {
  auto it = std::upper_bound(blk.begin(), blk.end(), pos, [](uint32_t p, const Blk &d) { return p < d.z; });
  if (it == blk.begin()) return -1;
  const ptrdiff_t b = (it - blk.begin()) - 1;
  return pos < blk[(size_t)b].w ? b : -1;
}

// a block the streaming SpMV stages as one tile (the others it walks tile by tile, reading cols and vals)
static inline bool one_tile(const PlanGeometry &geo, uint32_t e0, uint32_t e1) { return e1 >= e0 && e1 - (e0 & ~1u) <= geo.csr_tile; }

// ---- compact columns (mode none, streaming layout; see CsrCompact) -----------------------------------------------

// A block the SpMV stages as one tile whose columns span at most 65536 values gets its smallest column as base
// and every column as a 16-bit offset from it; every other block stays wide.  Config 2: a block
// of ~204 rows of the 3162-wide band spans ~6 530 columns.
struct CompactBuild {
  bool any = false;
  std::vector<uint32_t> cbase;  // per block: the base, or ABFT_CBASE_WIDE
  std::vector<uint16_t> c16;    // padded + 2: the kernel's 8-byte load at the last even index reads 2 past cols' padding
};

static inline void plan_compact_cols(const PlanGeometry &geo, const uint32_t *columns, const std::vector<Blk> &blk,
                                     size_t padded, CompactBuild &cb) {
  cb.cbase.assign(blk.size(), ABFT_CBASE_WIDE);
  cb.c16.assign(padded + 2, 0);
  cb.any = false;
  for (size_t b = 0; b < blk.size(); b++) {
    const uint32_t e0 = blk[b].z, e1 = blk[b].w;
    if (!one_tile(geo, e0, e1)) continue;
    uint32_t lo = 0, hi = 0;
    if (e1 > e0) lo = hi = columns[e0];
    for (uint32_t i = e0; i < e1; i++) {
      lo = std::min(lo, columns[i]);
      hi = std::max(hi, columns[i]);
    }
    if (hi - lo > 0xFFFFu) continue;
    cb.cbase[b] = lo;
    for (uint32_t i = e0; i < e1; i++) cb.c16[i] = (uint16_t)(columns[i] - lo);
    cb.any = true;
  }
}

// an element of a compact block got the column `col`: its new offset, or false -- the block goes wide
// (a column below the base wraps to a large offset)
static inline bool compact_offset(uint32_t base, uint32_t col, uint16_t &off) {
  const uint32_t d = col - base;
  off = (uint16_t)d;
  return d <= 0xFFFFu;
}

// ---- packed codes (mode none, streaming layout; see CsrPacked) ---------------------------------------------------

typedef std::array<uint64_t, ABFT_PAL_ENTRIES> Palette;

// The one planner of a packed block, at create and after an inject.  Elements [e0, e1) with columns c[] and value
// bits v[] (indexed from e0): true if the block packs, with its base, shift, padded palette (value patterns ascending,
// zeros behind) and codes[0, e1 - e0).  A block that packs is one the SpMV stages as one tile (as for compact
// columns) with at most 16 distinct value patterns whose column span fits the bits left over.
static inline bool plan_packed_block(const PlanGeometry &geo, uint32_t e0, uint32_t e1, const uint32_t *c, const uint64_t *v,
                                     uint32_t &cbase, uint32_t &shift, Palette &pal, uint16_t *codes) {
  if (!one_tile(geo, e0, e1)) return false;  // walked tile by tile
  const uint32_t n = e1 - e0;
  uint32_t nv = 0, lo = n ? c[0] : 0u, hi = lo;
  pal.fill(0);
  for (uint32_t i = 0; i < n; i++) {
    lo = std::min(lo, c[i]);
    hi = std::max(hi, c[i]);
    if (std::find(pal.begin(), pal.begin() + nv, v[i]) == pal.begin() + nv) {
      if (nv == ABFT_PAL_ENTRIES) return false;
      pal[nv++] = v[i];
    }
  }
  uint32_t k = 0;
  while ((1u << k) < nv) k++;
  shift = 16u - k;
  if (hi - lo >= (1u << shift)) return false;
  std::sort(pal.begin(), pal.begin() + nv);
  cbase = lo;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t idx = (uint32_t)(std::lower_bound(pal.begin(), pal.begin() + nv, v[i]) - pal.begin());
    codes[i] = (uint16_t)((idx << shift) | (c[i] - lo));
  }
  return true;
}

// The palettes of a matrix: the host copy of the pool, each palette's place in it by its 16 entries, and the device
// pool's capacity (entries) -- room for ABFT_PAL_SPARE palettes beyond those of create, sized once, so the pointer
// every SpMV (and any captured graph) holds never changes; a re-plan that would need more demotes its block instead.
struct PalettePool {
  std::vector<uint64_t> host;
  std::map<Palette, uint32_t> index;
  size_t cap = 0;

  // the descriptor of a packed block whose palette is `pal`: the palette's place in the pool, appended to the host
  // pool if it is new (the caller uploads host[had, size))
  Pair desc(uint32_t cbase, uint32_t shift, const Palette &pal) {
    auto it = index.find(pal);
    uint32_t no;
    if (it != index.end()) {
      no = it->second;
    } else {
      no = (uint32_t)(host.size() / ABFT_PAL_ENTRIES);
      index.emplace(pal, no);
      host.insert(host.end(), pal.begin(), pal.end());
    }
    return Pair{cbase, no << 5 | shift};
  }
  void seal(size_t spare_palettes = ABFT_PAL_SPARE) { cap = host.size() + spare_palettes * ABFT_PAL_ENTRIES; }
  bool takes(const Palette &pal) const { return index.count(pal) || host.size() + ABFT_PAL_ENTRIES <= cap; }
  void clear() { host.clear(); index.clear(); cap = 0; }
};

struct PackedBuild {
  bool any = false;
  std::vector<Pair> pdesc;      // per block {cbase, palette number << 5 | shift}; .y == 0: not packed
  std::vector<uint16_t> codes;  // padded + 2, as cols16: the kernel's loads at even indices stay inside
  std::vector<uint32_t> fast;   // per block: packed_fast_word, or 0: the general path (all 0 with the switch off)
};

// What the SpMV may skip on a packed block, proven here so that the kernel need not test it per element
// (0: nothing, the general path):
//   bit 0 (stage-fast): the block is staged as one tile; cbase + 2^shift <= n_in, so EVERY 16-bit code -- valid, stale
//     or corrupted -- decodes to a column inside the gathered vector; and the whole tile window of codes,
//     [e0 & ~1, (e0 & ~1) + csr_tile), lies inside the `codes_len` codes allocated, so the loads need no clamp.
//     The staged products of the slots outside [e0, e1) are then garbage, which no row's range reads.
//   bits 8..11 (row-fast): besides, every row has the same length 1..8 (the uniform flag, at most one row per
//     thread), kept here: thread t sums the `len` products from e0 + len * t.
// The one place the word is computed: at create, and again for a block re-planned after an inject.
#define ABFT_FAST_STAGE 1u
#define ABFT_FAST_LEN_SHIFT 8u
#define ABFT_FAST_LEN_MAX 8u
static inline uint32_t packed_fast_word(const PlanGeometry &geo, const Blk &b, Pair pd, uint32_t n_in, size_t codes_len) {
  const uint32_t e0 = b.z, e1 = b.w, shift = pd.y & 31u;
  if (pd.y == 0u || !one_tile(geo, e0, e1) || shift > 16u) return 0u;
  if ((uint64_t)pd.x + ((uint64_t)1 << shift) > (uint64_t)n_in) return 0u;
  if ((uint64_t)(e0 & ~1u) + geo.csr_tile > (uint64_t)codes_len) return 0u;
  uint32_t word = ABFT_FAST_STAGE;
  const uint32_t rows = (b.y & 0x7fffffffu) - b.x;
  if ((b.y >> 31) != 0u && rows > 0u && rows <= geo.block && (e1 - e0) % rows == 0u) {
    const uint32_t len = (e1 - e0) / rows;
    if (len >= 1u && len <= ABFT_FAST_LEN_MAX) word |= len << ABFT_FAST_LEN_SHIFT;
  }
  return word;
}

// at create: packed codes for every block that packs; the pool holds their palettes (empty if none packs)
// (`fast`: the switch; `n_in`: entries of the gathered vector)
static inline void plan_packed(const PlanGeometry &geo, const uint32_t *columns, const double *values,
                               const std::vector<Blk> &blk, size_t padded, PalettePool &pool, PackedBuild &pk,
                               bool fast = false, uint32_t n_in = 0) {
  pk.pdesc.assign(blk.size(), Pair{0u, 0u});
  pk.codes.assign(padded + 2, 0);
  pk.fast.assign(blk.size(), 0u);
  pk.any = false;
  Palette pal;
  std::vector<uint64_t> vb;
  for (size_t b = 0; b < blk.size(); b++) {
    const uint32_t e0 = blk[b].z, e1 = blk[b].w;
    if (!one_tile(geo, e0, e1)) continue;
    vb.resize(e1 - e0);
    if (e1 > e0) memcpy(vb.data(), values + e0, (size_t)(e1 - e0) * 8);
    uint32_t cbase, shift;
    if (!plan_packed_block(geo, e0, e1, columns + e0, vb.data(), cbase, shift, pal, pk.codes.data() + e0)) continue;
    pk.pdesc[b] = pool.desc(cbase, shift, pal);
    if (fast) pk.fast[b] = packed_fast_word(geo, blk[b], pk.pdesc[b], n_in, pk.codes.size());
    pk.any = true;
  }
  if (pk.any) pool.seal(); else pool.clear();
}

// after a change inside packed block [e0, e1), from the words the SpMV would otherwise read: its new descriptor and
// codes[0, e1 - e0) -- packed anew, or {0, 0}: demoted (it does not pack any more, or its palette is new and the
// pool is full), left to the compact / wide path
static inline Pair replan_packed_block(const PlanGeometry &geo, PalettePool &pool, uint32_t e0, uint32_t e1, const uint32_t *c,
                                       const uint64_t *v, uint16_t *codes) {
  uint32_t cbase, shift;
  Palette pal;
  if (plan_packed_block(geo, e0, e1, c, v, cbase, shift, pal, codes) && pool.takes(pal)) return pool.desc(cbase, shift, pal);
  return Pair{0u, 0u};
}

// ---- panel layout ------------------------------------------------------------------------------------------------

struct PanelBuild {
  uint32_t ngroups = 0, npanels = 0, width = 0;
  std::vector<uint32_t> seg_base;  // nseg + 1
  std::vector<uint16_t> seg_ptr;   // nseg * (panel_rows + 1)
  std::vector<uint32_t> pos, orig; // caller's index -> storage position and back
};

// Decide whether the panel layout pays for this matrix and, if so, build it.
// `out_idx` / `in_idx` are the element's output index and gather index (CSR: row /
// column; COO: column / row).  It pays when the input vector is much larger than
// an XCD's L2 and an output group reaches into several panels (scattered gather
// indices); banded matrices keep the streaming layout, whose x window already
// lives in L2.  Needs the gather indices of one output to be non-decreasing in
// the caller's order (as the reference loader delivers them): panels are swept
// in ascending order, so an output's additions then happen in the caller's order.
// `force`: the size gates are skipped.  knobs.width (entries) overrides the panel width.
static inline bool plan_panels(const PlanGeometry &geo, const LayoutKnobs &knobs, bool force, const uint32_t *in_idx,
                               const uint32_t *out_idx, int n_out, int n_in, int nnz, PanelBuild &pb) {
  if (nnz <= 0 || n_out <= 0) return false;
  const uint32_t R = geo.panel_rows;
  const uint32_t width = knob_u32(knobs.width, 1L, 1u << 18);  // 2 MB of x per panel; two panels per launch (PanelLaunch::chunk)
  if (!force && (size_t)n_in * sizeof(double) <= (size_t)8 << 20) return false;
  const uint64_t ngroups = ((uint64_t)n_out + R - 1) / R;
  const uint64_t npanels = ((uint64_t)n_in + width - 1) / width;
  const uint64_t nseg = ngroups * npanels;
  if (nseg == 0 || nseg > ((uint64_t)1 << 27)) return false;
  // the per-segment offset tables (2 bytes per output and segment) must stay small next to the matrix itself
  if (!force && nseg * (R + 1) * sizeof(uint16_t) > (uint64_t)nnz * 3u) return false;
  {
    std::vector<uint32_t> last((size_t)n_out, 0);
    for (int i = 0; i < nnz; i++) {
      if (in_idx[i] < last[out_idx[i]]) return false;  // would reorder an output's additions
      last[out_idx[i]] = in_idx[i];
    }
  }
  auto segment = [&](int i) {
    return (uint64_t)(out_idx[i] / R) * npanels + std::min<uint64_t>(in_idx[i] / width, npanels - 1);
  };
  pb.ngroups = (uint32_t)ngroups; pb.npanels = (uint32_t)npanels; pb.width = width;
  pb.seg_base.assign(nseg + 1, 0);
  for (int i = 0; i < nnz; i++) pb.seg_base[segment(i) + 1]++;
  uint64_t nonempty = 0;
  for (uint64_t sgm = 0; sgm < nseg; sgm++) {
    if (pb.seg_base[sgm + 1] > 65535u) return false;  // 16-bit offsets inside a segment
    nonempty += pb.seg_base[sgm + 1] != 0;
  }
  if (!force && nonempty < 3 * ngroups) return false;  // an output group stays within a panel or two: banded
  for (uint64_t sgm = 0; sgm < nseg; sgm++) pb.seg_base[sgm + 1] += pb.seg_base[sgm];
  // per segment: offsets of each of its panel_rows outputs (elements of one output contiguous)
  pb.seg_ptr.assign(nseg * (R + 1), 0);
  for (int i = 0; i < nnz; i++) pb.seg_ptr[segment(i) * (R + 1) + out_idx[i] % R + 1]++;
  for (uint64_t sgm = 0; sgm < nseg; sgm++) {
    uint16_t *p = pb.seg_ptr.data() + sgm * (R + 1);
    for (uint32_t r = 0; r < R; r++) p[r + 1] = (uint16_t)(p[r + 1] + p[r]);
  }
  // place: segment base + output's offset + arrival order within (segment, output)
  pb.pos.resize((size_t)nnz);
  pb.orig.resize((size_t)nnz);
  std::vector<uint16_t> cursor(nseg * R, 0);
  for (int i = 0; i < nnz; i++) {
    const uint64_t sgm = segment(i);
    const uint32_t lo = out_idx[i] % R;
    const uint32_t p = pb.seg_base[sgm] + pb.seg_ptr[sgm * (R + 1) + lo] + cursor[sgm * R + lo]++;
    pb.pos[i] = p;
    pb.orig[p] = (uint32_t)i;
  }
  return true;
}

// ---- sweep layout ------------------------------------------------------------------------------------------------

struct SweepBuild {
  uint32_t ngroups = 0, npanels = 0, width = 0;
  int rpt = 8;
  std::vector<uint32_t> wbase;     // nseg * 4 + 1
  std::vector<uint8_t> counts;     // [segment][thread][j]
  std::vector<uint32_t> pos, orig; // caller's index -> storage position and back
};

// Same decision as plan_panels (scattered columns over a vector much larger than an XCD's
// L2; a row's columns non-decreasing in the caller's order), then the sweep layout's arrays
// (CSR: the caller's order is row-major).  `capacity(rpt)`: workgroups of the kernel variant
// with `rpt` rows per thread that can be resident at once.  `force`: the size gates are skipped;
// knobs.width / knobs.rpt override the geometry.
// (constraints mode too, round 3: the kernel stages the columns and runs the reference's checks in the
// summing phase; round 2 sent that mode to the streaming layout, 2.5 x every other mode on config 4)
template <typename Cap>
static inline bool plan_sweep(const PlanGeometry &geo, const LayoutKnobs &knobs, bool force, bool constraints,
                              const uint32_t *cols, const uint32_t *rows, int n_out, int n_in, int nnz, Cap capacity,
                              SweepBuild &sb) {
  if (nnz <= 0 || n_out <= 0) return false;
  if (!force && (size_t)n_in * sizeof(double) <= (size_t)8 << 20) return false;
  // rows per thread: the group size that keeps the most workgroups per CU busy (up to 4: more did
  // not help), then the fewest rounds, then the smallest groups
  {
    double best = -1.0;
    uint64_t best_rounds = 0;
    for (int rpt : {2, 4, 8, 16}) {  // (1 row per thread, 8 workgroups per CU: 169 vs 128 us on config 4's 1/8 shard)
      if (rpt == 16 && constraints) continue;  // (its per-row check state does not fit 128 registers there)
      const uint64_t groups = ((uint64_t)n_out + 256u * rpt - 1) / (256u * rpt), cap = std::max<uint64_t>(capacity(rpt), 1);
      const uint64_t rounds = (groups + cap - 1) / cap;
      const double per_cu = std::min(4.0, (double)((groups + rounds - 1) / rounds) / 256.0);
      if (per_cu > best + 1e-9 || (per_cu > best - 1e-9 && rounds < best_rounds)) {
        best = per_cu; best_rounds = rounds; sb.rpt = rpt;
      }
    }
  }
  if (knobs.rpt) {
    const int v = *knobs.rpt;
    if (v == 2 || v == 4 || v == 8 || (v == 16 && !constraints)) sb.rpt = v;
  }
  // entries of the gathered vector per panel: about 1 MB of it (2 MB: 757 vs 743 us on config 4) unless that
  // leaves a segment well under two tiles on average -- the 1/8 row shard of config 4 that one rank
  // of an 8-GPU job multiplies: 161 us with 1 MB panels, 134 us with 2 MB ones
  // Inside that range the width is set so that the average segment just fills a whole number of
  // tiles: every tile costs its full load phase, so a segment of 1.6 tiles pays for 2 (config 4,
  // 16 rows per thread: 3 277 elements per segment at 2^17 entries, 724 us; 4 000 at 164 000 entries
  // -- two tiles less 1.5 standard deviations -- 681 us; 4 300, where most segments spill into a third
  // tile, 737 us; `gpurun_out/r2/width_ab2.log`)
  uint32_t width = 1u << 17;
  {
    const uint64_t groups = ((uint64_t)n_out + 256u * sb.rpt - 1) / (256u * sb.rpt);
    const double tile = 256.0 * (sb.rpt <= 4 ? 4.0 : (double)geo.sweep_ept);
    const double per_entry = (double)nnz / ((double)groups * (double)n_in);  // elements of a segment per entry of x
    if ((double)width * per_entry * 2.0 < 3.0 * tile) width = 1u << 18;
    for (int k = 1; k <= 8; k++) {
      const double w = (k * tile - 1.5 * std::sqrt(k * tile)) / per_entry;
      if (w < 0.92 * (double)(1u << 17)) continue;
      if (w <= 1.25 * (double)(1u << 18)) width = (uint32_t)w & ~15u;
      break;
    }
  }
  width = knob_u32(knobs.width, 1L, width);
  const uint64_t npanels = ((uint64_t)n_in + width - 1) / width;
  if (npanels == 0 || (uint64_t)n_out * npanels > ((uint64_t)1 << 31)) return false;
  // one count per (row, panel) must stay small next to the matrix itself
  if (!force && (uint64_t)n_out * npanels > (uint64_t)nnz * 3u) return false;
  auto panel_of = [&](int i) { return std::min<uint64_t>(cols[i] / width, npanels - 1); };
  for (int i = 1; i < nnz; i++)
    if (rows[i] == rows[i - 1] && cols[i] < cols[i - 1]) return false;  // would reorder a row's additions
  std::vector<uint8_t> rc((size_t)n_out * npanels, 0);  // elements per (row, panel)
  for (int i = 0; i < nnz; i++) {
    uint8_t &c = rc[(size_t)rows[i] * npanels + panel_of(i)];
    if (c == 255u) return false;  // one-byte counts: such a matrix keeps the panel layout
    c++;
  }
  if (!force) {  // a row group that stays within a panel or two is banded: streaming layout
    const uint64_t g2k = ((uint64_t)n_out + 2047) / 2048;
    uint64_t nonempty = 0;
    std::vector<char> seen(npanels);
    for (uint64_t g = 0; g < g2k; g++) {
      std::fill(seen.begin(), seen.end(), 0);
      const uint64_t r1 = std::min<uint64_t>((g + 1) * 2048, (uint64_t)n_out);
      for (uint64_t r = g * 2048; r < r1; r++)
        for (uint64_t c = 0; c < npanels; c++) seen[c] |= rc[r * npanels + c] != 0;
      for (uint64_t c = 0; c < npanels; c++) nonempty += seen[c];
    }
    if (nonempty < 3 * g2k) return false;
  }
  const uint32_t G = 256u * (uint32_t)sb.rpt, WR = 64u * (uint32_t)sb.rpt;
  const uint64_t ngroups = ((uint64_t)n_out + G - 1) / G, nseg = ngroups * npanels;
  if (nseg > ((uint64_t)1 << 26)) return false;
  sb.ngroups = (uint32_t)ngroups; sb.npanels = (uint32_t)npanels; sb.width = width;
  // element ranges: per (segment, wave) base, per (segment, thread, j) count
  sb.wbase.assign(nseg * 4 + 1, 0);
  sb.counts.assign((size_t)nseg * 256u * sb.rpt + 16, 0);
  uint64_t run = 0;
  for (uint64_t g = 0; g < ngroups; g++)
    for (uint64_t c = 0; c < npanels; c++) {
      const uint64_t seg = g * npanels + c;
      for (uint32_t w = 0; w < 4; w++) {
        sb.wbase[seg * 4 + w] = (uint32_t)run;
        for (uint32_t j = 0; j < (uint32_t)sb.rpt; j++)
          for (uint32_t l = 0; l < 64; l++) {
            const uint64_t row = g * G + w * WR + j * 64 + l;
            const uint32_t k = row < (uint64_t)n_out ? rc[row * npanels + c] : 0u;
            sb.counts[(seg * 256u + w * 64u + l) * sb.rpt + j] = (uint8_t)k;
            run += k;
          }
      }
    }
  sb.wbase[nseg * 4] = (uint32_t)run;
  // placement: rows ascending, a row's elements in the caller's order.  Inside a segment the
  // rows follow the ownership order (wave, j, lane) = ascending local index, so filling the
  // segments in row order lands every element at its place.
  sb.pos.resize((size_t)nnz);
  sb.orig.resize((size_t)nnz);
  std::vector<uint32_t> fill(nseg, 0);
  for (int i = 0; i < nnz; i++) {
    const uint64_t seg = (uint64_t)(rows[i] / G) * npanels + panel_of(i);
    const uint32_t p = sb.wbase[seg * 4] + fill[seg]++;
    sb.pos[i] = p;
    sb.orig[p] = (uint32_t)i;
  }
  return true;
}

// ---- slice layout ------------------------------------------------------------------------------------------------

struct SliceBuild {
  uint32_t nslices = 0, npanels = 0, width = 0, rows_log2 = 0;
  std::vector<uint32_t> sub;       // nslices * (npanels + 1)
  std::vector<uint16_t> rid;       // per stored element
  std::vector<uint32_t> pos, orig; // caller's index -> storage position and back
};

// The slice layout's arrays (see SliceLayout).  Opt-in only: measured slower than the sweep layout on config 4 and
// on its 1/8 shard, kept for A/B runs and because it has no limit on the elements of one row
// in one panel.  Needs a row's columns non-decreasing in the caller's order (panels ascend).  `waves(rows_log2)`:
// waves of the kernel resident at once with slices of that many rows.  knobs.width / knobs.slice_rows override the
// geometry.
template <typename Cap>
static inline bool plan_slice(const LayoutKnobs &knobs, const uint32_t *cols, const uint32_t *rows, int n_out, int n_in,
                              int nnz, Cap waves, SliceBuild &sb) {
  if (nnz <= 0 || n_out <= 0) return false;
  for (int i = 1; i < nnz; i++)
    if (rows[i] == rows[i - 1] && cols[i] < cols[i - 1]) return false;  // would reorder a row's additions
  // rows per slice: the smallest power of two (64..1024) with which every slice has a wave of its
  // own at once; beyond that, 512 and several rounds
  uint32_t lg = 6;
  while (lg < 10 && ((uint64_t)n_out + (1u << lg) - 1) >> lg > waves(lg)) lg++;
  if (((uint64_t)n_out + (1u << lg) - 1) >> lg > waves(lg)) lg = 9;
  if (knobs.slice_rows)
    for (uint32_t k = 4; k <= 11; k++)
      if (*knobs.slice_rows == (1L << k)) lg = k;
  const uint32_t width = knob_u32(knobs.width, 1L, 1u << 17);  // entries of the gathered vector per panel (1 MB of it)
  const uint64_t npanels = ((uint64_t)n_in + width - 1) / width;
  const uint64_t nslices = ((uint64_t)n_out + (1u << lg) - 1) >> lg;
  if (npanels == 0 || nslices * (npanels + 1) > ((uint64_t)1 << 28)) return false;
  sb.nslices = (uint32_t)nslices; sb.npanels = (uint32_t)npanels; sb.width = width; sb.rows_log2 = lg;
  auto panel_of = [&](int i) { return std::min<uint64_t>(cols[i] / width, npanels - 1); };
  sb.sub.assign(nslices * (npanels + 1), 0);
  // counts per (slice, panel) into sub[s][c + 1] ... then running bases
  std::vector<uint32_t> cnt(nslices * npanels, 0);
  for (int i = 0; i < nnz; i++) cnt[(uint64_t)(rows[i] >> lg) * npanels + panel_of(i)]++;
  uint32_t run = 0;
  for (uint64_t s = 0; s < nslices; s++) {
    for (uint64_t c = 0; c < npanels; c++) {
      sb.sub[s * (npanels + 1) + c] = run;
      run += cnt[s * npanels + c];
    }
    sb.sub[s * (npanels + 1) + npanels] = run;
  }
  // placement in the caller's order: inside a (slice, panel) run rows ascend and a row's elements keep their order
  sb.pos.resize((size_t)nnz);
  sb.orig.resize((size_t)nnz);
  sb.rid.assign((size_t)nnz + 2, 0);
  std::fill(cnt.begin(), cnt.end(), 0);
  for (int i = 0; i < nnz; i++) {
    const uint64_t s = rows[i] >> lg, c = panel_of(i);
    const uint32_t p = sb.sub[s * (npanels + 1) + c] + cnt[s * npanels + c]++;
    sb.pos[i] = p;
    sb.orig[p] = (uint32_t)i;
    sb.rid[p] = (uint16_t)(rows[i] - (uint32_t)(s << lg) + 1u);  // 0 = no element (what a load past the end returns)
  }
  return true;
}

// ---- a whole CSR matrix ------------------------------------------------------------------------------------------

struct CsrPlan {
  Layout layout = Layout::Stream;
  size_t padded = 0;  // elements cols / vals are allocated for: even, >= nnz + 2
  std::vector<uint32_t> rowptr;
  std::vector<Blk> blk;
  SliceBuild slice;
  SweepBuild sweep;
  PanelBuild panels;
  CompactBuild compact;  // streaming layout, mode none
  PackedBuild packed;    // ... (its palettes go to the caller's pool)
  // caller's index -> storage position and back (not on the streaming layout, which stores in the caller's order)
  const std::vector<uint32_t> &pos() const { return layout == Layout::Slice ? slice.pos : layout == Layout::Sweep ? sweep.pos : panels.pos; }
  const std::vector<uint32_t> &orig() const { return layout == Layout::Slice ? slice.orig : layout == Layout::Sweep ? sweep.orig : panels.orig; }
};

// Rows ascending (abft_hip.hip has checked it).  `mode_none`: the mode that reads compact columns and packed codes;
// `slice_waves(rows_log2)` / `sweep_cap(rpt)`: what of those kernels is resident at once.
template <typename SliceCap, typename SweepCap>
static inline void plan_csr(const PlanGeometry &geo, const LayoutKnobs &knobs, bool mode_none, bool constraints, bool force_stream,
                            const uint32_t *columns, const uint32_t *rows, const double *values, int n_out, int n_in, int nnz,
                            SliceCap slice_waves, SweepCap sweep_cap, PalettePool &pool, CsrPlan &plan) {
  plan.rowptr = build_rowptr(rows, n_out, nnz);
  cut_blocks(geo, plan.rowptr.data(), (uint32_t)n_out, geo.csr_tile, true, plan.blk);
  flag_uniform_blocks(geo, plan.rowptr.data(), geo.csr_tile, plan.blk);
  plan.padded = ((size_t)nnz + 3) & ~(size_t)1;
  const LayoutPolicy may = layout_policy(knobs.layout, false, constraints, force_stream);
  plan.layout = Layout::Stream;
  if (may.slice.tried && plan_slice(knobs, columns, rows, n_out, n_in, nnz, slice_waves, plan.slice))
    plan.layout = Layout::Slice;
  else if (may.sweep.tried &&
           plan_sweep(geo, knobs, may.sweep.forced, constraints, columns, rows, n_out, n_in, nnz, sweep_cap, plan.sweep))
    plan.layout = Layout::Sweep;
  else if (may.panels.tried && plan_panels(geo, knobs, may.panels.forced, columns, rows, n_out, n_in, nnz, plan.panels))
    plan.layout = Layout::Panels;
  if (plan.layout != Layout::Stream || !mode_none) return;
  if (knobs.compact) plan_compact_cols(geo, columns, plan.blk, plan.padded, plan.compact);
  if (knobs.packed)  // (the fast words: only where the caller has set the switch; unset is off here)
    plan_packed(geo, columns, values, plan.blk, plan.padded, pool, plan.packed, knobs.packed_fast.value_or(false), (uint32_t)n_in);
}

// ---- a whole COO matrix ------------------------------------------------------------------------------------------

struct CooPlan {
  Layout layout = Layout::Stream;    // Stream: grouped by output; Panels
  std::vector<uint32_t> grp;         // n_out + 1: first element of every output
  std::vector<uint32_t> pos, orig;   // caller's index -> storage position and back (at least one entry)
  std::vector<Blk> blk;
  PanelBuild panels;
  std::vector<Pair> as_created;      // constraints mode: nnz + 1
};

// Group by output index (col), stable in the caller's order: result[col] is then summed in the order the reference's
// serial scatter adds into it (COO/CPUContext.cpp:111-120) -- or (output group, row panel) segments when the gathered
// vector is far larger than L2 and the row indices are scattered (gather index = row, output = column).
static inline void plan_coo(const PlanGeometry &geo, const LayoutKnobs &knobs, bool constraints, const uint32_t *columns,
                            const uint32_t *rows, int n_out, int n_in, int nnz, CooPlan &plan) {
  plan.grp.assign((size_t)n_out + 1, 0);
  for (int i = 0; i < nnz; i++) plan.grp[columns[i] + 1]++;
  for (int c = 0; c < n_out; c++) plan.grp[c + 1] += plan.grp[c];
  const LayoutPolicy may = layout_policy(knobs.layout, true, constraints, false);
  const bool panels = may.panels.tried && plan_panels(geo, knobs, may.panels.forced, rows, columns, n_out, n_in, nnz, plan.panels);
  plan.layout = panels ? Layout::Panels : Layout::Stream;
  plan.orig.assign((size_t)std::max(nnz, 1), 0);
  plan.pos.assign((size_t)std::max(nnz, 1), 0);
  std::vector<uint32_t> fill(plan.grp.begin(), plan.grp.end() - 1);
  for (int i = 0; i < nnz; i++) {
    const uint32_t p = panels ? plan.panels.pos[i] : fill[columns[i]]++;
    plan.orig[p] = (uint32_t)i;
    plan.pos[i] = p;
  }
  cut_blocks(geo, plan.grp.data(), (uint32_t)n_out, geo.coo_tile, false, plan.blk);
  if (!constraints) return;
  // {col,row} of every stored element as it is now (kernels.hip, coo_constraints_cold); the complement for an
  // element that fails the reference's checks already (COO/CPUContext.cpp:155-188), which is then checked on
  // every pass.  (One entry more than elements: lanes past a tile's end read the entry of its first position,
  // which for an empty tile at the end of the matrix is position nnz.)
  plan.as_created.assign((size_t)nnz + 1, Pair{0u, 0u});
  for (int i = 0; i < nnz; i++) {
    bool fails = rows[i] >= (uint32_t)n_in || columns[i] >= (uint32_t)n_out;
    if (!fails && i + 1 < nnz) fails = rows[i] > rows[i + 1] || (rows[i] == rows[i + 1] && columns[i] >= columns[i + 1]);
    plan.as_created[plan.pos[i]] = fails ? Pair{~columns[i], ~rows[i]} : Pair{columns[i], rows[i]};
  }
}

// ---- launch geometry ---------------------------------------------------------------------------------------------

// sweep: all groups resident if they fit; else equal rounds
static inline uint32_t sweep_grid(uint32_t ngroups, uint32_t capacity) {
  const uint32_t rounds = (ngroups + capacity - 1) / capacity;
  return (ngroups + rounds - 1) / rounds;
}

// slice (four slices, one per wave, to a workgroup): all slices resident if they fit; else equal rounds
static inline uint32_t slice_grid(uint32_t nslices, uint32_t waves) {
  const uint32_t groups = (nslices + 3u) / 4u, cap = std::max(waves / 4u, 1u);
  const uint32_t rounds = (groups + cap - 1) / cap;
  return (groups + rounds - 1) / rounds;
}

// How a matrix in the panel layout is launched.  `first_cap`: workgroups the launch is capped at when every panel
// runs in one unpaced launch (CSR: the kernel's resident workgroups; COO: 8 per CU); `resident(kernel)`: resident
// workgroups of a COO panel kernel.
struct PanelLaunch {
  uint32_t grid = 0;   // workgroups
  uint32_t chunk = 0;  // panels per launch (0 = all)
  uint32_t lag = 0;    // COO: > 0: one launch, paced by a progress board per XCD (the caller allocates it)
  CooPanelKernel kernel = CooPanelKernel::Panels;
};

template <typename Resident>
static inline PanelLaunch panel_launch(const LayoutKnobs &knobs, bool coo, bool constraints, uint32_t n_in, uint32_t ngroups,
                                       uint32_t first_cap, Resident resident) {
  PanelLaunch L;
  L.grid = std::min<uint32_t>(ngroups, first_cap);
  // panels per launch: the kernel boundary keeps the chip in one window of x -- 4 MB (config 4's
  // 33 MB vector: 2 panels per launch were best), 8 MB where the whole vector is only a few L2s
  // large and its misses come out of the Infinity Cache anyway (config 5, 16.8 MB: 223 us with 2
  // panels per launch, 207 with 4, 210 with all 8 in one launch)
  L.chunk = knob_u32(knobs.chunk, 0L, (size_t)n_in * sizeof(double) <= ((size_t)24 << 20) ? 4u : 2u);
  if (L.chunk) L.grid = ngroups;  // one row group per workgroup between boundaries
  // COO (round 4): ALL panels in one launch, the workgroups of an XCD held inside one window of x by a progress
  // board per XCD instead of by kernel boundaries (knobs.panel_lag: panels a workgroup may be ahead of the
  // slowest of its XCD; 0 = the chunked launches above)
  // (config 5, sec7, same box, us per SpMV: two launches of 4 panels 201-202, one unpaced launch 201, paced with
  // lag 1 / 2 / 3: 207 / 195-196 / 202; panels of 1.3 MB instead of 2 MB: 223 unpaced, 198 with lag 2 --
  // gpurun_out/r4/c5_ab3.txt, c5_ab4.txt.  Default: lag 2 when every group has its own resident workgroup.)
  if (coo && !constraints)
    L.kernel = knobs.coo_pc ? CooPanelKernel::ProducerConsumer : knobs.coo_lean ? CooPanelKernel::Lean : CooPanelKernel::Panels;
  const uint32_t res = coo ? (uint32_t)resident(L.kernel) : 0u;
  L.lag = knob_u32(knobs.panel_lag, 0L, coo && ngroups <= res && !knobs.chunk ? 2u : 0u);
  if (coo && L.lag > 0) {
    L.chunk = 0;
    L.grid = std::min<uint32_t>(ngroups, std::max(res, 1u));
  } else {
    L.lag = 0;
  }
  // (tests: fewer workgroups than groups, i.e. several rounds of groups per workgroup, on small matrices)
  if (knobs.grid) L.grid = std::max<uint32_t>(1u, std::min<uint32_t>(L.grid, (uint32_t)std::max(1L, *knobs.grid)));
  return L;
}
