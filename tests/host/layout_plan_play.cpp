// layout_plan_play.cpp -- the matrix layout planner (abft_sparse_cg_amd/csrc/layout_plan.h) without a GPU: this
// program stands where abft_hip.hip's create_csr / create_coo / create_any stand, up to the first upload.
// tests/test_layout_plan_host.py builds it with AddressSanitizer and UBSan and feeds it cases on stdin
// (layout_plan_io.h has the format).  Per case it plans, prints one line -- the chosen layout, every scalar, a
// digest of every array -- and then holds the plan to what a kernel relies on when it indexes these tables
// unchecked; a broken invariant is a message on stderr and exit status 1.
#include "layout_plan_io.h"

#if !defined(ABFT_PAL_ENTRIES) || !defined(ABFT_CBASE_WIDE) || !defined(ABFT_PAL_SPARE)
#error "build with -DABFT_PAL_ENTRIES=... -DABFT_CBASE_WIDE=... -DABFT_PAL_SPARE=... as abft_internal.h and abft_hip.hip have them"
#endif
#include "layout_plan.h"

static const Case *g_case = nullptr;
#define NEED(cond, ...)                                                    \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "case %s: %s: ", g_case->name.c_str(), #cond);       \
      fprintf(stderr, __VA_ARGS__);                                        \
      fprintf(stderr, "\n");                                               \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

// ---- invariants ----------------------------------------------------------------------------------------------

static void check_permutation(const std::vector<uint32_t> &pos, const std::vector<uint32_t> &orig, int nnz) {
  NEED(pos.size() >= (size_t)nnz && orig.size() >= (size_t)nnz, "%zu %zu", pos.size(), orig.size());
  for (int i = 0; i < nnz; i++) {
    NEED(pos[i] < (uint32_t)nnz, "pos[%d] = %u", i, pos[i]);
    NEED(orig[pos[i]] == (uint32_t)i, "orig[pos[%d]] = %u", i, orig[pos[i]]);
  }
}

// within an output, stored order preserves the caller's order
static void check_order(const std::vector<uint32_t> &pos, const uint32_t *out_idx, int n_out, int nnz) {
  std::vector<int64_t> last((size_t)n_out, -1);
  for (int i = 0; i < nnz; i++) {
    NEED((int64_t)pos[i] > last[out_idx[i]], "element %d of output %u stored before its predecessor", i, out_idx[i]);
    last[out_idx[i]] = pos[i];
  }
}

static void check_blocks(const PlanGeometry &geo, const std::vector<Blk> &blk, const std::vector<uint32_t> &ptr, uint32_t n,
                         uint32_t tile, bool align2, uint32_t nnz) {
  uint32_t s = 0;
  for (const Blk &b : blk) {
    const uint32_t end = b.y & 0x7fffffffu, nseg = end - b.x;
    NEED(b.x == s && end > s && end <= n, "block [%u,%u) after %u", b.x, end, s);
    NEED(nseg <= geo.max_segments, "%u segments", nseg);
    NEED(b.z == ptr[b.x] && b.w == ptr[end] && b.z <= b.w && b.w <= nnz, "elements [%u,%u)", b.z, b.w);
    NEED(nseg == 1 || b.w - (align2 ? b.z & ~1u : b.z) <= tile, "block [%u,%u) holds %u elements", b.x, end, b.w - b.z);
    if (b.y & 0x80000000u) {
      NEED(align2 && nseg >= 2 && nseg <= geo.block && b.w - b.z <= tile, "uniform flag on [%u,%u)", b.x, end);
      for (uint32_t r = b.x; r < end; r++) NEED(ptr[r + 1] - ptr[r] == (b.w - b.z) / nseg, "row %u of a uniform block", r);
    }
    s = end;
  }
  NEED(s == n, "blocks end at %u of %u", s, n);
}

static void check_panels(const PlanGeometry &geo, const PanelBuild &pb, const std::vector<uint32_t> &pos, const uint32_t *in_idx,
                         const uint32_t *out_idx, int n_out, int n_in, int nnz) {
  const uint32_t R = geo.panel_rows;
  const uint64_t nseg = (uint64_t)pb.ngroups * pb.npanels;
  NEED(pb.width >= 1 && (uint64_t)pb.ngroups * R >= (uint64_t)n_out && (uint64_t)pb.npanels * pb.width >= (uint64_t)n_in, "geometry");
  NEED(pb.seg_base.size() == nseg + 1 && pb.seg_ptr.size() == nseg * (R + 1), "table sizes");
  NEED(pb.seg_base[0] == 0 && pb.seg_base[nseg] == (uint32_t)nnz, "bases end at %u", pb.seg_base[nseg]);
  for (uint64_t s = 0; s < nseg; s++) {
    NEED(pb.seg_base[s] <= pb.seg_base[s + 1], "segment %llu", (unsigned long long)s);
    const uint32_t len = pb.seg_base[s + 1] - pb.seg_base[s];
    const uint16_t *p = pb.seg_ptr.data() + s * (R + 1);
    NEED(len <= 65535u && p[0] == 0 && p[R] == len, "segment %llu: %u elements, offsets end at %u", (unsigned long long)s, len, p[R]);
    for (uint32_t r = 0; r < R; r++) NEED(p[r] <= p[r + 1], "segment %llu output %u", (unsigned long long)s, r);
  }
  for (int i = 0; i < nnz; i++) {
    const uint64_t s = (uint64_t)(out_idx[i] / R) * pb.npanels + std::min<uint64_t>(in_idx[i] / pb.width, pb.npanels - 1);
    const uint16_t *p = pb.seg_ptr.data() + s * (R + 1);
    const uint32_t off = pos[i] - pb.seg_base[s], lo = out_idx[i] % R;
    NEED(pos[i] >= pb.seg_base[s] && off >= p[lo] && off < p[lo + 1], "element %d outside its output's range", i);
  }
}

static void check_sweep(const SweepBuild &sb, const Matrix &M) {
  const uint32_t rpt = (uint32_t)sb.rpt, G = 256u * rpt;
  const uint64_t nseg = (uint64_t)sb.ngroups * sb.npanels;
  const int nnz = M.nnz();
  NEED(rpt == 2 || rpt == 4 || rpt == 8 || rpt == 16, "rpt %u", rpt);
  NEED((uint64_t)sb.ngroups * G >= (uint64_t)M.n_out && (uint64_t)sb.npanels * sb.width >= (uint64_t)M.n_in, "geometry");
  NEED(sb.wbase.size() == nseg * 4 + 1 && sb.counts.size() >= nseg * 256u * rpt, "table sizes");
  NEED(sb.wbase[0] == 0 && sb.wbase[nseg * 4] == (uint32_t)nnz, "bases end at %u", sb.wbase[nseg * 4]);
  for (uint64_t w = 0; w < nseg * 4; w++) {
    uint32_t sum = 0;
    for (uint32_t t = 0; t < 64u * rpt; t++) sum += sb.counts[(w / 4 * 256u + w % 4 * 64u) * rpt + t];
    NEED(sb.wbase[w] + sum == sb.wbase[w + 1], "wave %llu: %u counted, %u stored", (unsigned long long)w, sum, sb.wbase[w + 1] - sb.wbase[w]);
  }
  // every element inside its row's run: the run starts at the wave's base plus the counts of the rows owned before it
  std::vector<uint32_t> first((size_t)M.n_out * sb.npanels, 0);  // [row][panel]
  for (uint64_t seg = 0; seg < nseg; seg++)
    for (uint32_t w = 0; w < 4; w++) {
      uint32_t run = sb.wbase[seg * 4 + w];
      for (uint32_t j = 0; j < rpt; j++)
        for (uint32_t l = 0; l < 64; l++) {
          const uint64_t row = seg / sb.npanels * G + w * 64u * rpt + j * 64u + l;
          const uint32_t k = sb.counts[(seg * 256u + w * 64u + l) * rpt + j];
          NEED(row < (uint64_t)M.n_out || k == 0, "a count for row %llu", (unsigned long long)row);
          if (row < (uint64_t)M.n_out) first[row * sb.npanels + seg % sb.npanels] = run;
          run += k;
        }
    }
  for (int i = 0; i < nnz; i++) {
    const uint32_t row = M.rows[i], local = row % G, w = local / (64u * rpt), j = local % (64u * rpt) / 64u, l = local % 64u;
    const uint64_t c = std::min<uint64_t>(M.cols[i] / sb.width, sb.npanels - 1), seg = (uint64_t)(row / G) * sb.npanels + c;
    const uint32_t at = first[(size_t)row * sb.npanels + c], k = sb.counts[(seg * 256u + w * 64u + l) * rpt + j];
    NEED(sb.pos[i] >= at && sb.pos[i] < at + k, "element %d at %u outside its row's run [%u,%u)", i, sb.pos[i], at, at + k);
  }
}

static void check_slice(const SliceBuild &sb, const Matrix &M) {
  const int nnz = M.nnz();
  const uint32_t lg = sb.rows_log2;
  NEED(lg >= 4 && lg <= 11 && ((uint64_t)sb.nslices << lg) >= (uint64_t)M.n_out && (uint64_t)sb.npanels * sb.width >= (uint64_t)M.n_in, "geometry");
  NEED(sb.sub.size() == (size_t)sb.nslices * (sb.npanels + 1) && sb.rid.size() >= (size_t)nnz + 2, "table sizes");
  uint32_t run = 0;
  for (size_t k = 0; k < sb.sub.size(); k++) {
    NEED(sb.sub[k] >= run, "sub[%zu]", k);
    run = sb.sub[k];
  }
  NEED(sb.sub.empty() || (sb.sub[0] == 0 && sb.sub.back() == (uint32_t)nnz), "bases end at %u", sb.sub.back());
  for (int i = 0; i < nnz; i++) {
    const uint64_t s = M.rows[i] >> lg, c = std::min<uint64_t>(M.cols[i] / sb.width, sb.npanels - 1);
    const uint32_t p = sb.pos[i];
    NEED(p >= sb.sub[s * (sb.npanels + 1) + c] && p < sb.sub[s * (sb.npanels + 1) + c + 1], "element %d outside its run", i);
    NEED(sb.rid[p] >= 1 && (s << lg) + sb.rid[p] - 1 == M.rows[i], "rid[%u] = %u", p, sb.rid[p]);
  }
  NEED(sb.rid[(size_t)nnz] == 0 && sb.rid[(size_t)nnz + 1] == 0, "the padding names an element");
}

static uint64_t bits(double v) {
  uint64_t u;
  memcpy(&u, &v, 8);
  return u;
}

static void check_packed_block(const Blk &b, Pair d, const uint16_t *codes, const PalettePool &pool, const uint32_t *c, const uint64_t *v) {
  const uint32_t shift = d.y & 31u, pbase = (d.y >> 5) * ABFT_PAL_ENTRIES;
  NEED(shift >= 12u && shift <= 16u && (size_t)pbase + ABFT_PAL_ENTRIES <= pool.host.size(), "descriptor %u %u", d.x, d.y);
  for (uint32_t i = 0; i < b.w - b.z; i++) {
    NEED((uint32_t)(codes[i] >> shift) < ABFT_PAL_ENTRIES, "palette index");
    NEED(d.x + (codes[i] & ((1u << shift) - 1u)) == c[i] && pool.host[pbase + (codes[i] >> shift)] == v[i], "element %u of block at %u", i, b.z);
  }
}

// compact and packed codes decode to what was given; a re-plan after one element changed gives what planning the
// changed block from scratch gives; the pool stays inside its capacity and demotes when it would not
static void check_stream(const PlanGeometry &geo, const LayoutKnobs &knobs, const CsrPlan &plan, const PalettePool &pool, const Matrix &M) {
  const int nnz = M.nnz();
  std::vector<uint64_t> vb((size_t)nnz);
  for (int i = 0; i < nnz; i++) vb[i] = bits(M.vals[i]);
  NEED(plan.padded % 2 == 0 && plan.padded >= (size_t)nnz + 2, "padded %zu", plan.padded);
  if (plan.compact.any) {
    NEED(knobs.compact && plan.compact.cbase.size() == plan.blk.size() && plan.compact.c16.size() == plan.padded + 2, "compact sizes");
    for (size_t b = 0; b < plan.blk.size(); b++) {
      const Blk &B = plan.blk[b];
      uint32_t lo = ~0u, hi = 0;
      for (uint32_t i = B.z; i < B.w; i++) { lo = std::min(lo, M.cols[i]); hi = std::max(hi, M.cols[i]); }
      const bool fits = one_tile(geo, B.z, B.w) && (B.w == B.z || hi - lo <= 0xFFFFu);
      NEED((plan.compact.cbase[b] != ABFT_CBASE_WIDE) == fits, "block %zu: compact %d, fits %d", b, !fits, fits);
      if (fits)
        for (uint32_t i = B.z; i < B.w; i++) NEED(plan.compact.cbase[b] + plan.compact.c16[i] == M.cols[i], "element %u", i);
    }
  }
  if (!plan.packed.any) {
    NEED(pool.host.empty() && pool.index.empty(), "a pool with nothing packed");
    return;
  }
  NEED(knobs.packed && plan.packed.pdesc.size() == plan.blk.size() && plan.packed.codes.size() == plan.padded + 2, "packed sizes");
  NEED(pool.cap == pool.host.size() + ABFT_PAL_SPARE * ABFT_PAL_ENTRIES && pool.index.size() * ABFT_PAL_ENTRIES == pool.host.size(), "pool");
  size_t replanned = 0;
  for (size_t b = 0; b < plan.blk.size(); b++) {
    const Blk &B = plan.blk[b];
    const uint32_t n = B.w - B.z;
    std::vector<uint16_t> codes(n + 1);
    uint32_t cbase, shift;
    Palette pal;
    const bool packs = plan_packed_block(geo, B.z, B.w, M.cols.data() + B.z, vb.data() + B.z, cbase, shift, pal, codes.data());
    NEED((plan.packed.pdesc[b].y != 0u) == packs, "block %zu: packed %d, packs %d", b, !packs, packs);
    if (!packs) continue;
    check_packed_block(B, plan.packed.pdesc[b], plan.packed.codes.data() + B.z, pool, M.cols.data() + B.z, vb.data() + B.z);
    if (n == 0 || replanned >= 6) continue;
    // one element changed: its column (one up; far away) or its value (a pattern of the block; a new one)
    for (int what = 0; what < 4; what++) {
      replanned++;
      std::vector<uint32_t> c(M.cols.begin() + B.z, M.cols.begin() + B.w);
      std::vector<uint64_t> v(vb.begin() + B.z, vb.begin() + B.w);
      const uint32_t at = (uint32_t)(b * 7 + (size_t)what) % n;
      if (what == 0) c[at] += 1;
      if (what == 1) c[at] ^= 1u << 20;
      if (what == 2) v[at] = v[0];
      if (what == 3) v[at] ^= 1ull << 51;
      const ptrdiff_t holds = block_holding(plan.blk, B.z + at);
      NEED(holds == (ptrdiff_t)b, "block_holding(%u) = %td, not %zu", B.z + at, holds, b);
      PalettePool again = pool;
      std::vector<uint16_t> fresh(n + 1), re(n + 1);
      const Pair d = replan_packed_block(geo, again, B.z, B.w, c.data(), v.data(), re.data());
      const bool packs_now = plan_packed_block(geo, B.z, B.w, c.data(), v.data(), cbase, shift, pal, fresh.data());
      NEED((d.y != 0u) == packs_now, "re-plan %d of block %zu: packed %d, packs %d", what, b, d.y != 0u, packs_now);  // (1024 spare palettes: room)
      NEED(again.host.size() <= again.cap, "pool over its capacity");
      if (!packs_now) continue;
      NEED(d.x == cbase && (d.y & 31u) == shift && re == fresh, "re-plan %d of block %zu differs from a fresh plan", what, b);
      check_packed_block(B, d, re.data(), again, c.data(), v.data());
      const uint32_t no = d.y >> 5;
      NEED(std::equal(pal.begin(), pal.end(), again.host.begin() + no * ABFT_PAL_ENTRIES), "palette %u", no);
      // compact columns under the same change
      uint16_t off;
      const uint32_t base = *std::min_element(M.cols.begin() + B.z, M.cols.begin() + B.w);
      if (compact_offset(base, c[at], off)) NEED(base + off == c[at], "offset"); else NEED(c[at] - base > 0xFFFFu, "went wide");
    }
    // a pool with room for two more palettes: the third new one demotes its block, and nothing is written past the end
    PalettePool small = pool;
    small.seal(2);
    std::vector<uint64_t> v(vb.begin() + B.z, vb.begin() + B.w);
    std::vector<uint16_t> re(n + 1);
    for (int k = 0; k < 4; k++) {
      v[0] = 0x7ff8000000000000ull + (uint64_t)k + b * 4;  // (a pattern no generator makes)
      const bool packs_now = plan_packed_block(geo, B.z, B.w, M.cols.data() + B.z, v.data(), cbase, shift, pal, re.data());
      const Pair d = replan_packed_block(geo, small, B.z, B.w, M.cols.data() + B.z, v.data(), re.data());
      NEED(small.host.size() <= small.cap, "pool over its capacity");
      NEED((d.y != 0u) == (packs_now && k < 2), "re-plan %d into a pool with two spare palettes: packed %d", k, d.y != 0u);
    }
  }
  for (int i = 0; i < nnz; i += std::max(1, nnz / 64)) {
    const ptrdiff_t b = block_holding(plan.blk, (uint32_t)i);
    NEED(b >= 0 && plan.blk[(size_t)b].z <= (uint32_t)i && (uint32_t)i < plan.blk[(size_t)b].w, "block_holding(%d) = %td", i, b);
  }
  NEED(block_holding(plan.blk, (uint32_t)nnz) < 0, "an element past the end has a block");
}

// ---- one case ----------------------------------------------------------------------------------------------------

static void print_panels(Line &L, const Case &c, const LayoutKnobs &knobs, const PanelBuild &pb, const Matrix &M) {
  L.num("ngroups", pb.ngroups).num("npanels", pb.npanels).num("width", pb.width).arr("seg_base", pb.seg_base).arr("seg_ptr", pb.seg_ptr);
  L.num("xpf", (uint32_t)std::max(0L, knobs.xpf));
  auto resident = [&](CooPanelKernel k) { return (uint32_t)(coo_panels_per_cu(c, (int)k) * c.cus); };
  const int per_cu = c.coo ? 8 : csr_panels_per_cu(c);
  const PanelLaunch P = panel_launch(knobs, c.coo, c.mode == 1, (uint32_t)M.n_in, pb.ngroups, (uint32_t)(per_cu * c.cus), resident);
  L.num("panel_grid", P.grid).num("panel_chunk", P.chunk).num("panel_lag", P.lag).num("coo_kernel", (int)P.kernel);
  NEED(P.grid >= 1 && P.grid <= pb.ngroups, "panel grid %u of %u groups", P.grid, pb.ngroups);
  NEED(c.coo || (P.lag == 0 && P.kernel == CooPanelKernel::Panels), "a CSR matrix with a COO launch");
  NEED(P.lag == 0 || P.chunk == 0, "paced and chunked");
}

static void run_csr(const Case &c, const PlanGeometry &geo, const LayoutKnobs &knobs, const Matrix &M) {
  const int nnz = M.nnz();
  CsrPlan plan;
  PalettePool pool;
  auto waves = [&](uint32_t lg) { return slice_wave_capacity(c, lg); };
  auto cap = [&](int rpt) { return sweep_capacity(c, rpt); };
  plan_csr(geo, knobs, c.mode == 0, c.mode == 1, c.stream, M.cols.data(), M.rows.data(), M.vals.data(), M.n_out, M.n_in, nnz, waves, cap,
           pool, plan);
  Line L(c.name);
  L.num("layout", layout_number(plan.layout)).arr("rowptr", plan.rowptr).arr("blk", plan.blk);
  static const std::vector<uint32_t> none32;
  static const std::vector<uint16_t> none16;
  static const std::vector<Pair> none_pair;
  if (plan.layout == Layout::Slice) {
    const SliceBuild &s = plan.slice;
    L.num("nslices", s.nslices).num("npanels", s.npanels).num("width", s.width).num("rows_log2", s.rows_log2);
    L.arr("sub", s.sub).arr("rid", s.rid).arr("pos", s.pos).arr("orig", s.orig);
    const uint32_t grid = slice_grid(s.nslices, (uint32_t)waves(s.rows_log2));
    L.num("grid", grid).num("lag", knob_u32(knobs.slice_lag, 0L, 2u));
    NEED(grid >= 1 && grid <= (s.nslices + 3) / 4, "slice grid %u", grid);
    check_slice(s, M);
  } else if (plan.layout == Layout::Sweep) {
    const SweepBuild &s = plan.sweep;
    L.num("ngroups", s.ngroups).num("npanels", s.npanels).num("width", s.width).num("rpt", s.rpt);
    L.arr("wbase", s.wbase).arr("counts", s.counts).arr("pos", s.pos).arr("orig", s.orig);
    const uint32_t grid = sweep_grid(s.ngroups, (uint32_t)cap(s.rpt));
    L.num("grid", grid).num("lag", knob_u32(knobs.sweep_lag, 0L, 2u));
    NEED(grid >= 1 && grid <= s.ngroups, "sweep grid %u", grid);
    NEED(c.mode != 1 || s.rpt != 16, "16 rows per thread in constraints mode");
    check_sweep(s, M);
  } else if (plan.layout == Layout::Panels) {
    L.arr("pos", plan.panels.pos).arr("orig", plan.panels.orig);
    print_panels(L, c, knobs, plan.panels, M);
    check_panels(geo, plan.panels, plan.panels.pos, M.cols.data(), M.rows.data(), M.n_out, M.n_in, nnz);
  } else {
    const bool co = plan.compact.any, pk = plan.packed.any;
    L.num("compact", co).arr("cbase", co ? plan.compact.cbase : none32).arr("c16", co ? plan.compact.c16 : none16);
    L.num("packed", pk).arr("pdesc", pk ? plan.packed.pdesc : none_pair).arr("codes", pk ? plan.packed.codes : none16);
    L.arr("pal", pool.host).num("pal_cap", (long long)pool.cap);
    NEED(c.mode == 0 || (!co && !pk), "compact or packed in mode %d", c.mode);
    check_stream(geo, knobs, plan, pool, M);
  }
  L.print();
  NEED(plan.rowptr.size() == (size_t)M.n_out + 1 && plan.rowptr[0] == 0 && plan.rowptr[(size_t)M.n_out] == (uint32_t)nnz, "row pointers");
  for (int i = 0; i < nnz; i++) NEED(plan.rowptr[M.rows[i]] <= (uint32_t)i && (uint32_t)i < plan.rowptr[M.rows[i] + 1], "element %d", i);
  check_blocks(geo, plan.blk, plan.rowptr, (uint32_t)M.n_out, geo.csr_tile, true, (uint32_t)nnz);
  if (plan.layout != Layout::Stream) {
    check_permutation(plan.pos(), plan.orig(), nnz);
    check_order(plan.pos(), M.rows.data(), M.n_out, nnz);
  }
}

static void run_coo(const Case &c, const PlanGeometry &geo, const LayoutKnobs &knobs, const Matrix &M) {
  const int nnz = M.nnz();
  CooPlan plan;
  // (COO: the output is the column, the gathered index the row)
  plan_coo(geo, knobs, c.mode == 1, M.cols.data(), M.rows.data(), M.n_out, M.n_in, nnz, plan);
  Line L(c.name);
  L.num("layout", layout_number(plan.layout)).arr("grp", plan.grp).arr("blk", plan.blk);
  L.arr("pos", plan.pos.data(), (size_t)nnz).arr("orig", plan.orig.data(), (size_t)nnz).arr("as_created", plan.as_created);
  if (plan.layout == Layout::Panels) {
    print_panels(L, c, knobs, plan.panels, M);
    check_panels(geo, plan.panels, plan.pos, M.rows.data(), M.cols.data(), M.n_out, M.n_in, nnz);
  }
  L.print();
  NEED(plan.layout == Layout::Stream || plan.layout == Layout::Panels, "layout");
  check_permutation(plan.pos, plan.orig, nnz);
  check_order(plan.pos, M.cols.data(), M.n_out, nnz);
  check_blocks(geo, plan.blk, plan.grp, (uint32_t)M.n_out, geo.coo_tile, false, (uint32_t)nnz);
  if (plan.layout == Layout::Stream)
    for (int i = 0; i < nnz; i++) NEED(plan.grp[M.cols[i]] <= plan.pos[i] && plan.pos[i] < plan.grp[M.cols[i] + 1], "element %d", i);
  NEED(plan.as_created.size() == (c.mode == 1 ? (size_t)nnz + 1 : 0), "as_created");
  for (int i = 0; c.mode == 1 && i < nnz; i++) {
    const Pair p = plan.as_created[plan.pos[i]];
    NEED((p.x == M.cols[i] && p.y == M.rows[i]) || (p.x == ~M.cols[i] && p.y == ~M.rows[i]), "as_created of element %d", i);
  }
}

int main() {
  Case c;
  while (read_case(stdin, c)) {
    g_case = &c;
    const PlanGeometry geo = {c.geo[0], c.geo[1], c.geo[2], c.geo[3], c.geo[4], c.geo[5]};
    const LayoutKnobs knobs = read_knobs([&](const char *name) { return c.get(name); });
    const Matrix M = generate(c);
    // (what abft_hip.hip refuses before it plans)
    NEED(c.coo || std::is_sorted(M.rows.begin(), M.rows.end()), "rows not sorted");
    if (c.coo) run_coo(c, geo, knobs, M); else run_csr(c, geo, knobs, M);
  }
  return 0;
}
