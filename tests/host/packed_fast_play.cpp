// The fast words of packed row blocks (abft_sparse_cg_amd/csrc/layout_plan.h, packed_fast_word) without a GPU: plans
// seeded matrices at the library's geometry and at a toy one and checks, for every block, that the word is set exactly
// when its conditions hold and that what the SpMV then skips cannot go wrong: all 65 536 code values decode to a
// column inside the gathered vector and an entry inside the palette pool, the whole tile window of codes is allocated
// (every code of it is read here, under AddressSanitizer), the row length in the word is every row's length, and a
// re-planned block's word is what a fresh plan gives, or 0.  Built with -fsanitize=address,undefined by
// tests/test_packed_fast_host.py; a broken expectation or a sanitizer report ends it with a non-zero status.
// Usage: packed_fast_play BLOCK CSR_TILE  -- prints one line per case:
//   name blocks packed stage_fast row_fast window_fails alloc_only_fails replanned
#include <cstdarg>
#include <cstdio>
#include <string>

#if !defined(ABFT_PAL_ENTRIES) || !defined(ABFT_CBASE_WIDE) || !defined(ABFT_PAL_SPARE)
#error "build with -DABFT_PAL_ENTRIES=... -DABFT_CBASE_WIDE=... -DABFT_PAL_SPARE=... as abft_internal.h and abft_hip.hip have them"
#endif
#include "layout_plan.h"

[[noreturn]] static void fail(const char *what, int line, const char *fmt, ...) {
  fprintf(stderr, "packed_fast_play: %s (line %d): ", what, line);
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
  exit(1);
}
#define NEED(cond, ...) do { if (!(cond)) fail(#cond, __LINE__, __VA_ARGS__); } while (0)

static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }

struct Rng {  // xorshift64*: the same stream everywhere
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
  uint32_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32); }
  uint32_t below(uint32_t n) { return next() % n; }
};

struct Matrix {
  int n_out = 0, n_in = 0;
  std::vector<uint32_t> cols, rows;
  std::vector<double> vals;
  void add(uint32_t r, uint32_t c, double v) { rows.push_back(r); cols.push_back(c); vals.push_back(v); }
  int nnz() const { return (int)cols.size(); }
};

// rows of `len(r)` elements, columns ascending from about the row's own index (clamped into the vector), values from a
// palette of `nv` patterns
template <typename Len, typename First>
static Matrix banded(int n_out, int n_in, uint32_t nv, Len len, First first) {
  Matrix M;
  M.n_out = n_out; M.n_in = n_in;
  for (int r = 0; r < n_out; r++) {
    const uint32_t L = len(r);
    uint32_t c = std::min<uint32_t>(first(r), (uint32_t)n_in - std::min<uint32_t>(L, (uint32_t)n_in));
    for (uint32_t j = 0; j < L && c < (uint32_t)n_in; j++, c++) M.add((uint32_t)r, c, 1.0 + (double)((r + 3 * j) % nv));
  }
  return M;
}

struct Counts { size_t blocks = 0, packed = 0, stage = 0, row = 0, window_fails = 0, alloc_only = 0, replanned = 0; };

static volatile uint32_t g_sink;

// what a set word promises, from the arrays alone
static void check_word(const PlanGeometry &geo, const Blk &B, Pair pd, uint32_t word, uint32_t n_in, const uint16_t *codes, size_t codes_len,
                       const PalettePool &pool, const uint32_t *rowptr) {
  if (word == 0u) return;
  NEED((word & ABFT_FAST_STAGE) != 0u && (word & ~(ABFT_FAST_STAGE | 0xFu << ABFT_FAST_LEN_SHIFT)) == 0u, "word %#x", word);
  NEED(pd.y != 0u, "a fast word on a block that is not packed");
  const uint32_t shift = pd.y & 31u, mask = (1u << shift) - 1u, pbase = (pd.y >> 5) * ABFT_PAL_ENTRIES;
  NEED(shift >= 12u && shift <= 16u, "shift %u", shift);
  for (uint32_t code = 0; code < 65536u; code++) {
    NEED((uint64_t)pd.x + (code & mask) < (uint64_t)n_in, "code %#x gathers entry %llu of %u", code, (unsigned long long)pd.x + (code & mask), n_in);
    NEED((size_t)pbase + (code >> shift) < pool.host.size(), "code %#x reads past the palette pool", code);
  }
  const uint32_t base = B.z & ~1u;
  NEED((size_t)base + geo.csr_tile <= codes_len && B.w - base <= geo.csr_tile, "tile window [%u, %u) of %zu codes", base, base + geo.csr_tile, codes_len);
  uint32_t sum = 0;
  for (uint32_t k = 0; k < geo.csr_tile; k++) sum += codes[base + k];  // (every slot the kernel loads: the sanitizer watches)
  g_sink = sum;
  const uint32_t len = word >> ABFT_FAST_LEN_SHIFT;
  if (len == 0u) return;
  const uint32_t rows = (B.y & 0x7fffffffu) - B.x;
  NEED(len <= ABFT_FAST_LEN_MAX && rows >= 1u && rows <= geo.block && B.z + len * rows == B.w, "len %u, %u rows, elements [%u, %u)", len, rows, B.z, B.w);
  for (uint32_t r = B.x; r < (B.y & 0x7fffffffu); r++)
    NEED(rowptr[r] == B.z + len * (r - B.x) && rowptr[r + 1] - rowptr[r] == len, "row %u is [%u, %u), the word says %u elements", r, rowptr[r], rowptr[r + 1], len);
}

// the conditions of the issue, spelt out a second time
static uint32_t expected_word(const PlanGeometry &geo, const Blk &B, Pair pd, uint32_t n_in, size_t codes_len, const uint32_t *rowptr, bool *window,
                              bool *alloc) {
  *window = *alloc = false;
  if (pd.y == 0u) return 0u;
  if (!(B.w >= B.z && B.w - (B.z & ~1u) <= geo.csr_tile)) return 0u;
  *window = (uint64_t)pd.x + (1ull << (pd.y & 31u)) <= (uint64_t)n_in;
  *alloc = (uint64_t)(B.z & ~1u) + geo.csr_tile <= (uint64_t)codes_len;
  if (!*window || !*alloc) return 0u;
  uint32_t word = 1u;
  const uint32_t r0 = B.x, r1 = B.y & 0x7fffffffu;
  if ((B.y >> 31) != 0u && r1 - r0 <= geo.block) {
    const uint32_t len = rowptr[r0 + 1] - rowptr[r0];
    bool same = len >= 1u && len <= 8u;
    for (uint32_t r = r0; same && r < r1; r++) same = rowptr[r + 1] - rowptr[r] == len;
    if (same) word |= len << 8;
  }
  return word;
}

static void run(const char *name, const PlanGeometry &geo, const Matrix &M) {
  LayoutKnobs knobs;
  knobs.packed_fast = true;
  CsrPlan plan;
  PalettePool pool;
  auto never = [](auto) { return (uint64_t)1; };
  const int nnz = M.nnz();
  plan_csr(geo, knobs, true, false, true, M.cols.data(), M.rows.data(), M.vals.data(), M.n_out, M.n_in, nnz, never, never, pool, plan);
  NEED(plan.layout == Layout::Stream, "forced to stream");
  Counts n;
  n.blocks = plan.blk.size();
  const PackedBuild &pk = plan.packed;
  if (pk.any) {
    NEED(pk.fast.size() == plan.blk.size() && pk.pdesc.size() == plan.blk.size() && pk.codes.size() == plan.padded + 2, "sizes");
    std::vector<uint64_t> vb((size_t)nnz);
    for (int i = 0; i < nnz; i++) vb[i] = bits(M.vals[i]);
    for (size_t b = 0; b < plan.blk.size(); b++) {
      const Blk &B = plan.blk[b];
      bool window, alloc;
      const uint32_t want = expected_word(geo, B, pk.pdesc[b], (uint32_t)M.n_in, pk.codes.size(), plan.rowptr.data(), &window, &alloc);
      NEED(pk.fast[b] == want, "block %zu: word %#x, the conditions give %#x", b, pk.fast[b], want);
      NEED(pk.fast[b] == packed_fast_word(geo, B, pk.pdesc[b], (uint32_t)M.n_in, pk.codes.size()), "block %zu: create and the function differ", b);
      check_word(geo, B, pk.pdesc[b], pk.fast[b], (uint32_t)M.n_in, pk.codes.data(), pk.codes.size(), pool, plan.rowptr.data());
      n.packed += pk.pdesc[b].y != 0u;
      n.stage += (pk.fast[b] & 1u) != 0u;
      n.row += (pk.fast[b] >> 8) != 0u;
      if (pk.pdesc[b].y != 0u && one_tile(geo, B.z, B.w)) {
        n.window_fails += !window;
        n.alloc_only += window && !alloc;
      }
      // one element changed, the block planned again: the word the re-plan leads to is a fresh plan's, or 0
      const uint32_t cnt = B.w - B.z;
      if (pk.pdesc[b].y == 0u || cnt == 0u || (b % 7 != 0 && b + 3 < plan.blk.size())) continue;
      for (int what = 0; what < 5; what++) {
        std::vector<uint32_t> c(M.cols.begin() + B.z, M.cols.begin() + B.w);
        std::vector<uint64_t> v(vb.begin() + B.z, vb.begin() + B.w);
        const uint32_t at = (uint32_t)(b * 5 + (size_t)what) % cnt;
        if (what == 0) c[at] = std::min<uint32_t>(c[at] + 1u, (uint32_t)M.n_in - 1u);
        if (what == 1) c[at] ^= 1u << 20;                   // far away: the block does not pack any more
        if (what == 2) c[at] = (uint32_t)M.n_in - 1u;       // the window may now reach the vector's end
        if (what == 3) v[at] ^= 1ull << 51;                 // a new value pattern: maybe a smaller shift
        if (what == 4) c[at] = 0u;                          // the base moves down
        PalettePool again = pool, fresh_pool = pool;
        std::vector<uint16_t> re(cnt + 1), fresh(cnt + 1);
        const Pair d = replan_packed_block(geo, again, B.z, B.w, c.data(), v.data(), re.data());
        const uint32_t word = packed_fast_word(geo, B, d, (uint32_t)M.n_in, pk.codes.size());
        uint32_t cbase, shift;
        Palette pal;
        uint32_t fresh_word = 0u;
        Pair fd{0u, 0u};
        if (plan_packed_block(geo, B.z, B.w, c.data(), v.data(), cbase, shift, pal, fresh.data()) && fresh_pool.takes(pal)) {
          fd = fresh_pool.desc(cbase, shift, pal);
          bool w2, a2;
          fresh_word = expected_word(geo, B, fd, (uint32_t)M.n_in, pk.codes.size(), plan.rowptr.data(), &w2, &a2);
        }
        NEED(d.x == fd.x && d.y == fd.y, "re-plan %d of block %zu: descriptor {%u, %#x}, fresh {%u, %#x}", what, b, d.x, d.y, fd.x, fd.y);
        NEED(word == fresh_word && (d.y != 0u || word == 0u), "re-plan %d of block %zu: word %#x, fresh %#x", what, b, word, fresh_word);
        // the re-planned codes in their place, as the device would hold them
        std::vector<uint16_t> codes2 = pk.codes;
        if (d.y != 0u) std::copy(re.begin(), re.begin() + cnt, codes2.begin() + B.z);
        check_word(geo, B, d, word, (uint32_t)M.n_in, codes2.data(), codes2.size(), again, plan.rowptr.data());
        n.replanned++;
      }
    }
  }
  // the switch off, or unset: no word anywhere
  for (int off = 0; off < 2; off++) {
    LayoutKnobs k2;
    if (off) k2.packed_fast = false;
    CsrPlan p2;
    PalettePool pool2;
    plan_csr(geo, k2, true, false, true, M.cols.data(), M.rows.data(), M.vals.data(), M.n_out, M.n_in, nnz, never, never, pool2, p2);
    NEED(p2.packed.pdesc.size() == pk.pdesc.size() && p2.packed.codes == pk.codes, "the switch changed the codes");
    for (size_t b = 0; b < p2.packed.pdesc.size(); b++) NEED(p2.packed.pdesc[b].x == pk.pdesc[b].x && p2.packed.pdesc[b].y == pk.pdesc[b].y, "the switch changed descriptor %zu", b);
    for (uint32_t w : p2.packed.fast) NEED(w == 0u, "a word with the switch off");
  }
  printf("%s %zu %zu %zu %zu %zu %zu %zu\n", name, n.blocks, n.packed, n.stage, n.row, n.window_fails, n.alloc_only, n.replanned);
}

int main(int argc, char **argv) {
  NEED(argc == 3, "usage: packed_fast_play BLOCK CSR_TILE");
  PlanGeometry geo;
  geo.block = (uint32_t)atoi(argv[1]);
  geo.csr_tile = (uint32_t)atoi(argv[2]);
  geo.coo_tile = geo.csr_tile; geo.panel_rows = geo.block; geo.sweep_ept = 8; geo.max_segments = 4 * geo.block;
  const bool toy = geo.csr_tile < 64;
  // rows: few at the toy geometry (a block is a row or two), the gathered vector as long as the windows need
  const int R = toy ? 400 : 67600;
  {  // two values, rows of 5 next to the diagonal: shift 15, so only the blocks within 32768 entries of the vector's end fail the window
    const int n_in = 67600;
    const double step = (double)(n_in - 5) / (double)R;
    run("band2.last_blocks", geo, banded(R, n_in, 2, [](int) { return 5u; }, [&](int r) { return (uint32_t)(r * step); }));
  }
  {  // the same band, but the last rows hold small columns: their window is fine, their tile reaches past the codes
    const int n_in = 67600, tail = toy ? 3 : 300;
    const double step = (double)(n_in - 40000) / (double)R;
    run("small_columns_last", geo, banded(R, n_in, 2, [](int) { return 3u; }, [&](int r) { return r >= R - tail ? (uint32_t)(r - (R - tail)) : (uint32_t)(r * step); }));
  }
  {  // a vector shorter than any window
    const int n = toy ? 400 : 3000;
    run("short_vector", geo, banded(n, n, 2, [](int) { return 5u; }, [](int r) { return (uint32_t)r; }));
    run("short_vector.4095", geo, banded(toy ? 400 : 4000, 4095, 16, [](int) { return 2u; }, [](int r) { return (uint32_t)r; }));
    run("vector.4096", geo, banded(toy ? 400 : 4000, 4096, 16, [](int) { return 2u; }, [](int) { return 0u; }));  // exactly one window
  }
  // sixteen values (shift 12), uniform rows of every length the row-fast field knows and its neighbours; then with a
  // one-element first row, so that later blocks start at odd elements
  for (uint32_t len : {1u, 2u, 3u, 4u, 5u, 7u, 8u, 9u, 16u})
    for (int odd = 0; odd < 2; odd++) {
      const int n = toy ? 300 : 12000;
      const std::string name = "band16.len" + std::to_string(len) + (odd ? ".odd" : "");
      run(name.c_str(), geo, banded(n, 12000, 16, [&](int r) { return odd && r == 0 ? 1u : len; }, [&](int r) { return (uint32_t)((double)r * 11000.0 / n); }));
    }
  // seeded: row lengths, palettes and vector lengths at random
  for (uint64_t seed = 1; seed <= (toy ? 40u : 12u); seed++) {
    Rng g(seed);
    const int n_out = toy ? 60 + (int)g.below(200) : 3000 + (int)g.below(6000);
    const int n_in = 2000 + (int)g.below(seed % 3 == 0 ? 6000u : 80000u);
    const uint32_t nv = 1 + g.below(18), maxlen = 1 + g.below(toy ? 9u : 12u), mode = g.below(3);
    std::vector<uint32_t> len((size_t)n_out), first((size_t)n_out);
    const uint32_t fixed = 1 + g.below(maxlen);
    for (int r = 0; r < n_out; r++) {
      len[r] = mode == 0 ? fixed : mode == 1 ? (g.below(10) ? fixed : g.below(maxlen + 1)) : g.below(maxlen + 1);
      first[r] = (uint32_t)((double)r / n_out * n_in) + g.below(64);
    }
    const std::string name = "seeded." + std::to_string(seed);
    run(name.c_str(), geo, banded(n_out, n_in, nv, [&](int r) { return len[r]; }, [&](int r) { return first[r]; }));
  }
  return 0;
}
