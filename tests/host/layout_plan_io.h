// layout_plan_io.h -- what tests/host/layout_plan_play.cpp reads and prints, apart from the planner itself: the case
// description on stdin, the seeded matrix generators, the stand-ins for the kernels' occupancy, the digest.  (The
// program that recorded tests/golden/layout_plan.json from the parent commit's planner shared this file, so both
// read the same cases and print the same format.)
//
//   case NAME
//   geo BLOCK CSR_TILE COO_TILE PANEL_ROWS SWEEP_EPT MAX_SEGMENTS
//   fmt csr|coo          mode 0..5 (abft_hip.h: 0 none, 1 constraints)      stream 1 (create_csr_stream)
//   cus N                compute units the occupancy stand-ins multiply by
//   env NAME VALUE       an environment variable of the create (VALUE may be empty)
//   gen KIND A B C ...   the matrix (see generate)
//   run
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

struct Case {
  std::string name, kind;
  uint32_t geo[6] = {256, 1024, 1024, 2048, 8, 1024};
  bool coo = false, stream = false;
  int mode = 0, cus = 256;
  std::vector<std::pair<std::string, std::string>> env;
  std::vector<long> arg;
  long a(size_t k, long unset = 0) const { return k < arg.size() ? arg[k] : unset; }
  const char *get(const char *name) const {
    for (auto &kv : env)
      if (kv.first == name) return kv.second.c_str();
    return nullptr;
  }
};

static inline bool read_case(FILE *f, Case &c) {
  c = Case();
  char line[512];
  bool any = false;
  while (fgets(line, sizeof(line), f)) {
    std::istringstream in(line);
    std::string word;
    if (!(in >> word)) continue;
    any = true;
    if (word == "run") return true;
    if (word == "case") in >> c.name;
    else if (word == "geo") for (uint32_t &g : c.geo) in >> g;
    else if (word == "fmt") { in >> word; c.coo = word == "coo"; }
    else if (word == "mode") in >> c.mode;
    else if (word == "stream") in >> c.stream;
    else if (word == "cus") in >> c.cus;
    else if (word == "env") { std::string n, v; in >> n; in >> v; c.env.emplace_back(n, v); }
    else if (word == "gen") { in >> c.kind; long v; while (in >> v) c.arg.push_back(v); }
    else { fprintf(stderr, "unknown line: %s", line); exit(2); }
  }
  if (any) { fprintf(stderr, "case %s has no `run`\n", c.name.c_str()); exit(2); }
  return false;
}

// ---- matrices, in the caller's order (row-major, rows ascending) ----

struct Matrix {
  int n_out = 0, n_in = 0;
  std::vector<uint32_t> cols, rows;
  std::vector<double> vals;
  int nnz() const { return (int)cols.size(); }
  void add(uint32_t r, uint32_t c, double v) { rows.push_back(r); cols.push_back(c); vals.push_back(v); }
};

struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull) {}
  uint64_t next() {  // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

// the value of an element: one of `nvals` patterns (0: every element its own)
static inline double value_of(Rng &rng, long nvals, size_t i) {
  return nvals > 0 ? 1.0 + 0.5 * (double)rng.below((uint32_t)nvals) : 1.0 + 1e-3 * (double)i;
}

//   rand ROWS COLS K SEED NVALS [DESC_ROW [STEP]]   K random columns in every STEP-th row, ascending (row DESC_ROW: descending)
//   revrand ...                               as rand, the elements in reverse order (COO only: rows descend)
//   band N HALF NVALS                         columns [r - HALF, r + HALF] inside the matrix
//   uniform N K STRIDE [ROW LEN]              every row K elements, columns (r + j * STRIDE) mod N ascending; row ROW: LEN
//   longrow N_OUT N_IN ROW LEN                one element per row on the diagonal; row ROW: LEN elements over all columns
//   trailing N K EMPTY SEED                   as rand, the last EMPTY rows empty
//   empty N                                   no elements
//   span HI                                   2 rows over HI + 1 columns: {0, HI}, {5}
//   vals NV HI                                4 rows, NV + 1 elements of NV distinct values, columns from 0 to HI
//   tiny N_OUT N_IN MAXK SEED NVALS           0 .. MAXK columns per row, ascending, repeats allowed
static inline Matrix generate(const Case &c) {
  Matrix M;
  const std::string &k = c.kind;
  if (k == "rand" || k == "revrand" || k == "trailing" || k == "tiny") {
    const bool tr = k == "trailing", tiny = k == "tiny";
    const int nrows = (int)c.a(0), ncols = tr ? nrows : (int)c.a(1);
    const long K = tr ? c.a(1) : c.a(2), nvals = tr ? 3 : c.a(4), desc = tr || tiny ? -1 : c.a(5, -1), step = tr || tiny ? 1 : c.a(6, 1);
    const int filled = tr ? nrows - (int)c.a(2) : nrows;
    Rng rng((uint64_t)c.a(3));
    std::vector<uint32_t> row;
    for (int r = 0; r < filled; r += (int)step) {
      row.resize(tiny ? rng.below((uint32_t)K + 1) : (size_t)K);
      for (uint32_t &x : row) x = rng.below((uint32_t)ncols);
      std::sort(row.begin(), row.end());
      if (r == desc) std::reverse(row.begin(), row.end());
      for (uint32_t x : row) M.add((uint32_t)r, x, value_of(rng, nvals, M.cols.size()));
    }
    if (k == "revrand") {
      std::reverse(M.rows.begin(), M.rows.end());
      std::reverse(M.cols.begin(), M.cols.end());
      std::reverse(M.vals.begin(), M.vals.end());
    }
    // (COO: the columns are the outputs, the rows what is gathered)
    M.n_out = c.coo ? ncols : nrows;
    M.n_in = c.coo ? nrows : ncols;
  } else if (k == "band") {
    M.n_out = M.n_in = (int)c.a(0);
    Rng rng(1);
    for (long r = 0; r < M.n_out; r++)
      for (long x = std::max(0L, r - c.a(1)); x <= std::min((long)M.n_in - 1, r + c.a(1)); x++)
        M.add((uint32_t)r, (uint32_t)x, value_of(rng, c.a(2), M.cols.size()));
  } else if (k == "uniform") {
    M.n_out = M.n_in = (int)c.a(0);
    std::vector<uint32_t> row;
    for (long r = 0; r < M.n_out; r++) {
      row.resize((size_t)(r == c.a(3, -1) ? c.a(4) : c.a(1)));
      for (size_t j = 0; j < row.size(); j++) row[j] = (uint32_t)((r + (long)j * c.a(2)) % M.n_in);
      std::sort(row.begin(), row.end());
      for (uint32_t x : row) M.add((uint32_t)r, x, x % 2 ? -1.0 : 4.0);
    }
  } else if (k == "longrow") {
    M.n_out = (int)c.a(0); M.n_in = (int)c.a(1);
    for (long r = 0; r < M.n_out; r++) {
      if (r != c.a(2)) { M.add((uint32_t)r, (uint32_t)(r % M.n_in), 2.0); continue; }
      for (long j = 0; j < c.a(3); j++) M.add((uint32_t)r, (uint32_t)(j * M.n_in / c.a(3)), 1.0 + (double)(j % 3));
    }
  } else if (k == "empty") {
    M.n_out = M.n_in = (int)c.a(0);
  } else if (k == "span") {
    M.n_out = 2; M.n_in = (int)c.a(0) + 1;
    M.add(0, 0, 1.0); M.add(0, (uint32_t)c.a(0), 2.0); M.add(1, 5, 1.0);
  } else if (k == "vals") {
    M.n_out = 4; M.n_in = (int)c.a(1) + 1;
    const long nv = c.a(0);
    for (long j = 0; j <= nv; j++)
      M.add((uint32_t)(j * 4 / (nv + 1)), (uint32_t)(j == nv ? c.a(1) : j), 1.0 + (double)(j % nv));
  } else {
    fprintf(stderr, "unknown matrix kind %s\n", k.c_str());
    exit(2);
  }
  return M;
}

// ---- stand-ins for the occupancy the library asks the runtime for (resident workgroups per compute unit) ----

static inline uint64_t sweep_capacity(const Case &c, int rpt) { return (uint64_t)(rpt <= 4 ? 4 : rpt == 8 ? 2 : 1) * (uint64_t)c.cus; }
static inline uint64_t slice_wave_capacity(const Case &c, uint32_t lg) { return (uint64_t)(lg <= 8 ? 2 : 1) * 4u * (uint64_t)c.cus; }
static inline int csr_panels_per_cu(const Case &) { return 2; }
static inline int coo_panels_per_cu(const Case &c, int kernel) { return kernel == 1 ? 1 : kernel == 2 ? 3 : 2 + (c.mode == 0); }

// ---- digest ----

static inline uint64_t fnv1a(const void *p, size_t bytes, uint64_t h = 0xcbf29ce484222325ull) {
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < bytes; i++) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}

// one output line per case: NAME key=value ...; an array prints as LENGTH:DIGEST
struct Line {
  std::string text;
  explicit Line(const std::string &name) : text(name) {}
  Line &num(const char *key, long long v) { text += " " + std::string(key) + "=" + std::to_string(v); return *this; }
  template <typename T>
  Line &arr(const char *key, const std::vector<T> &v) { return arr(key, v.data(), v.size()); }
  template <typename T>
  Line &arr(const char *key, const T *p, size_t n) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%zu:%016llx", n, (unsigned long long)fnv1a(p, n * sizeof(T)));
    text += " " + std::string(key) + "=" + buf;
    return *this;
  }
  void print() const { puts(text.c_str()); }
};
