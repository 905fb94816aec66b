"""IEEE-754 special values for the kernel tests: a comparison that is bit-exact except for NaN
payloads, input builders that mix +-0, subnormals, +-Inf, NaN, DBL_MAX and overflowing /
underflowing products into matrices and vectors, and the exact sum with an error bound derived
from the summation trees of the reduction kernels (test infrastructure only, not a conftest)."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTERNAL_H = os.path.join(ROOT, "abft_sparse_cg_amd", "csrc", "abft_internal.h")


def f64(bits):
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


DBL_MAX = float(np.finfo(np.float64).max)
TINY = f64(0x0000000000000001)        # 2^-1074, the smallest subnormal
MAX_SUB = f64(0x000FFFFFFFFFFFFF)     # the largest subnormal
MIN_NORMAL = f64(0x0010000000000000)  # 2^-1022
QNAN = f64(0x7FF800000000BEEF)        # quiet NaN with a payload
NEG_QNAN = f64(0xFFF8000000001234)
INF = float("inf")
U = 2.0 ** -53

# finite values an ordinary row may hold (products with x of order 1 stay finite)
FINITE_SPECIALS = [0.0, -0.0, TINY, -TINY, MAX_SUB, -MAX_SUB, MIN_NORMAL, -MIN_NORMAL, 1e-200, -1e-200]
# every kind of value, for element-wise kernels
ALL_SPECIALS = FINITE_SPECIALS + [1e200, -1e200, DBL_MAX, -DBL_MAX, INF, -INF, QNAN, NEG_QNAN]


def config_value(name):
    """an integer #define / constexpr of abft_internal.h"""
    with open(INTERNAL_H) as f:
        text = f.read()
    m = re.search(r"#define\s+%s\s+(\d+)" % name, text) or re.search(r"constexpr int %s\s*=\s*(\d+)" % name, text)
    assert m, name
    return int(m.group(1))


def csr_tile():
    """elements the streaming CSR kernel stages per tile: ABFT_BLOCK * ABFT_CFG_CSR_EPT"""
    return config_value("ABFT_BLOCK") * config_value("ABFT_CFG_CSR_EPT")


# ------------------------------------------------------------------ comparison --

def ieee_equal(gpu, ref):
    """True when the two float64 arrays are bit-identical, except that a NaN matches a NaN of
    any sign and payload.  The exception exists because IEEE 754 leaves the sign and payload of
    a NaN produced by an operation open: x86 SSE (the oracle and the reference) produces the
    default NaN 0xFFF8000000000000, gfx950 produces 0x7FF8000000000000.  Everything else must
    match exactly: the sign of a zero, every bit of a subnormal, the sign of an Inf."""
    a = np.ascontiguousarray(gpu, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(ref, dtype=np.float64).reshape(-1)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return bool(np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def ieee_diff(gpu, ref, limit=8):
    """the first few positions where ieee_equal fails, with both values as hex (for messages)"""
    a = np.ascontiguousarray(gpu, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(ref, dtype=np.float64).reshape(-1)
    bad = (np.isnan(a) != np.isnan(b)) | (~np.isnan(a) & (a.view(np.uint64) != b.view(np.uint64)))
    return [(int(i), float(a[i]).hex(), float(b[i]).hex()) for i in np.flatnonzero(bad)[:limit]]


def value_class(v):
    v = float(v)
    return "nan" if v != v else "+inf" if v == INF else "-inf" if v == -INF else "finite"


# ------------------------------------------------------------------ exact sums --

def exact_sum(terms):
    """The correctly rounded sum of the float64 terms (math.fsum), with the IEEE class of a sum
    that holds non-finite terms: any NaN, or +Inf with -Inf, gives NaN; one kind of Inf gives it.
    A finite sum whose exact value overflows gives the Inf of its sign.  An exact zero is +0.0 (also
    when every term is -0.0): what the reference's sums, which start from +0.0, return."""
    t = [float(v) for v in np.asarray(terms, dtype=np.float64).reshape(-1)]
    if any(v != v for v in t) or (INF in t and -INF in t):
        return float("nan")
    if INF in t:
        return INF
    if -INF in t:
        return -INF
    try:
        s = math.fsum(t)
    except OverflowError:  # an intermediate sum overflowed: sum 2^-64 times the terms instead
        s = math.fsum(math.ldexp(v, -64) for v in t)
        s = math.copysign(INF, s) if abs(s) > math.ldexp(DBL_MAX, -64) else math.ldexp(s, 64)
    return s if s != 0.0 else 0.0  # an exact zero is +0.0, as a sum that starts from +0.0 gives


def sum_bound(terms, h):
    """|computed - exact_sum(terms)| <= (h + 1) 2^-53 sum |terms| (+ one 2^-1074 per term for products
    that underflowed), for a summation tree of depth h over the terms.  The +1 covers the rounding of
    each product that formed a term."""
    t = np.abs(np.asarray(terms, dtype=np.float64).reshape(-1))
    return (h + 1) * U * math.fsum(t.tolist()) + len(t) * TINY


# Depth of the summation trees, from kernels.hip.  Every level of a tree rounds once, so a sum of
# depth h is off by at most about h 2^-53 sum |terms|.
#   block_sum: wave_sum is six DPP add steps (row_shr 1, 2, 4, 8, row_bcast 15, 31), then
#     (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]) over the four waves: 2 more -> BLOCK = 8.
#   dot_kernel (and the r.r of calc_xr, calc_r, residual_restart, dot_block, which walk the elements
#     the same way): G = reduce_blocks(n) workgroups of 256 threads; each thread adds its elements
#     serially (at most ceil(n / (256 G)) of them, rounded up to even for the 16-byte walk), then
#     block_sum (8).  reduce_finish: the last workgroup's threads add ceil(G / 256) partials serially,
#     then block_sum (8).
#   fuse_finalize_kernel (<= 8192 partials): one workgroup of 1024; per pass a thread adds
#     (v0 + v1) + (v2 + v3) four times into its sum (16 loads a pass: depth 4 per pass + 2), wave_sum
#     (6), then thread 0 adds the 16 wave sums serially (16).
#   fold_partials_kernel (> 8192 partials): nb = min(64, ceil(nblk / 2048)) workgroups, each adds a
#     chunk of ceil(nblk / nb) partials, a thread (v0 + v1) + (v2 + v3) per 1024 of them (depth 1 per
#     pass + 2), block_sum (8), then reduce_finish over nb <= 256 partials: 1 + 8.
#   A fused SpMV partial: each thread adds x[row] * y[row] of its rows serially (rows_per_thread),
#     then block_sum (8).
BLOCK_DEPTH = 8


def reduce_blocks(n):
    """kernels.hip reduce_blocks: >= 8 elements per thread before adding blocks, at most ABFT_MAX_PARTIALS"""
    nb = max(1, -(-n // (256 * 8)))
    return min(nb, config_value("ABFT_CFG_MAX_PARTIALS"))


def dot_depth(n):
    g = reduce_blocks(n)
    per_thread = -(-n // (256 * g))
    per_thread += per_thread & 1
    return per_thread + BLOCK_DEPTH + -(-g // 256) + BLOCK_DEPTH


def finalize_depth(nblk):
    if nblk <= 8192:
        passes = max(1, -(-nblk // (16 * 1024)))
        return 4 * passes + 2 + 6 + 16
    nb = min(64, -(-nblk // 2048))
    chunk = -(-nblk // nb)
    return -(-chunk // 1024) + 2 + BLOCK_DEPTH + 1 + BLOCK_DEPTH


def fused_depth(rows_per_thread, nblk):
    return rows_per_thread + BLOCK_DEPTH + finalize_depth(nblk)


# -------------------------------------------------------------- input builders --

class Built:
    """A matrix as (output index, gather index, value) triplets in summation order, its input
    vector, and the rows built on purpose: name -> list of output indices.  csr() / coo() give the
    create_matrix arguments (cols, rows, vals, n): CSR sums row r over its elements in column order;
    COO adds element (col=out, row=in) into y[out] in storage order, sorted by (row, col) -- the same
    order of terms for each output."""

    def __init__(self, n, out, inn, vals, x, crafted):
        self.n, self.x, self.crafted = n, np.asarray(x, dtype=np.float64), crafted
        order = np.lexsort((inn, out))
        self.out = np.asarray(out, dtype=np.uint32)[order]
        self.inn = np.asarray(inn, dtype=np.uint32)[order]
        self.vals = np.asarray(vals, dtype=np.float64)[order]

    def csr(self):
        return self.inn.copy(), self.out.copy(), self.vals.copy(), self.n

    def coo(self):
        order = np.lexsort((self.out, self.inn))
        return self.out[order].copy(), self.inn[order].copy(), self.vals[order].copy(), self.n

    def mat(self, fmt):
        return self.csr() if fmt == 0 else self.coo()

    def element_of(self, fmt, out, inn):
        """the caller's element index of (out, inn) in fmt's order"""
        c, r, _, _ = self.mat(fmt)
        o, i = (r, c) if fmt == 0 else (c, r)
        hit = np.flatnonzero((o == out) & (i == inn))
        assert len(hit) == 1
        return int(hit[0])

    def without(self, kinds):
        """the same matrix with the rows of the given crafted kinds emptied"""
        drop = np.isin(self.out, [r for k in kinds for r in self.crafted[k]])
        crafted = {k: ([] if k in kinds else v) for k, v in self.crafted.items()}
        return Built(self.n, self.out[~drop], self.inn[~drop], self.vals[~drop], self.x, crafted)

    def finite_x(self):
        """x with its non-finite entries and those beyond 1e100 set to 1.0: every product and row sum
        finite and of ordinary size once the rows with non-finite stored values, DBL_MAX or
        overflowing products are gone (without(["value_nonfinite", "max_order", "edge", "underflow"]))"""
        x = self.x.copy()
        x[~np.isfinite(x) | (np.abs(x) > 1e100)] = 1.0
        return x

    def row_terms(self, r):
        m = self.out == r
        return self.vals[m] * self.x[self.inn[m]]


def special_matrix(n=2304, seed=0, long_len=None, boundaries=(16, 64, 256, 257, 1024)):
    """Square n x n matrix and x with every kind of special value, the non-finite ones confined to
    the rows built for them (most rows stay finite, so the bit-exact check of those rows means
    something).  Rows built on purpose (self.crafted):
      negzero     every product -0.0 (sum +0.0: the sum starts from +0.0)
      inf_ninf    products +Inf and -Inf (NaN)
      zero_nan    a 0.0 value times x = NaN, and one times x = Inf (NaN: the product is formed)
      max_order   DBL_MAX, DBL_MAX, -DBL_MAX in element order (+Inf; a finite value if reordered)
      subnormal   every product subnormal (the sum is exact)
      underflow   products that underflow into subnormals or to zero, and that overflow
      empty       no element (+0.0)
      last_inf    rows of 1..13 elements whose last product is +-Inf (+-Inf)
      value_nonfinite  elements whose stored value is +-Inf or NaN
      edge        MAX, MAX | -MAX and -0 | -0 products across the column boundaries `boundaries`
                  (panel widths) and, in one long row, across the tile boundaries of the CSR kernel"""
    rng = np.random.default_rng(seed)
    tile = csr_tile()
    long_len = long_len or (2 * tile + 5)
    assert n > long_len + 16
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3, size=n)
    # special columns, spread over the range; ordinary rows never read them
    spec_cols = {}
    special_x = {"pzero": 0.0, "nzero": -0.0, "tiny": TINY, "maxsub": MAX_SUB, "minnorm": MIN_NORMAL,
                 "big": 1e200, "small": 1e-200, "huge": 1e160, "dmax": DBL_MAX, "inf": INF, "ninf": -INF,
                 "nan": QNAN, "three": 3.0}
    for k, (name, v) in enumerate(special_x.items()):
        c = (k * 173 + 37) % n
        spec_cols[name] = c
        x[c] = v
    ones = set()
    for b in boundaries:
        for c in (b - 2, b - 1, b, b + 1):
            if 0 <= c < n:
                ones.add(c)
    ones -= set(spec_cols.values())
    for c in ones:
        x[c] = 1.0
    bad_x = set(spec_cols.values()) | ones
    ordinary_cols = np.array(sorted(set(range(n)) - bad_x))
    zero_cols = [spec_cols[k] for k in ("pzero", "nzero", "tiny", "maxsub", "minnorm", "small")]

    out, inn, vals = [], [], []
    crafted = {k: [] for k in ("negzero", "inf_ninf", "zero_nan", "max_order", "subnormal", "underflow", "empty",
                               "last_inf", "edge", "value_nonfinite")}

    def add(r, terms):
        for c, v in terms:
            out.append(r)
            inn.append(c)
            vals.append(v)

    # crafted rows at the start, the middle and the end of the matrix (different blocks / groups)
    rows = iter([0, 1, 2, 3, 5, 8, 13, 21, n // 2, n // 2 + 1, n // 2 + 3, n - 1, n - 2, n - 3, n - 5, n - 8,
                 n // 3, n // 3 + 1, 2 * n // 3, 2 * n // 3 + 1] + list(range(100, 140)) + list(range(700, 720)))
    used = set()

    def take(kind):
        r = next(rows)
        used.add(r)
        crafted[kind].append(r)
        return r

    sc = spec_cols
    add(take("negzero"), [(sc["pzero"], -1.0), (sc["nzero"], 2.0), (sc["tiny"], -0.0), (sc["three"], -0.0)])
    add(take("negzero"), [(sc["nzero"], 5.0)])
    add(take("inf_ninf"), [(sc["inf"], 1.0), (sc["ninf"], 1.0)])
    add(take("inf_ninf"), sorted([(sc["dmax"], 4.0), (sc["inf"], -1.0)]))  # overflow to +Inf, then -Inf
    add(take("zero_nan"), sorted([(sc["nan"], 0.0), (sc["three"], 1.0)]))
    add(take("zero_nan"), sorted([(sc["inf"], 0.0), (sc["three"], 2.0)]))
    add(take("zero_nan"), sorted([(sc["ninf"], -0.0)]))
    ones_sorted = sorted(ones)
    add(take("max_order"), [(ones_sorted[0], DBL_MAX), (ones_sorted[1], DBL_MAX), (ones_sorted[2], -DBL_MAX)])
    add(take("max_order"), [(ones_sorted[3], -DBL_MAX), (ones_sorted[5], -DBL_MAX), (ones_sorted[8], DBL_MAX)])
    add(take("subnormal"), sorted([(sc["tiny"], 3.0), (sc["maxsub"], 0.5), (sc["three"], TINY), (sc["minnorm"], -0.25)]))
    add(take("subnormal"), sorted([(sc["tiny"], -7.0), (sc["three"], MAX_SUB)]))
    add(take("underflow"), sorted([(sc["small"], 1e-200), (sc["big"], 1e-170), (sc["three"], 1.0)]))  # 0, 1e30, 3
    add(take("underflow"), sorted([(sc["small"], 1e-120), (sc["tiny"], 0.75), (sc["minnorm"], 0.5)]))  # subnormal products
    add(take("underflow"), sorted([(sc["huge"], 1e160), (sc["three"], 1.0)]))  # overflow: +Inf
    take("empty")
    take("empty")
    oc = ordinary_cols
    add(take("value_nonfinite"), [(int(oc[3]), 2.0), (int(oc[40]), INF)])
    add(take("value_nonfinite"), [(int(oc[7]), QNAN), (int(oc[90]), 1.0)])
    add(take("value_nonfinite"), [(int(oc[11]), -INF)])
    for length in range(1, 14):
        r = take("last_inf")
        cs = list(ordinary_cols[rng.choice(len(ordinary_cols), size=length - 1, replace=False)])
        last = sc["inf"] if length % 2 else sc["ninf"]
        cs = sorted(c for c in cs if c < last)
        terms = [(c, float(rng.standard_normal())) for c in cs] + [(last, 1.0 + length)]
        add(r, terms)
    # across column (panel) boundaries: MAX, MAX | -MAX and -0 | -0
    for b in boundaries:
        if b + 1 >= n:
            continue
        if (b - 2) in ones and (b - 1) in ones and b in ones:
            add(take("edge"), [(b - 2, DBL_MAX), (b - 1, DBL_MAX), (b, -DBL_MAX)])
        if (b - 1) in ones and b in ones:
            add(take("edge"), [(b - 1, -0.0), (b, -0.0)])
    # one long row across the CSR tile boundaries: special values on each side of every boundary
    r = n // 4
    used.add(r)
    crafted["edge"].append(r)
    cs = np.sort(ordinary_cols[rng.choice(len(ordinary_cols), size=long_len, replace=False)])
    v = rng.standard_normal(long_len)
    for t in range(0, long_len, tile):
        for k, s in ((t - 1, -0.0), (t, TINY), (t + 1, -TINY), (t - 2, 1e-200)):
            if 0 <= k < long_len:
                v[k] = s
    add(r, list(zip(cs.tolist(), v.tolist())))

    # ordinary rows: standard normals scaled by 10^[-3, 3], 15 % finite special values, some reading
    # the zero / subnormal columns of x
    for r in range(n):
        if r in used:
            continue
        k = int(rng.choice([1, 2, 3, 4, 5, 7, 9, 12, 20]))
        cs = set(ordinary_cols[rng.choice(len(ordinary_cols), size=k, replace=False)].tolist())
        if rng.random() < 0.3:
            cs.add(int(rng.choice(zero_cols)))
        cs = sorted(cs)
        vv = rng.standard_normal(len(cs)) * 10.0 ** rng.integers(-3, 4, size=len(cs))
        sp = rng.random(len(cs)) < 0.15
        vv[sp] = rng.choice(FINITE_SPECIALS, size=int(sp.sum()))
        add(r, list(zip(cs, vv.tolist())))
    return Built(n, out, inn, vals, x, crafted)


def tile_edge_matrix(fmt_parities=(0, 1), seed=3):
    """CSR rows with TILE - 1, TILE, TILE + 1, 2 TILE and 2 TILE + 1 elements, each the only row of its
    block, the block's first element at an even and at an odd position (a short filler row before it
    sets the parity), TILE = csr_tile() read from abft_internal.h.  Per (length, parity) three rows:
    DBL_MAX, DBL_MAX, -DBL_MAX straddling the first tile boundary of the block (+Inf only in element
    order), -0.0 / subnormal products on both sides of every boundary, and a last product of +Inf.
    -> (Built, {name: row})"""
    rng = np.random.default_rng(seed)
    tile = csr_tile()
    lengths = [tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1]
    n = 2 * tile + 64
    x = rng.standard_normal(n)
    x[n - 1] = INF
    out, inn, vals = [], [], []
    named = {}
    nnz, r = 0, 0
    for length in lengths:
        for parity in fmt_parities:
            for kind in ("order", "signs", "last_inf"):
                filler = 3 if (nnz + 3) % 2 == parity else 4
                for c in range(filler):  # filler row
                    out.append(r)
                    inn.append(c)
                    vals.append(float(rng.standard_normal()))
                nnz += filler
                r += 1
                cs = np.sort(rng.choice(n - 1, size=length, replace=False))
                v = rng.standard_normal(length)
                base = nnz & ~1
                bounds = [b - nnz for b in range(base + tile, nnz + length, tile)]  # row-relative tile starts
                if kind == "order":
                    k = bounds[0] if bounds else length - 1
                    k = max(k, 2)
                    v[k - 2], v[k - 1], v[k] = DBL_MAX, DBL_MAX, -DBL_MAX
                    x[cs[k - 2:k + 1]] = 1.0
                elif kind == "signs":
                    for b in bounds + [0, length]:
                        for k, s in ((b - 2, TINY), (b - 1, -0.0), (b, -0.0), (b + 1, MAX_SUB)):
                            if 0 <= k < length:
                                v[k] = s
                else:
                    cs[-1] = n - 1
                    cs = np.sort(cs)
                    v[-1] = 2.0
                for c, vv in zip(cs.tolist(), v.tolist()):
                    out.append(r)
                    inn.append(c)
                    vals.append(vv)
                named["%s/%d/%s" % (kind, length, "odd" if parity else "even")] = r
                nnz += length
                r += 1
    assert r < n
    return Built(n, out, inn, vals, x, {"tile": list(named.values())}), named


def special_vector(n, seed, kinds=ALL_SPECIALS, frac=0.2):
    """ordinary values (standard normals scaled by 10^[-3, 3]) with a fraction `frac` of the given kinds"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, size=n)
    sp = rng.random(n) < frac
    v[sp] = rng.choice(np.array(kinds, dtype=np.float64), size=int(sp.sum()))
    return v


def exact_pair(n, seed, kind):
    """two vectors whose dot product is exact in any order of summation:
    'int'      small integers (|a b| <= 64, sum < 2^53)
    'sub'      multiples of 2^-1074 times small integers, total below 2^-1022
    'negzero'  every product -0.0 (the exact value is 0: the result must be +0.0)"""
    rng = np.random.default_rng(seed)
    if kind == "int":
        return rng.integers(-8, 9, size=n).astype(np.float64), rng.integers(-8, 9, size=n).astype(np.float64)
    if kind == "sub":
        k = max(1, (2 ** 50) // (8 * max(n, 1)))  # |each product| <= 8 k 2^-1074: n of them stay below 2^-1022
        a = rng.integers(-k, k + 1, size=n).astype(np.float64) * TINY
        return a, rng.integers(-8, 9, size=n).astype(np.float64)
    if kind == "negzero":
        a = np.where(rng.random(n) < 0.5, -0.0, 0.0)
        b = np.where(a.view(np.uint64) != 0, 1.0, -1.0) * (1.0 + rng.integers(0, 4, size=n))
        return a, b
    raise ValueError(kind)
