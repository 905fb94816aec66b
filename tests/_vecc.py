"""numpy model of the protected vector element -- the (64, 57) SECDED code in a double's low 7
bits -- and of the four protected CG operations.  Written from the rule in
the text, not from the device code: data bit d = 7..63 takes the next Hamming position that is no
power of two, from 3 on; check bit k (position 2^k) sits in bit 1 + k; bit 0 is the overall parity.
Every sum here is serial, in element order, with separate multiply and add."""
import os
import re

import numpy as np

import _ieee as I

U = np.uint64
CODE = U(0x7F)


def _masks():
    out, pos = [1 << (1 + k) for k in range(6)], 3
    for d in range(7, 64):
        while pos & (pos - 1) == 0:
            pos += 1
        for k in range(6):
            if (pos >> k) & 1:
                out[k] |= 1 << d
        pos += 1
    assert pos == 64
    return [U(m) for m in out]


MASKS = _masks()
# Hamming position -> bit of the word
BIT_OF_POSITION = {}
for _k in range(6):
    BIT_OF_POSITION[1 << _k] = 1 + _k
_pos = 3
for _d in range(7, 64):
    while _pos & (_pos - 1) == 0:
        _pos += 1
    BIT_OF_POSITION[_pos] = _d
    _pos += 1


def words(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(U).copy()


def parity(w):
    w = np.asarray(w, dtype=U).copy()
    for s in (32, 16, 8, 4, 2, 1):
        w ^= w >> U(s)
    return (w & U(1)).astype(np.int64)


def syndrome(w):
    w = np.asarray(w, dtype=U)
    s = np.zeros(w.shape, np.int64)
    for k in range(6):
        s |= parity(w & MASKS[k]) << k
    return s


def strip(a):
    """stored words (or a downloaded array of them) -> the values: bits 0..6 cleared"""
    a = np.asarray(a)
    w = a if a.dtype == U else np.ascontiguousarray(a, dtype=np.float64).view(U)
    return (w & ~CODE).view(np.float64)


def encode(values):
    """doubles -> stored words"""
    v = np.ascontiguousarray(values, dtype=np.float64)
    w = v.view(U) & ~CODE
    lost = np.isnan(v) & ((w & U(0x000FFFFFFFFFFFFF)) == 0)  # a NaN whose payload was cut off
    w = np.where(lost, w | U(1 << 51), w)
    for k in range(6):
        w = w | (parity(w & MASKS[k]).astype(U) << U(1 + k))
    return w | parity(w).astype(U)


def decode(stored):
    """-> (words after repair, status, bit): status 0 clean, 1 one flipped bit (repaired; `bit` is
    the one), 2 two flipped bits (the word unchanged, bit -1)"""
    w = np.asarray(stored, dtype=U).copy()
    s, p = syndrome(w), parity(w)
    status = np.where(p == 1, 1, np.where(s != 0, 2, 0))
    bit = np.full(w.shape, -1, np.int64)
    for i in np.flatnonzero(status == 1):
        bit.flat[i] = BIT_OF_POSITION[int(s.flat[i])] if s.flat[i] else 0
        w.flat[i] ^= U(1 << int(bit.flat[i]))
    return w, status, bit


def value(stored):
    """what a kernel computes with: the repaired word without its code bits"""
    return strip(decode(stored)[0])


def serial_sum(terms):
    acc = 0.0
    for t in np.asarray(terms, dtype=np.float64):
        acc = acc + t
    return float(acc)


def dot(aw, bw):
    with np.errstate(all="ignore"):
        return serial_sum(value(aw) * value(bw))


def csr_of(cols, rows, vals, n):
    """caller-order triplets (rows ascending) -> (rowptr, cols, vals)"""
    rows = np.asarray(rows, dtype=np.int64)
    assert np.all(np.diff(rows) >= 0)
    rowptr = np.zeros(n + 1, np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr), np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.float64)


def spmv(rowptr, cols, vals, xw):
    """-> (stored words of y, the fused product sum value(x[row]) * strip(y[row]) as a serial sum)"""
    x = value(xw)
    n = len(rowptr) - 1
    acc = np.zeros(n)
    length = np.diff(rowptr)
    with np.errstate(all="ignore"):
        for k in range(int(length.max()) if n else 0):
            live = np.flatnonzero(length > k)
            e = rowptr[live] + k
            acc[live] = acc[live] + vals[e] * x[cols[e]]
        yw = encode(acc)
        return yw, serial_sum(x[:n] * strip(yw))


def calc_xr(xw, rw, pw, ww, alpha):
    """-> (x words, r words, r.r over the stored r)"""
    with np.errstate(all="ignore"):
        xs = encode(value(xw) + alpha * value(pw))
        rs = encode(value(rw) - alpha * value(ww))
        return xs, rs, serial_sum(strip(rs) * strip(rs))


def calc_p(pw, rw, beta):
    with np.errstate(all="ignore"):
        return encode(value(rw) + beta * value(pw))


def assert_words(got, want, what=""):
    """The comparison rule for stored words.  Where the model's value is no NaN the whole word -- value
    bits and the 7 code bits -- equals the model's; where it is a NaN the device's value is one too (sign
    and payload open: x86 and the GPU return different default NaNs), in the same places and nowhere else;
    and every stored word, NaN or not, is a codeword."""
    got, want = np.asarray(got, dtype=U), np.asarray(want, dtype=U)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(strip(want))
    got_nan = np.isnan(strip(got))
    assert np.array_equal(got_nan, nan), (what, "NaNs at", np.flatnonzero(got_nan != nan)[:8].tolist())
    bad = np.flatnonzero((got != want) & ~nan)
    assert bad.size == 0, (what, [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]])
    status = decode(got)[1]
    assert not status.any(), (what, "no codewords at", np.flatnonzero(status)[:8].tolist())


def salted(n, seed):
    """random doubles salted with +-0, subnormals, +-inf, a quiet NaN and a NaN whose payload lies in bits 0..6 only"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
    special = np.array([0.0, -0.0, 5e-324, -2.5e-310, np.inf, -np.inf, np.nan], np.float64)
    special = np.concatenate([special, np.array([0x7FF0000000000041], U).view(np.float64)])
    at = rng.permutation(n)[:min(n, len(special))]
    v[at] = special[:len(at)]
    return v


# ------------------------------------------------------------------------------------------------
# Inputs of the edge tests: test_vector_ecc_edges_host.py checks them and the model on them without
# a GPU, test_gpu_vector_ecc_edges.py runs the kernels on them.

INF, NAN = float("inf"), float("nan")
T = I.TINY  # 2^-1074
HUGE = I.f64(0x7FEFFFFFFFFFFF80)  # 0x1.fffffffffff80p+1023: DBL_MAX with bits 0..6 clear
EDGE_LENGTHS = [1, 2, 3, 255, 257, 4099]
SCALARS = [0.37251, -1.0, 0.0, -0.0, 5e-324, 1e308, INF, -INF, NAN]  # alpha and beta
_FINITE = I.FINITE_SPECIALS + [1e200, -1e200]
_HUGE = _FINITE + [HUGE, -HUGE, 2.0 ** 1023, -2.0 ** 1023]
# family -> the kinds mixed into ordinary values; each adds to the one before it
FAMILIES = {"finite": _FINITE, "huge": _HUGE, "inf": _HUGE + [INF, -INF],
            "nan": _HUGE + [INF, -INF, I.QNAN, I.NEG_QNAN]}


def operand_seed(n, k):
    """the seed of operand k (x, r, p, w) of the special-value calls at length n"""
    return 1000 * n + k


def family(name, n, seed):
    """stored words of a vector of the family: ordinary values with a fifth of the family's kinds, encoded"""
    return encode(I.special_vector(n, seed, kinds=FAMILIES[name]))


# (x, p, alpha, the value calc_xr stores in x, what a wrong kernel would get wrong).  The same rows drive
# r -= alpha w with w = -p, and p' = r + beta p with r = x and beta = alpha.
CRAFTED = [
    (1.0, 2.0 ** -46, 1.0, 1.0, "truncation, not rounding"),
    (-1.0, -2.0 ** -46, 1.0, -1.0, "toward zero, not downward"),
    (1.0, 2.0 ** -45, 1.0, 1.0 + 2.0 ** -45, "the lowest kept bit survives"),
    (0.0, 128 * T, 0.5, 0.0, "a subnormal below the cut"),
    (-0.0, -128 * T, 0.5, -0.0, "the sign of a truncated zero"),
    (1.5, -1.5, 1.0, 0.0, "exact cancellation"),
    (-(1.0 + 2.0 ** -29), 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, 0.0, "separate multiply and add: an FMA leaves 2^-60"),
    (INF, -INF, 1.0, NAN, "Inf - Inf"),
    (1.0, INF, 0.0, NAN, "0 * Inf"),
    (HUGE, HUGE, 1.0, INF, "overflow"),
]


def crafted_positions(n):
    """0, 1, n - 2, n - 1 where n allows"""
    out = []
    for i in (0, 1, n - 2, n - 1):
        if 0 <= i < n and i not in out:
            out.append(i)
    return out


def crafted_calls(n):
    """the crafted rows as calls on a vector of n elements: [(alpha, {index: row of CRAFTED})], the rows of
    one alpha dealt cyclically over crafted_positions(n), a new call when the positions are used up"""
    at = crafted_positions(n)
    calls = []
    for alpha in sorted({row[2] for row in CRAFTED}):
        rows = [row for row in CRAFTED if row[2] == alpha]
        for k in range(0, len(rows), len(at)):
            calls.append((alpha, dict(zip(at, rows[k:k + len(at)]))))
    return calls


# A3: n = 4099 -- 3 workgroups, chains of 2-3 steps a thread at VEC == 2 and of 5-6 at VEC == 1
FLIP_N = 4099
SWEEP = [(61 * j + 5, j) for j in range(64)]  # (index, bit): every bit of the word, each in an element of its own
WALK = list(zip([0, 1, 2, 1535, 1536, 1537, 3072, 3073, 4096, 4097, 4098], [0, 3, 63, 7, 30, 51, 55, 62, 1, 6, 40]))


def walk_class(i, n, vec):
    """where the vector kernels (kernels.hip: first = (block * 256 + thread) * VEC, stride = grid * 256 * VEC, a
    pair where VEC == 2 and i + 1 < n) meet element i: (workgroup, thread of the grid, round of that thread,
    'first' / 'second' of a pair or 'single')"""
    stride = I.reduce_blocks(n) * 256 * vec
    base = i - i % vec
    half = "single" if vec == 1 or base + 1 >= n else ("first", "second")[i - base]
    thread = (base % stride) // vec
    return thread // 256, thread, base // stride, half


# A5: 66 workgroups: ticket groups of 32, 32 and 2
MANY_N = 65 * 2048 + 1
MANY_FLIPS = [(0, 17), (65535, 0), (65536, 63), (MANY_N - 1, 4)]  # (index, bit)


def event_cap():
    """EVENT_CAP of abft_hip.hip: the slots of the device event queue"""
    with open(os.path.join(I.ROOT, "abft_sparse_cg_amd", "csrc", "abft_hip.hip")) as f:
        m = re.search(r"EVENT_CAP\s*=\s*1u\s*<<\s*(\d+)\s*;", f.read())
    assert m
    return 1 << int(m.group(1))


def arrow(n, dense=1, seed=11):
    """lower arrow: row 0 is (0, 0), row i > 0 is (i, 0), (i, i); with dense == 2 column 1 is dense as well:
    (i, 1) in every row i > 1.  Random values.  -> (cols, rows, vals, n), rows and the columns inside a row ascending"""
    i = np.arange(n, dtype=np.int64)
    parts = [(i[1:], np.zeros(n - 1, np.int64))]
    if dense == 2:
        parts.append((i[2:], np.ones(n - 2, np.int64)))
    parts.append((i, i))
    rows, cols = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    order = np.lexsort((cols, rows))
    vals = np.random.default_rng(seed).standard_normal(len(rows))
    return cols[order].astype(np.uint32), rows[order].astype(np.uint32), vals, n


def arrow_spd(n):
    """symmetric arrow a_00 = n, a_ii = 4, a_i0 = a_0i = 0.5: SPD by diagonal dominance; row 0 is one long row"""
    i = np.arange(1, n, dtype=np.int64)
    rows = np.concatenate([np.zeros(n, np.int64), i, i])
    cols = np.concatenate([np.arange(n, dtype=np.int64), np.zeros(n - 1, np.int64), i])
    vals = np.concatenate([[float(n)], np.full(n - 1, 0.5), np.full(n - 1, 0.5), np.full(n - 1, 4.0)])
    order = np.lexsort((cols, rows))
    return cols[order].astype(np.uint32), rows[order].astype(np.uint32), vals[order], n
