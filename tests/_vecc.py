"""numpy model of the protected vector element -- the (64, 57) SECDED code in a double's low 7
bits -- and of the four protected CG operations.  Written from the rule in
the text, not from the device code: data bit d = 7..63 takes the next Hamming position that is no
power of two, from 3 on; check bit k (position 2^k) sits in bit 1 + k; bit 0 is the overall parity.
Every sum here is serial, in element order, with separate multiply and add."""
import numpy as np

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


def salted(n, seed):
    """random doubles salted with +-0, subnormals, +-inf, a quiet NaN and a NaN whose payload lies in bits 0..6 only"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
    special = np.array([0.0, -0.0, 5e-324, -2.5e-310, np.inf, -np.inf, np.nan], np.float64)
    special = np.concatenate([special, np.array([0x7FF0000000000041], U).view(np.float64)])
    at = rng.permutation(n)[:min(n, len(special))]
    v[at] = special[:len(at)]
    return v
