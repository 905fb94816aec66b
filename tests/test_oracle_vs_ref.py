"""Pins oracle/abft_oracle.c against the REFERENCE's own CPUContext objects
(oracle/_ref/, built from the reference tree by oracle/Makefile).  Where that
build is absent, the reference's side of every comparison comes from
tests/golden/oracle_vs_ref.npz: what the same calls returned in the reference
build, recorded with

    ABFT_RECORD_REF=1 python -m pytest tests/test_oracle_vs_ref.py

(which needs oracle/_ref and rewrites the fixture)."""
import json
import os

import numpy as np
import pytest

from _capture import run_captured
from _oracle import (COO, CSR, MODES, Oracle, OracleMatrix, Ref, event_lines, have_ref, laplace5,
                     ora_calc_p, ora_calc_xr, ora_dot, random_spd, ref_cg, ref_flip_spmv, ref_inject_rand, rhs)

pytestmark = pytest.mark.ref

STORE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vs_ref.npz")
RECORD = os.environ.get("ABFT_RECORD_REF") == "1"
_recorded = {}
_stored = None


def _pack(obj, arrays):
    """nested tuples / lists of arrays and scalars -> JSON-able tree; arrays go to `arrays`, a leaf names its dtype,
    its shape and the earlier array of the same dtype and shape it is stored against (-1: none)"""
    if isinstance(obj, np.ndarray):
        obj = np.ascontiguousarray(obj)
        base = max((i for i, a in enumerate(arrays) if a.dtype == obj.dtype and a.shape == obj.shape), default=-1)
        arrays.append(obj)
        return {"@": [obj.dtype.str, list(obj.shape), base]}
    if isinstance(obj, (list, tuple)):
        return [_pack(v, arrays) for v in obj]
    if isinstance(obj, np.generic):
        return obj.item()
    return obj


def _leaves(tree):
    if isinstance(tree, dict):
        yield tree["@"]
    elif isinstance(tree, list):
        for v in tree:
            yield from _leaves(v)


def _unpack(tree, it):
    if isinstance(tree, dict):
        return next(it)
    if isinstance(tree, list):
        return [_unpack(v, it) for v in tree]
    return tree


def _write_store(records):
    """Every array is stored as its bytes XOR those of its base (the results of neighbouring cases differ in a few
    elements), all in one compressed blob."""
    arrays = []
    tree = {k: _pack(v, arrays) for k, v in sorted(records.items())}
    raw = [np.frombuffer(a.tobytes(), dtype=np.uint8) for a in arrays]
    leaves = [l for k in sorted(tree) for l in _leaves(tree[k])]
    blob = [r ^ raw[base] if base >= 0 else r for r, (_, _, base) in zip(raw, leaves)]
    np.savez_compressed(STORE, tree=np.frombuffer(json.dumps(tree, sort_keys=True).encode(), dtype=np.uint8),
                        blob=np.concatenate(blob) if blob else np.zeros(0, np.uint8))


def _read_store():
    with np.load(STORE) as z:
        tree, blob = json.loads(z["tree"].tobytes().decode()), z["blob"]
    leaves = [l for k in sorted(tree) for l in _leaves(tree[k])]
    raw, off = [], 0
    for dt, shape, base in leaves:
        n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
        raw.append(blob[off:off + n] ^ raw[base] if base >= 0 else blob[off:off + n])
        off += n
    assert off == len(blob)
    it = iter(np.frombuffer(r.tobytes(), dtype=dt).reshape(shape) for r, (dt, shape, _) in zip(raw, leaves))
    return {k: _unpack(tree[k], it) for k in sorted(tree)}


def ref_side(key, fn, *args):
    """The reference's result of fn(*args): computed live where oracle/_ref is built, else the recorded one."""
    if have_ref():
        res = fn(*args)
        if RECORD:
            _recorded[key] = res
        return res
    global _stored
    if _stored is None:
        _stored = _read_store()
    return _stored[key]


@pytest.fixture(scope="module", autouse=True)
def _record_store():
    yield
    if RECORD and _recorded:
        assert have_ref()
        _write_store(_recorded)


FMTS = [CSR, COO]
NBITS = {CSR: 96, COO: 128}


def _rand_words(fmt, rng):
    n = 3 if fmt == CSR else 4
    w = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    ew = 2 if fmt == CSR else 0
    w[ew] &= 0x00FFFFFF
    return w


@pytest.mark.parametrize("fmt", FMTS)
def test_syndrome_parity_match_reference_on_random_words(fmt):
    rng = np.random.default_rng(7)
    n = 3 if fmt == CSR else 4
    words = [rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32) for _ in range(2000)]

    def ref_words():
        import ctypes
        L = Ref.lib(fmt)
        ptrs = [w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) for w in words]
        return [L.ref_ecc_syndrome(p) for p in ptrs], [L.ref_ecc_parity(p) for p in ptrs]

    syn, par = ref_side("syndrome_parity/%d" % fmt, ref_words)
    for w, s, p in zip(words, syn, par):
        assert Oracle.syndrome(fmt, w) == s
        assert Oracle.parity(fmt, w) == p


@pytest.mark.parametrize("fmt", FMTS)
def test_flipped_bit_matches_reference_for_every_syndrome(fmt):
    syns = []
    for h in range(1, 128):
        s = 0
        for p in range(1, 8):
            if (h >> (p - 1)) & 1:
                s |= 1 << (32 - p)
        syns.append(s)
    bits = ref_side("flipped_bit/%d" % fmt, lambda: [Ref.lib(fmt).ref_ecc_flipped_bit(s) for s in syns])
    for h, s, b in zip(range(1, 128), syns, bits):
        assert Oracle.flipped_bit(fmt, s) == b, h


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("mode", MODES)
def test_encoded_matrix_identical(fmt, mode):
    cols, rows, vals, n = random_spd(60, 6, seed=3)
    o = OracleMatrix(fmt, mode, cols, rows, vals, n)

    def ref_encoded():
        r = Ref(fmt, mode, cols, rows, vals, n)
        return r.stored_words(), (r.rowptr() if fmt == CSR else None)

    words, rowptr = ref_side("encoded/%d/%s" % (fmt, mode), ref_encoded)
    assert np.array_equal(o.stored_words(), words)
    if fmt == CSR:
        assert np.array_equal(o.csr_arrays()[1], rowptr)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("mode", MODES)
def test_spmv_bit_identical_no_faults(fmt, mode):
    for i, mat in enumerate((laplace5(9, 7), random_spd(80, 8, seed=5))):
        cols, rows, vals, n = mat
        x = rhs(n, 11) - 0.5
        o = OracleMatrix(fmt, mode, cols, rows, vals, n)
        code, text, ((y_ref,), _) = ref_side("spmv/%d/%s/%d" % (fmt, mode, i), run_captured, ref_flip_spmv, fmt, mode, mat,
                                             0, [], x, 1)
        assert code == 0 and text == ""
        y = o.spmv(x)
        assert np.array_equal(y.view(np.uint64), y_ref.view(np.uint64))
        assert o.events() == ([], False)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("mode", ["sed", "sec7", "sec8", "secded"])
def test_every_single_flip_same_events_and_result(fmt, mode):
    mat = random_spd(24, 4, seed=9)
    cols, rows, vals, n = mat
    x = rhs(n, 2) + 0.25
    index = len(vals) // 2
    for bit in range(NBITS[fmt]):
        code, text, res = ref_side("single_flip/%d/%s/%d" % (fmt, mode, bit), run_captured, ref_flip_spmv, fmt, mode, mat,
                                   index, [bit], x)
        o = OracleMatrix(fmt, mode, cols, rows, vals, n)
        o.inject(index, [bit])
        y1 = o.spmv(x)
        ev, fatal = o.events()
        lines = event_lines(ev, fmt)
        if fatal:
            assert code == 1, (bit, text)
            assert text == "".join(lines)
        else:
            assert code == 0, (bit, text)
            y2 = o.spmv(x)
            ev2, _ = o.events()
            assert text == "".join(lines + event_lines(ev2, fmt)), bit
            (r1, r2), words = res
            assert np.array_equal(y1.view(np.uint64), r1.view(np.uint64)), bit
            assert np.array_equal(y2.view(np.uint64), r2.view(np.uint64)), bit
            assert np.array_equal(o.stored_words(), words), bit


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("mode", ["sec8", "secded"])
def test_double_flips_same_behaviour(fmt, mode):
    mat = random_spd(24, 4, seed=10)
    cols, rows, vals, n = mat
    x = rhs(n, 3) + 0.25
    index = 7
    rng = np.random.default_rng(1)
    for _ in range(60):
        b1, b2 = rng.choice(NBITS[fmt], size=2, replace=False)
        # a double flip that changes the gather index beyond the vector is UB in the reference
        code, text, res = ref_side("double_flip/%d/%s/%d_%d" % (fmt, mode, b1, b2), run_captured, ref_flip_spmv, fmt, mode,
                                   mat, index, [b1, b2], x, 1)
        o = OracleMatrix(fmt, mode, cols, rows, vals, n)
        o.inject(index, [b1, b2])
        y = o.spmv(x)
        ev, fatal = o.events()
        if mode == "secded":
            assert fatal and code == 1
            assert text == "[ECC] double-bit error detected\n" == "".join(event_lines(ev, fmt))
        else:
            assert not fatal and ev == []  # sec8 is blind to double flips (parity 0)
            if code == 0:
                assert text == ""


@pytest.mark.parametrize("fmt", FMTS)
def test_constraints_violations_match(fmt):
    mat = random_spd(30, 6, seed=4)
    cols, rows, vals, n = mat
    x = rhs(n, 5)
    idx_bits = range(64, 96) if fmt == CSR else range(0, 64)
    hit = 0
    for index in (0, 5, len(vals) - 1, len(vals) // 3):
        for bit in idx_bits:
            code, text, res = ref_side("constraints/%d/%d/%d" % (fmt, index, bit), run_captured, ref_flip_spmv, fmt,
                                       "constraints", mat, index, [bit], x, 1)
            if code not in (0, 1):
                continue  # reference faulted on an out-of-range gather before any check fired
            o = OracleMatrix(fmt, "constraints", cols, rows, vals, n)
            o.inject(index, [bit])
            y = o.spmv(x)
            ev, fatal = o.events()
            assert (code == 1) == fatal, (index, bit, text)
            assert text == "".join(event_lines(ev, fmt)), (index, bit)
            if not fatal:
                assert np.array_equal(y.view(np.uint64), res[0][0].view(np.uint64))
            hit += fatal
    assert hit > 20


def test_vector_kernels_bit_identical():
    cols, rows, vals, n = laplace5(5, 5)
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(1000), rng.standard_normal(1000)
    x1, r1, p1, w1 = (rng.standard_normal(1000) for _ in range(4))

    def ref_vectors():
        r = Ref(CSR, "none", cols, rows, vals, n)
        x2, r2, p2 = x1.copy(), r1.copy(), p1.copy()
        d = r.dot(a, b)
        rr = r.calc_xr(x2, r2, p1, w1, 0.37)
        r.calc_p(p2, r2, 1.7)
        return d, rr, x2, r2, p2

    d, rr, x2, r2, p2 = ref_side("vector_kernels", ref_vectors)
    assert ora_dot(a, b) == d
    assert ora_calc_xr(x1, r1, p1, w1, 0.37) == rr
    assert np.array_equal(x1, x2) and np.array_equal(r1, r2)
    ora_calc_p(p1, r1, 1.7)
    assert np.array_equal(p1, p2)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("mode", MODES)
def test_cg_history_bit_identical(fmt, mode):
    mat = laplace5(16, 16)
    cols, rows, vals, n = mat
    b = rhs(n, 1)
    o = OracleMatrix(fmt, mode, cols, rows, vals, n)
    it_o, h_o, x_o, fatal = o.cg(b)
    code, text, (it_r, h_r, x_r) = ref_side("cg/%d/%s" % (fmt, mode), run_captured, ref_cg, fmt, mode, mat, b)
    assert code == 0 and not fatal
    assert it_o == it_r and it_o > 10
    assert np.array_equal(h_o.view(np.uint64), h_r.view(np.uint64))
    assert np.array_equal(x_o.view(np.uint64), x_r.view(np.uint64))


@pytest.mark.parametrize("fmt", FMTS)
def test_inject_rand_draws_like_reference(fmt):
    """Same libc rand() sequence -> same element and bits as inject_bitflip."""
    import ctypes
    libc = ctypes.CDLL(None)
    mat = random_spd(30, 6, seed=12)
    cols, rows, vals, n = mat

    for kind in (0, 1, 2):
        for flips in (1, 2, 3):
            code, text, words = ref_side("inject_rand/%d/%d/%d" % (fmt, kind, flips), run_captured, ref_inject_rand, fmt, mat,
                                         1234, kind, flips)
            assert code == 0
            libc.srand(1234)
            o = OracleMatrix(fmt, "none", cols, rows, vals, n)
            idx, bits = o.inject_rand(kind, flips)
            assert text == "".join("*** flipping bit %d at index %d ***\n" % (b, idx) for b in bits)
            assert np.array_equal(o.stored_words(), words)


# ---- IEEE special values (tests/_ieee.py): both sides on the x86 host, so every bit is compared, NaN bits included

def _special():
    import _ieee
    return _ieee.special_matrix(n=300, seed=1, long_len=260, boundaries=(16, 64, 257))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("mode", MODES)
def test_spmv_special_values_bit_identical(fmt, mode):
    B = _special()
    mat = B.mat(fmt)
    o = OracleMatrix(fmt, mode, *mat)
    code, text, ((r1, r2), words) = ref_side("special_spmv/%d/%s" % (fmt, mode), run_captured, ref_flip_spmv, fmt, mode,
                                             mat, 0, [], B.x, 2)
    assert code == 0 and text == ""
    assert np.array_equal(o.stored_words(), words)  # ECC words of NaN, Inf and subnormal values too
    y1, y2 = o.spmv(B.x), o.spmv(B.x)
    assert np.array_equal(y1.view(np.uint64), r1.view(np.uint64))
    assert np.array_equal(y2.view(np.uint64), r2.view(np.uint64))
    assert np.isnan(y1).any() and np.isinf(y1).any() and (y1.view(np.uint64) == 0).any()
    assert o.events() == ([], False)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("mode", ["sec7", "secded"])
def test_flip_on_nonfinite_value_same_repair(fmt, mode):
    B = _special()
    mat = B.mat(fmt)
    vals = mat[2]
    vbit0 = 0 if fmt == CSR else 64
    for index in np.flatnonzero(~np.isfinite(vals)).tolist():
        for bit in (vbit0 + 3, vbit0 + 51, vbit0 + 63):
            code, text, res = ref_side("special_flip/%d/%s/%d/%d" % (fmt, mode, index, bit), run_captured, ref_flip_spmv,
                                       fmt, mode, mat, index, [bit], B.x)
            o = OracleMatrix(fmt, mode, *mat)
            o.inject(index, [bit])
            y1 = o.spmv(B.x)
            ev1, fatal = o.events()
            y2 = o.spmv(B.x)
            ev2, _ = o.events()
            assert code == 0 and not fatal and len(ev1) == 1
            assert ev2 == [] and text == "".join(event_lines(ev1, fmt)), (index, bit)  # repaired once, written back
            (r1, r2), words = res
            assert np.array_equal(y1.view(np.uint64), r1.view(np.uint64))
            assert np.array_equal(y2.view(np.uint64), r2.view(np.uint64))
            assert np.array_equal(o.stored_words(), words)


def test_vector_kernels_special_values_bit_identical():
    import _ieee
    cols, rows, vals, n = laplace5(5, 5)
    m = 777
    # no NaN inputs here: x86 returns the first operand's payload when both are NaN, and the two builds may
    # commute a reduction's add, so a NaN input payload beside a generated default NaN has no fixed bits
    kinds = [v for v in _ieee.ALL_SPECIALS if v == v]
    a, b, x1, r1, p1, w1 = (_ieee.special_vector(m, s, kinds) for s in range(6))
    ia, ib = _ieee.exact_pair(m, 1, "negzero")
    sa, sb = _ieee.exact_pair(m, 2, "sub")

    def ref_vectors():
        r = Ref(CSR, "none", cols, rows, vals, n)
        # scalars as arrays: the fixture keeps an array's bytes, a scalar only as a JSON number
        out = [np.array([r.dot(a, b), r.dot(ia, ib), r.dot(sa, sb)])]
        for alpha, beta in ((0.37, 1.7), (-0.0, _ieee.INF), (_ieee.INF, -0.0)):
            x2, r2, p2 = x1.copy(), r1.copy(), p1.copy()
            rr = r.calc_xr(x2, r2, p1, w1, alpha)
            r.calc_p(p2, r2, beta)
            out.append((np.array([rr]), x2, r2, p2))
        return out

    got = ref_side("special_vectors", ref_vectors)
    with np.errstate(all="ignore"):
        assert np.array_equal(np.asarray(got[0]).view(np.uint64),
                              np.array([ora_dot(a, b), ora_dot(ia, ib), ora_dot(sa, sb)]).view(np.uint64))
        for (alpha, beta), (rr, x2, r2, p2) in zip(((0.37, 1.7), (-0.0, _ieee.INF), (_ieee.INF, -0.0)), got[1:]):
            x3, r3, p3 = x1.copy(), r1.copy(), p1.copy()
            rr3 = ora_calc_xr(x3, r3, p1, w1, alpha)
            ora_calc_p(p3, r3, beta)
            assert np.array_equal(np.array([rr3]).view(np.uint64), np.asarray(rr).view(np.uint64))
            for mine, theirs in ((x3, x2), (r3, r2), (p3, p2)):
                assert np.array_equal(mine.view(np.uint64), theirs.view(np.uint64))
