"""Host checks of tests/_ieee.py (the comparison, the exact sums, the built inputs) and of
context.fdiv, which decides alpha and beta of the CG loop on the host."""
import itertools
import math

import numpy as np
import pytest

import _ieee as I
from _oracle import COO, CSR, OracleMatrix


def test_ieee_equal_is_bit_exact_except_nan_payloads():
    a = np.array([0.0, -0.0, I.TINY, I.INF, I.QNAN, 1.5])
    assert I.ieee_equal(a, a.copy())
    assert I.ieee_equal(a, np.array([0.0, -0.0, I.TINY, I.INF, I.NEG_QNAN, 1.5]))  # NaN sign / payload
    for i, other in ((0, -0.0), (1, 0.0), (2, 2 * I.TINY), (2, 0.0), (3, -I.INF), (4, 0.0), (5, np.nextafter(1.5, 2))):
        b = a.copy()
        b[i] = other
        assert not I.ieee_equal(a, b), (i, other)
        assert I.ieee_diff(a, b)[0][0] == i
    assert not I.ieee_equal(a, a[:-1])


def test_value_class():
    assert [I.value_class(v) for v in (1.0, -0.0, I.INF, -I.INF, I.QNAN)] == ["finite", "finite", "+inf", "-inf", "nan"]


def test_exact_sum_classes_and_values():
    assert I.exact_sum([1e16, 1.0, -1e16]) == 1.0
    assert math.isnan(I.exact_sum([I.INF, -I.INF]))
    assert math.isnan(I.exact_sum([1.0, I.QNAN]))
    assert I.exact_sum([I.INF, 1.0]) == I.INF and I.exact_sum([-I.INF, -1.0]) == -I.INF
    assert I.exact_sum([I.DBL_MAX, I.DBL_MAX, -I.DBL_MAX]) == I.DBL_MAX  # exact value is finite
    assert I.exact_sum([I.DBL_MAX, I.DBL_MAX]) == I.INF
    assert I.exact_sum([-I.DBL_MAX, -I.DBL_MAX]) == -I.INF
    assert I.exact_sum([I.TINY] * 5) == 5 * I.TINY
    for zeros in ([-0.0], [-0.0, -0.0], [1.0, -1.0], [-I.TINY, I.TINY], []):
        z = I.exact_sum(zeros)
        assert z == 0.0 and math.copysign(1.0, z) == 1.0, zeros


@pytest.mark.parametrize("kind", ["int", "sub", "negzero"])
@pytest.mark.parametrize("n", [1, 64, 4097])
def test_exact_pairs_sum_exactly_in_any_order(kind, n):
    a, b = I.exact_pair(n, 3, kind)
    p = a * b
    want = I.exact_sum(p)
    rng = np.random.default_rng(0)
    for _ in range(3):
        q = p[rng.permutation(n)]
        s = 0.0
        for v in q:
            s += v
        assert s == want
    if kind == "sub":
        assert np.abs(p).sum() < I.MIN_NORMAL
    if kind == "negzero":
        assert want == 0.0 and all(v == 0 and math.copysign(1, v) < 0 for v in p)


def test_sum_bound_holds_for_serial_sums():
    rng = np.random.default_rng(1)
    for n in (10, 1000, 100000):
        t = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, size=n)
        t = np.concatenate([t, -t[: n // 2] * (1 + 1e-9)])  # heavy cancellation
        s = 0.0
        for v in t.tolist():
            s += v
        assert abs(s - I.exact_sum(t)) <= I.sum_bound(t, len(t))


def test_depths_follow_the_kernel_shapes():
    assert I.csr_tile() == I.config_value("ABFT_BLOCK") * I.config_value("ABFT_CFG_CSR_EPT") > 0
    assert I.reduce_blocks(1) == 1 and I.reduce_blocks(2048) == 1 and I.reduce_blocks(2049) == 2
    assert I.reduce_blocks(1 << 30) == I.config_value("ABFT_CFG_MAX_PARTIALS")
    assert I.dot_depth(1) == 2 + 8 + 1 + 8
    assert I.finalize_depth(8192) == 4 + 2 + 6 + 16
    assert I.finalize_depth(8193) == 2 + 2 + 8 + 1 + 8  # 5 workgroups of 1639 partials


@pytest.mark.parametrize("fmt", [CSR, COO])
def test_special_matrix_rows_give_what_they_were_built_for(fmt):
    B = I.special_matrix()
    y = OracleMatrix(fmt, "none", *B.mat(fmt)).spmv(B.x)
    c = B.crafted
    for r in c["negzero"] + c["empty"]:
        assert y[r] == 0.0 and math.copysign(1.0, y[r]) == 1.0, r
    for r in c["inf_ninf"] + c["zero_nan"]:
        assert math.isnan(y[r]), r
    assert [y[r] for r in c["max_order"]] == [I.INF, -I.INF]
    for r in c["subnormal"]:
        t = B.row_terms(r)
        assert 0 < abs(y[r]) < I.MIN_NORMAL * 64 and y[r] == I.exact_sum(t)
    for r in c["last_inf"]:
        assert math.isinf(y[r]) and y[r] == B.row_terms(r)[-1], r
    for r in c["edge"]:
        assert y[r] in (I.INF, 0.0) or np.isfinite(y[r])
    finite = np.isfinite(y)
    assert finite.mean() > 0.95  # most rows finite: the bit-exact check of those rows means something
    # every kind of value is in the matrix and in x
    for v in (0.0, I.TINY, I.MAX_SUB, I.MIN_NORMAL, I.DBL_MAX, 1e-200):
        assert np.any(np.abs(B.vals) == v) or np.any(np.abs(B.x) == v), v
    for v in (-0.0, I.INF, -I.INF):
        assert np.any(B.x.view(np.uint64) == np.float64(v).view(np.uint64))
    assert np.any(np.isnan(B.x))


def test_tile_edge_rows_sit_where_they_should():
    T, named = I.tile_edge_matrix()
    tile = I.csr_tile()
    c, r, v, n = T.csr()
    rowptr = np.searchsorted(r, np.arange(n + 1))
    y = OracleMatrix(CSR, "none", c, r, v, n).spmv(T.x)
    for name, row in named.items():
        kind, length, parity = name.split("/")
        e0, e1 = rowptr[row], rowptr[row + 1]
        assert e1 - e0 == int(length) and e0 % 2 == (parity == "odd"), name
        assert int(length) in (tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1)
        if kind in ("order", "last_inf"):
            assert y[row] == I.INF, name
        else:
            assert np.isfinite(y[row]), name


SIGNED = [float(v) for v in (0.0, -0.0, I.TINY, -I.TINY, 1.0, -1.0, I.DBL_MAX, -I.DBL_MAX, I.INF, -I.INF, float("nan"))]


def test_fdiv_is_ieee_division():
    """on Python floats, as cg_solve passes them (the values of ctypes doubles)"""
    from abft_sparse_cg_amd.context import fdiv
    for a, b in itertools.product(SIGNED, SIGNED):
        with np.errstate(all="ignore"):
            want = np.float64(a) / np.float64(b)
        got = fdiv(a, b)
        assert I.ieee_equal([got], [want]), (a, b, got, want)
