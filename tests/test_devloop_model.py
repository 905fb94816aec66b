"""tests/_devloop.model_iteration, the reference the GPU tests of the device-scalar CG loop rest on, against the
oracle's calc_xr / calc_p (oracle/abft_oracle.c, itself compared with the reference's CPUContext): the vectors bit
for bit on the same scalars, the terms of both reductions against the exact sum.  No GPU."""
import numpy as np
import pytest

import _ieee as I
from _devloop import model_iteration
from _oracle import CSR, OracleMatrix, laplace5, ora_calc_p, ora_calc_xr, random_spd, rhs

SYSTEMS = {"laplace9x7": lambda: laplace5(9, 7), "random300": lambda: random_spd(300, 5, seed=5)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_model_iteration_equals_the_oracle(name):
    cols, rows, vals, n = SYSTEMS[name]()
    o = OracleMatrix(CSR, "none", cols, rows, vals, n)
    b = rhs(n, 3)
    x, r, p = np.zeros(n), b.copy(), b.copy()
    rr = float(np.dot(r, r))
    for it in range(5):
        # the oracle's own iteration: serial sums, alpha and beta the quotients of ITS scalars
        w = o.spmv(p)
        pw = float(np.dot(p, w))
        alpha = float(np.float64(rr) / np.float64(pw))
        xo, ro, po = x.copy(), r.copy(), p.copy()
        rr_new = ora_calc_xr(xo, ro, po, w, alpha)
        beta = float(np.float64(rr_new) / np.float64(rr))
        ora_calc_p(po, ro, beta)
        keep = [v.copy() for v in (x, r, p)]
        m = model_iteration(o, x, r, p, 0, np.full(n, np.nan), rr, pw, rr_new)
        for v, k in zip((x, r, p), keep):  # the inputs stay as they were
            assert np.array_equal(bits(v), bits(k))
        assert m.alpha == alpha and m.beta == beta
        for got, want in ((m.w, w), (m.x, xo), (m.r, ro), (m.p, po)):
            assert np.array_equal(bits(got), bits(want)), it
        # the terms: those of the two sums, and any summation of them lands within the bound of a tree of the
        # kernels' depth around the exact sum
        assert np.array_equal(bits(m.pw_terms), bits(p * w)) and np.array_equal(bits(m.rr_terms), bits(ro * ro))
        for terms, ser in ((m.pw_terms, pw), (m.rr_terms, rr_new)):
            ex = I.exact_sum(terms)
            bound = I.sum_bound(terms, I.dot_depth(n))
            assert abs(float(np.dot(terms, np.ones(n))) - ex) <= bound
            assert abs(ser - ex) <= I.sum_bound(terms, n)  # (the oracle's serial sum: depth n)
        x, r, p, rr = m.x, m.r, m.p, rr_new
    assert rr < float(np.dot(b, b))


def test_model_iteration_on_a_window_of_the_gathered_vector():
    """p a window of a longer vector (a shard): the product's terms and the updates use the window only"""
    cols, rows, vals, n = random_spd(300, 5, seed=5)
    lo, hi, off, n_pad = 100, 200, 131, 400
    m_rows = (rows >= lo) & (rows < hi)
    pin = np.where(cols < 150, cols, cols + 100).astype(np.uint32)[m_rows]  # columns spread over the padded input
    o = OracleMatrix(CSR, "none", pin, (rows[m_rows] - lo).astype(np.uint32), vals[m_rows], hi - lo, n_in=n_pad)
    rng = np.random.default_rng(8)
    p_full = rng.standard_normal(n_pad)
    x, r = rng.standard_normal(hi - lo), rng.standard_normal(hi - lo)
    m = model_iteration(o, x, r, p_full, off, np.zeros(hi - lo), 1.5, 0.75, 3.0)
    w = o.spmv(p_full)
    assert m.alpha == 2.0 and m.beta == 2.0
    assert np.array_equal(bits(m.pw_terms), bits(p_full[off:off + hi - lo] * w))
    xo, ro, po = x.copy(), r.copy(), p_full[off:off + hi - lo].copy()
    ora_calc_xr(xo, ro, po, w, 2.0)
    ora_calc_p(po, ro, 2.0)
    for got, want in ((m.x, xo), (m.r, ro), (m.p, po)):
        assert np.array_equal(bits(got), bits(want))
