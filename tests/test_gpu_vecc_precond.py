"""The three host-scalar entries of Jacobi-preconditioned CG on protected vectors:
abft_hip_precond_start_vecc, abft_hip_calc_r_precond_vecc, abft_hip_calc_px_precond_vecc.

Yardsticks: the numpy model of tests/_vecc_precond.py (every stored word bit for bit, sums within the bar of
test_gpu_vector_ecc.py), and -- with dinv == enc(1.0) -- the plain protected calls this feature does not touch.
Events are (kind, index, bit | operand << 8), the operand counted among the entry's own vector arguments:
precond_start_vecc(r 0, dinv 1, p 2), calc_r_precond_vecc(r 0, w 1, dinv 2), calc_px_precond_vecc(x 0, p 1, r 2, dinv 3)."""
import math

import numpy as np
import pytest

import _ieee as I
import _vecc
import _vecc_precond as P
from test_gpu_vector_ecc import CORRECTED, DOUBLE, Box, bits_of
from test_gpu_vector_ecc_edges import check_sum

pytestmark = pytest.mark.gpu

U = np.uint64
ALPHA, BETA = 0.71, 0.125


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def operands(n, family=None):
    """stored words of x, r, p, w, dinv"""
    if family:
        return [_vecc.family(family, n, _vecc.operand_seed(n, k)) for k in range(5)]
    rng = np.random.default_rng(n)
    v = [_vecc.encode(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)) for _ in range(4)]
    return v + [_vecc.encode(10.0 ** rng.uniform(-3, 3, n))]  # a positive diagonal over six decades


def put(box, v, words):
    box.ctx.upload(v, np.asarray(words, dtype=U).view(np.float64))


def sum_ok(got, aw, bw_values, n, what):
    """got against sum strip(aw) * bw_values: the bar of test_gpu_vector_ecc.py, 1e-13 of the sum of the terms'
    magnitudes; where a term is no finite number or a partial sum can overflow that bar says nothing, and the rule of
    test_gpu_vector_ecc_edges.py holds instead (the class of the result, or its error bound)"""
    with np.errstate(all="ignore"):
        terms = _vecc.strip(aw) * bw_values
    if np.isfinite(terms).all() and float(np.abs(terms).sum()) < I.DBL_MAX / 2:
        want = _vecc.serial_sum(terms)
        assert abs(got - want) <= 1e-13 * float(np.abs(terms).sum()), (what, got, want)
    else:
        check_sum(got, terms, I.dot_depth(n), what)


def z_of(dw, rw):
    with np.errstate(all="ignore"):
        return _vecc.value(dw) * _vecc.strip(rw)


# --------------------------------------------------------------- 1. each entry against the model --

@pytest.mark.parametrize("family", [None, "nan"], ids=["ordinary", "nan"])
@pytest.mark.parametrize("offset", [0, 1])  # whole vectors (the walk by pairs) and views at offset 1 (entry by entry)
def test_entries_against_the_model(amd, offset, family):
    box = Box(amd)
    for n in _vecc.EDGE_LENGTHS:
        xw, rw, pw, ww, dw = operands(n, family)
        x, r, p, w, d = (box.vec(a, offset) for a in (xw, rw, pw, ww, dw))
        what = (n, offset, family)
        # the start: p is only written, r and dinv only read
        rz, rr = box.ctx.precond_start_vecc(r, d, p)
        ps, _, _ = P.precond_start(rw, dw)
        _vecc.assert_words(box.words(p), ps, (what, "start p"))
        assert np.array_equal(box.words(r), rw) and np.array_equal(box.words(d), dw)
        sum_ok(rz, rw, z_of(dw, rw), n, (what, "start r.z"))
        sum_ok(rr, rw, _vecc.strip(rw), n, (what, "start r.r"))
        alone = box.ctx.dot_vecc(r, r)
        assert bits_of(rr) == bits_of(alone) or (math.isnan(rr) and math.isnan(alone)), (what, rr, alone)
        for s in _vecc.SCALARS:
            put(box, r, rw), put(box, p, pw)
            rz, rr = box.ctx.calc_r_precond_vecc(r, w, d, s)
            rs, _, _ = P.calc_r_precond(rw, ww, dw, s)
            got_r = box.words(r)
            _vecc.assert_words(got_r, rs, (what, s, "r"))
            assert np.array_equal(box.words(w), ww) and np.array_equal(box.words(d), dw)
            # the sums are over what the DEVICE stored (a NaN's payload is the device's own)
            sum_ok(rz, got_r, z_of(dw, got_r), n, (what, s, "r.z"))
            sum_ok(rr, got_r, _vecc.strip(got_r), n, (what, s, "r.r"))
            # x and p from the old p, with the r just stored; alpha and beta both walk the scalars
            beta = _vecc.SCALARS[(_vecc.SCALARS.index(s) + 1) % len(_vecc.SCALARS)] if s == s else s
            put(box, r, rs)
            box.ctx.calc_px_precond_vecc(x, p, r, d, s, beta)
            xs, qs = P.calc_px_precond(xw, pw, rs, dw, s, beta)
            _vecc.assert_words(box.words(x), xs, (what, s, "x"))
            _vecc.assert_words(box.words(p), qs, (what, s, beta, "p"))
            assert np.array_equal(box.words(r), rs) and np.array_equal(box.words(d), dw)
            put(box, x, xw)
    assert box.take() == []
    box.ctx.close()


# ------------------------------------------- 2. dinv == enc(1.0): the plain protected calls' bits --

@pytest.mark.parametrize("n", _vecc.EDGE_LENGTHS)
def test_unit_dinv_leaves_the_plain_protected_calls_bits(amd, n):
    box = Box(amd)
    xw, rw, pw, ww, _ = operands(n)
    one = _vecc.encode(np.ones(n))
    d = box.vec(one)
    for alpha, beta in ((0.37251, -1.3125e-3), (-1.0, 0.0)):
        x0, r0, p0, w0 = (box.vec(a) for a in (xw, rw, pw, ww))
        rr0 = box.ctx.calc_r_vecc(r0, w0, alpha)
        box.ctx.calc_px_vecc(x0, p0, r0, alpha, beta)
        x, r, p, w = (box.vec(a) for a in (xw, rw, pw, ww))
        rz, rr = box.ctx.calc_r_precond_vecc(r, w, d, alpha)
        assert np.array_equal(box.words(r), box.words(r0)), (n, alpha)
        assert bits_of(rr) == bits_of(rr0) and bits_of(rz) == bits_of(rr), (n, alpha, rz, rr, rr0)
        box.ctx.calc_px_precond_vecc(x, p, r, d, alpha, beta)
        for name, got, want in (("x", x, x0), ("p", p, p0), ("r", r, r0)):
            assert np.array_equal(box.words(got), box.words(want)), (n, alpha, name)
    r, p = box.vec(rw), box.vec(np.zeros(n, U))
    rz, rr = box.ctx.precond_start_vecc(r, d, p)
    assert np.array_equal(box.words(p), rw), n  # a copy of r
    assert bits_of(rr) == bits_of(box.ctx.dot_vecc(r, r)) and bits_of(rz) == bits_of(rr)
    assert np.array_equal(box.words(d), one) and box.take() == []
    box.ctx.close()


# ----------------------------------------------------------------------------------- 3. flips --

def flip_sites(n):
    return [0, n // 2, n - 1]


FLIP_BITS = [0, 3, 55]  # the overall parity, a check bit, a data bit


@pytest.mark.parametrize("n", [1025, 4099])
def test_a_flip_in_any_operand_is_repaired_and_reported_once(amd, n):
    box = Box(amd)
    xw, rw, pw, ww, dw = operands(n)
    x, r, p, w, d = (box.vec(a) for a in (xw, rw, pw, ww, dw))
    start0 = box.ctx.precond_start_vecc(r, d, p)
    ps0 = box.words(p)
    sums0 = box.ctx.calc_r_precond_vecc(r, w, d, ALPHA)
    r0 = box.words(r)
    put(box, p, pw)
    box.ctx.calc_px_precond_vecc(x, p, r, d, ALPHA, BETA)
    x0, p0 = box.words(x), box.words(p)
    assert box.take() == []

    def same(a, b):
        return [bits_of(v) for v in a] == [bits_of(v) for v in b]

    def kept(v, clean, flipped_here, at, bit):
        """a vector the call only reads keeps its flip -- dinv excepted: its repaired word is stored back"""
        return np.array_equal(box.words(v), P.flipped(clean, at, [bit]) if flipped_here else clean)

    for at in flip_sites(n):
        for bit in FLIP_BITS:
            for op, name in enumerate(("r", "dinv")):  # precond_start_vecc(r, dinv, p)
                put(box, r, rw), put(box, d, dw), put(box, p, np.zeros(n, U))
                box.ctx.flip_vector((r, d)[op], at, [bit])
                assert same(box.ctx.precond_start_vecc(r, d, p), start0), (at, bit, name)
                assert box.take() == [(CORRECTED, at, bit | op << 8)], (at, bit, name)
                assert np.array_equal(box.words(p), ps0)
                assert kept(r, rw, op == 0, at, bit) and np.array_equal(box.words(d), dw), (at, bit, name)
            for op, name in enumerate(("r", "w", "dinv")):  # calc_r_precond_vecc(r, w, dinv)
                put(box, r, rw), put(box, w, ww), put(box, d, dw)
                box.ctx.flip_vector((r, w, d)[op], at, [bit])
                assert same(box.ctx.calc_r_precond_vecc(r, w, d, ALPHA), sums0), (at, bit, name)
                assert box.take() == [(CORRECTED, at, bit | op << 8)], (at, bit, name)
                assert np.array_equal(box.words(r), r0)
                assert kept(w, ww, op == 1, at, bit) and np.array_equal(box.words(d), dw), (at, bit, name)
            for op, name in enumerate(("x", "p", "r", "dinv")):  # calc_px_precond_vecc(x, p, r, dinv)
                put(box, x, xw), put(box, p, pw), put(box, r, r0), put(box, d, dw)
                box.ctx.flip_vector((x, p, r, d)[op], at, [bit])
                box.ctx.calc_px_precond_vecc(x, p, r, d, ALPHA, BETA)
                assert box.take() == [(CORRECTED, at, bit | op << 8)], (at, bit, name)
                assert np.array_equal(box.words(x), x0) and np.array_equal(box.words(p), p0), (at, bit, name)
                assert kept(r, r0, op == 2, at, bit) and np.array_equal(box.words(d), dw), (at, bit, name)
    box.ctx.close()


@pytest.mark.parametrize("entry", ["start", "calc_r", "calc_px"])
def test_a_flip_in_dinv_is_gone_after_the_call_that_met_it(amd, entry):
    n, at, bit = 4099, 2050, 41
    box = Box(amd)
    xw, rw, pw, ww, dw = operands(n)
    x, r, p, w, d = (box.vec(a) for a in (xw, rw, pw, ww, dw))
    call = {"start": lambda: box.ctx.precond_start_vecc(r, d, p),
            "calc_r": lambda: box.ctx.calc_r_precond_vecc(r, w, d, 0.0),  # alpha 0: r keeps its words
            "calc_px": lambda: box.ctx.calc_px_precond_vecc(x, p, r, d, ALPHA, BETA)}[entry]
    op = {"start": 1, "calc_r": 2, "calc_px": 3}[entry]
    box.ctx.flip_vector(d, at, [bit])
    assert np.array_equal(box.words(d), P.flipped(dw, at, [bit]))
    call()
    assert box.take() == [(CORRECTED, at, bit | op << 8)]
    assert np.array_equal(box.words(d), dw)  # gone from memory ...
    call()
    assert box.take() == []  # ... and a second call reports nothing
    assert np.array_equal(box.words(d), dw)
    box.ctx.close()


@pytest.mark.parametrize("entry", ["start", "calc_r", "calc_px"])
def test_two_flips_in_one_dinv_word_are_fatal_and_dinv_is_left_as_it_is(amd, entry):
    n, at, two = 1025, 600, [52, 17]
    box = Box(amd)
    xw, rw, pw, ww, dw = operands(n)
    x, r, p, w, d = (box.vec(a) for a in (xw, rw, pw, ww, dw))
    box.ctx.flip_vector(d, at, two)
    bad = P.flipped(dw, at, two)
    if entry == "start":
        box.ctx.precond_start_vecc(r, d, p)
    elif entry == "calc_r":
        box.ctx.calc_r_precond_vecc(r, w, d, ALPHA)
    else:
        box.ctx.calc_px_precond_vecc(x, p, r, d, ALPHA, BETA)
        box.ctx.synchronize()
    op = {"start": 1, "calc_r": 2, "calc_px": 3}[entry]
    box.ctx._drain()
    assert box.fatal
    assert box.take() == [(DOUBLE, at, op << 8)]
    assert np.array_equal(box.words(d), bad)
    box.ctx.close()


# -------------------------------------------------------------------------------- 4. refusals --

def test_refusals_leave_every_operand_untouched(amd):
    n = 1025
    box = Box(amd)
    ctx = box.ctx
    xw, rw, pw, ww, dw = operands(n)
    x, r, p, w, d = (box.vec(a) for a in (xw, rw, pw, ww, dw))
    marks = _vecc.encode(np.arange(1.0, n + 1.0))
    short = box.vec(marks[:-1])
    both = box.vec(np.concatenate([marks, marks]))
    lo, hi = ctx.view_vector(both, 0, n), ctx.view_vector(both, n - 1, n)  # one entry shared
    everything = [x, r, p, w, d, short, both]

    def refused(call, text):
        pre = [box.words(v) for v in everything]
        with pytest.raises(amd.AbftError, match=text):
            call()
        assert all(np.array_equal(box.words(v), a) for v, a in zip(everything, pre)), text
        assert box.take() == []

    entries = {
        "precond_start_vecc": (lambda v: ctx.precond_start_vecc(*v), [r, d, p]),
        "calc_r_precond_vecc": (lambda v: ctx.calc_r_precond_vecc(*v, ALPHA), [r, w, d]),
        "calc_px_precond_vecc": (lambda v: ctx.calc_px_precond_vecc(*v, ALPHA, BETA), [x, p, r, d]),
    }
    for name, (call, args) in entries.items():
        for k in range(len(args)):  # every length
            v = list(args)
            v[k] = short
            refused(lambda: call(v), name + ": lengths differ")
        for i in range(len(args)):  # every overlap, dinv's included: a shared entry, and the same vector twice
            for j in range(i + 1, len(args)):
                v = list(args)
                v[i], v[j] = lo, hi
                refused(lambda: call(v), name + ": .*overlap")
                v = list(args)
                v[j] = v[i]
                refused(lambda: call(v), name + ": .*overlap")

    # a null dinv (and a null result), at the C boundary
    out = np.zeros(2)
    outp = out.ctypes.data_as(amd.capi.f64p)
    L, chk = ctx.L, amd.capi.check
    h = ctx.h
    refused(lambda: chk(L.abft_hip_precond_start_vecc(h, r.h, None, p.h, outp)), "precond_start_vecc: null vector")
    refused(lambda: chk(L.abft_hip_calc_r_precond_vecc(h, r.h, w.h, None, ALPHA, outp)),
            "calc_r_precond_vecc: null vector")
    refused(lambda: chk(L.abft_hip_calc_px_precond_vecc(h, x.h, p.h, r.h, None, ALPHA, BETA)),
            "calc_px_precond_vecc: null vector")
    refused(lambda: chk(L.abft_hip_precond_start_vecc(h, r.h, d.h, p.h, None)), "precond_start_vecc: null result")
    refused(lambda: chk(L.abft_hip_calc_r_precond_vecc(h, r.h, w.h, d.h, ALPHA, None)),
            "calc_r_precond_vecc: null result")
    # and the calls themselves are fine
    ctx.precond_start_vecc(r, d, p)
    ctx.calc_r_precond_vecc(r, w, d, ALPHA)
    ctx.calc_px_precond_vecc(x, p, r, d, ALPHA, BETA)
    assert not np.array_equal(box.words(x), xw) and box.take() == []
    box.ctx.close()
