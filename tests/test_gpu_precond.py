"""Jacobi-preconditioned CG on the GPU (abft_hip_matrix_diag_inverse, abft_hip_precond_start,
abft_hip_calc_xr_precond, abft_hip_calc_p_precond, their block forms, cg_solve / cg_solve_block with precond=,
the CLI's --precond):

    diagonal     jacobi(A) is numpy's 1 / diag bit for bit in every format, mode and layout; rows without a usable
                 diagonal get 1.0 and are counted
    one call     x, r, p after every entry are numpy's bits (z = dinv * r, r - alpha w, z + beta p, x + alpha p,
                 each a separate rounded operation); the two sums within 1e-12 of math.fsum
    deferral     the x half carried out by calc_p_precond or flushed by anything else: the same bits
    identity     dinv == 1.0: plain CG bit for bit;  dinv == 0.25: x, r, rr identical, p scaled exactly
    it helps     badly scaled systems converge that plain CG does not solve; fewer iterations on power-law rows
    faults       a damaged dinv changes the rate only; a flip in x is rolled back under PCG as under CG
"""
import hashlib
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _ieee import ieee_diff, ieee_equal, special_vector
from _oracle import laplace5, random_spd
from _precond import diagonal, matvec, model_cg, scaled

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("none", "constraints", "sed", "sec7", "sec8", "secded")
SOLVE_MODES = ("none", "sed", "secded")


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64),
                          np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def close(got, terms):
    """a tree sum of non-negative terms against math.fsum of the same rounded terms: 1e-12 relative"""
    want = math.fsum(float(t) for t in terms)
    return abs(got - want) <= 1e-12 * abs(want)


def flipped(v, bit):
    u = np.array([v], dtype=np.float64).view(np.uint64)
    u ^= np.uint64(1) << np.uint64(bit)
    return u.view(np.float64)[0]


# ------------------------------------------------------------------ 1. the diagonal --

# run in a child so that the layout can be forced
DIAG_PROBE = r'''
import ctypes
import sys
sys.path.insert(0, "tests")
import numpy as np
import abft_sparse_cg_amd as amd
from abft_sparse_cg_amd import generators
from _oracle import laplace5, random_spd
from _precond import diagonal

def bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))

FMT, LAYOUT = sys.argv[1], sys.argv[2]
mats = {"laplace5": laplace5(40, 33), "random": random_spd(3000, 12, 5), "powerlaw": generators.generate("powerlaw:4096,1")}

# a matrix with every kind of unusable diagonal: laplace5(12, 12) with
#   row 5 emptied, the diagonal of row 7 removed, those of rows 9, 11, 13, 15 set to 0, -4, inf, NaN,
#   and three elements on the diagonal of row 20: 0.1 in its place, 0.2 and 0.3 behind the row's last element;
#   in the caller's order (0.1 + 0.2) + 0.3 = 0.6000000000000001, in the reverse order 0.6
c, r, v, n = laplace5(12, 12)
keep = ~((r == 5) | ((r == 7) & (c == 7)))
c, r, v = c[keep], r[keep], v[keep].copy()
for row, val in ((9, 0.0), (11, -4.0), (13, np.inf), (15, np.nan), (20, 0.1)):
    v[(r == row) & (c == row)] = val
at = int(np.flatnonzero(r == 20)[-1]) + 1
c, r, v = np.insert(c, at, [20, 20]), np.insert(r, at, [20, 20]), np.insert(v, at, [0.2, 0.3])
want_bad = np.ones(n)
ok = np.ones(n, dtype=bool)
ok[[5, 7, 9, 11, 13, 15]] = False
d = diagonal(c, r, v, n)
assert d[20] == (0.1 + 0.2) + 0.3 and d[20] != (0.3 + 0.2) + 0.1
want_bad[ok] = 1.0 / d[ok]

seen = set()
for mode in ("none", "constraints", "sed", "sec7", "sec8", "secded"):
    ctx = amd.HIPContext(mode, FMT, on_event=lambda ev, fatal: None)
    for name, (cols, rows, vals, nn) in mats.items():
        A = ctx.create_matrix(cols, rows, vals, nn, len(vals))
        if LAYOUT == "sweep" and mode != "constraints" and name == "laplace5":
            assert ctx.matrix_info(A)[0] == "sweep", (mode, name, ctx.matrix_info(A))
        seen.add(ctx.matrix_info(A)[0])
        if LAYOUT == "stream":
            assert ctx.matrix_info(A)[0] == "stream", (mode, name, ctx.matrix_info(A))
        dinv = ctx.jacobi(A)
        assert dinv.bad == 0 and dinv.N == nn
        got = ctx.download(dinv)
        assert bits_equal(got, 1.0 / diagonal(cols, rows, vals, nn)), (mode, name)
        ctx.destroy_vector(dinv)
        ctx.destroy_matrix(A)
    A = ctx.create_matrix(c, r, v, n, len(v))
    try:
        ctx.jacobi(A)
    except ValueError as e:
        assert "6 of 144 rows" in str(e), e
    else:
        raise AssertionError("strict jacobi accepted a bad diagonal")
    dinv = ctx.jacobi(A, strict=False)
    assert dinv.bad == 6, dinv.bad
    assert bits_equal(ctx.download(dinv), want_bad), (mode, ctx.download(dinv)[[5, 7, 9, 11, 13, 15, 20]])
    # wrong length, and (mode none) a flipped value bit of a diagonal element is seen by the next call
    short = ctx.create_vector(n - 1)
    bad = ctypes.c_uint32(0)
    rc = ctx.L.abft_hip_matrix_diag_inverse(ctx.h, A.h, short.h, ctypes.byref(bad))
    assert rc == -1, rc
    if mode == "none":
        idx = int(np.flatnonzero((r == 3) & (c == 3))[0])
        ctx.inject_at(A, idx, [52 if FMT == "csr" else 64 + 52])
        again = ctx.download(ctx.jacobi(A, strict=False))
        want = want_bad.copy()
        u = np.array([4.0]).view(np.uint64)
        u ^= np.uint64(1) << np.uint64(52)
        want[3] = 1.0 / u.view(np.float64)[0]
        assert want[3] != want_bad[3] and bits_equal(again, want), (again[3], want[3])
    assert ctx.event_log == [], (mode, ctx.event_log[:4])
    ctx.close()
assert LAYOUT in ("auto", "stream") or LAYOUT in seen, seen   # the forced layout's cold path did run
print("ok")
'''


@pytest.mark.parametrize("fmt,layout", [("csr", "auto"), ("coo", "auto"), ("csr", "stream"), ("coo", "stream"),
                                        ("coo", "panels"), ("csr", "sweep")])
def test_diagonal_in_every_format_mode_and_layout(fmt, layout):
    env = dict(os.environ)
    if layout != "auto":
        env.update(ABFT_HIP_LAYOUT=layout)
    if layout in ("panels", "sweep"):
        env.update(ABFT_HIP_PANEL_WIDTH="16")
    p = subprocess.run([sys.executable, "-c", DIAG_PROBE, fmt, layout], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_diagonal_refuses_shards(amd):
    cols, rows, vals, n = laplace5(12, 12)
    for fmt in ("csr", "coo"):
        ctx = amd.HIPContext("none", fmt)
        try:
            m = (rows if fmt == "csr" else cols) < 72  # CSR shards own rows, COO shards columns
            A = ctx.create_matrix(cols[m], rows[m], vals[m], 72, int(m.sum()), n_in=n)
            with pytest.raises(amd.AbftError) as e:
                ctx.jacobi(A)
            assert e.value.code == -1 and "shard" in str(e.value)
        finally:
            ctx.close()


# ------------------------------------------------------------------ 2. one call, bit for bit --

def placed(ctx, arrays, offsets):
    """upload each array into a view at the given offset of a fresh parent: offset 1 is 8 bytes off a 16-byte
    boundary (the one-entry kernels), 0 and 2 are aligned (the paired ones)"""
    out = []
    for a, off in zip(arrays, offsets):
        parent = ctx.create_vector(len(a) + 3)
        v = ctx.view_vector(parent, off, len(a)) if off else ctx.view_vector(parent, 0, len(a))
        ctx.upload(v, a)
        out.append(v)
    return out


SINGLE_CASES = [(1, "aligned"), (2, "aligned"), (2, "odd"), (7, "aligned"), (7, "odd"), (1001, "aligned"),
                (1001, "odd"), (1001, "dinv_odd"), (1001, "mixed"), (2 ** 20 + 3, "aligned"), (2 ** 20 + 3, "odd"),
                (2 ** 20 + 3, "dinv_odd")]


@pytest.mark.parametrize("n,place", SINGLE_CASES)
@pytest.mark.parametrize("data", ["finite", "special"])
def test_single_entries_bit_for_bit(amd, n, place, data):
    rng = np.random.default_rng(n + len(place))
    if data == "finite":
        x0, r0, p0, w0 = (rng.standard_normal(n) for _ in range(4))
    else:
        x0, r0, p0, w0 = (special_vector(n, 10 + i) for i in range(4))
    d0 = np.exp(rng.standard_normal(n) * 3.0)  # positive, five decades
    if data == "special":
        d0[::7] = 1.0
        d0[3::11] = 2.0 ** -1000
    alpha, beta = 0.37, -1.25
    # offsets of (x, r, p, w, dinv)
    offs = {"aligned": (0, 0, 0, 0, 0), "odd": (1, 1, 1, 1, 1), "dinv_odd": (2, 0, 2, 0, 1), "mixed": (1, 0, 1, 0, 0)}[place]
    ctx = amd.HIPContext("none", "csr")
    try:
        def fresh():
            return placed(ctx, (x0, r0, p0, w0, d0), offs)

        with np.errstate(all="ignore"):
            # precond_start
            x, r, p, w, d = fresh()
            rz, rr = ctx.precond_start(r, d, p)
            z = d0 * r0
            assert ieee_equal(ctx.download(p), z), ieee_diff(ctx.download(p), z)
            assert bits_equal(ctx.download(r), r0) and bits_equal(ctx.download(d), d0)
            if data == "finite":
                assert close(rz, r0 * z) and close(rr, r0 * r0), (rz, rr)
                assert rr == ctx.dot(r, r)
            # calc_xr_precond then calc_p_precond (the x half deferred where the rules allow it)
            x, r, p, w, d = fresh()
            rz, rr = ctx.calc_xr_precond(x, r, p, w, d, alpha)
            r1 = r0 - alpha * w0
            z1 = d0 * r1
            if data == "finite":
                assert close(rz, r1 * z1) and close(rr, r1 * r1), (rz, rr)
            ctx.calc_p_precond(p, r, d, beta)
            x1 = x0 + alpha * p0
            p1 = z1 + beta * p0
            for name, v, want in (("x", x, x1), ("r", r, r1), ("p", p, p1), ("w", w, w0), ("dinv", d, d0)):
                assert ieee_equal(ctx.download(v), want), (name, ieee_diff(ctx.download(v), want))
            # calc_p_precond on its own
            x, r, p, w, d = fresh()
            ctx.calc_p_precond(p, r, d, beta)
            want = d0 * r0 + beta * p0
            assert ieee_equal(ctx.download(p), want), ieee_diff(ctx.download(p), want)
            assert bits_equal(ctx.download(x), x0)
            # dinv == 1.0: the sums are the plain calls' bits
            if data == "finite":
                ones = placed(ctx, (np.ones(n),), (offs[4],))[0]
                x, r, p, w, d = fresh()
                want_rr = ctx.calc_xr(x, r, p, w, alpha)
                ctx.calc_p(p, r, beta)
                xa, ra, pa = ctx.download(x), ctx.download(r), ctx.download(p)
                x, r, p, w, d = fresh()
                rz, rr = ctx.calc_xr_precond(x, r, p, w, ones, alpha)
                ctx.calc_p_precond(p, r, ones, beta)
                assert rz == want_rr and rr == want_rr, (rz, rr, want_rr)  # whatever dinv's own alignment
                assert close(rr, ra * ra)
                assert bits_equal(ctx.download(x), xa) and bits_equal(ctx.download(r), ra) and bits_equal(ctx.download(p), pa)
                rz, rr = ctx.precond_start(r, ones, p)
                assert rz == rr == ctx.dot(r, r) and bits_equal(ctx.download(p), ra)
    finally:
        ctx.close()


def test_single_entries_check_their_arguments(amd):
    n = 100
    ctx = amd.HIPContext("none", "csr")
    try:
        x, r, p, w, d = (ctx.create_vector(n) for _ in range(5))
        for v in (x, r, p, w, d):
            ctx.upload(v, np.ones(n))
        short = ctx.create_vector(n - 1)
        overlap = ctx.view_vector(r, 10, n - 10)
        bad = [lambda: ctx.precond_start(r, short, p), lambda: ctx.precond_start(short, d, p),
               lambda: ctx.precond_start(r, p, p), lambda: ctx.precond_start(r, d, r),
               lambda: ctx.calc_xr_precond(x, r, p, short, d, 0.5), lambda: ctx.calc_xr_precond(x, r, p, w, short, 0.5),
               lambda: ctx.calc_xr_precond(x, r, p, w, x, 0.5), lambda: ctx.calc_xr_precond(x, r, p, w, r, 0.5),
               lambda: ctx.calc_p_precond(p, r, p, 0.5), lambda: ctx.calc_p_precond(p, short, d, 0.5),
               lambda: ctx.calc_p_precond(ctx.view_vector(p, 0, n - 10), overlap, ctx.view_vector(p, 10, n - 10), 0.5)]
        for i, f in enumerate(bad):
            with pytest.raises(amd.AbftError) as e:
                f()
            assert e.value.code == -1, i
        # nothing was enqueued: every vector still holds its ones
        for v in (x, r, p, w, d):
            assert bits_equal(ctx.download(v), np.ones(n))
        # dinv may alias a vector the call only reads
        ctx.calc_xr_precond(x, r, p, w, w, 0.5)
        ctx.calc_p_precond(p, r, r, 0.5)
        # length 0
        e0 = [ctx.create_vector(0) for _ in range(5)]
        assert ctx.precond_start(e0[1], e0[4], e0[2]) == (0.0, 0.0)
        assert ctx.calc_xr_precond(*e0[:4], e0[4], 0.5) == (0.0, 0.0)
        ctx.calc_p_precond(e0[2], e0[1], e0[4], 0.5)
    finally:
        ctx.close()


@pytest.mark.parametrize("k", range(1, 9))
@pytest.mark.parametrize("data", ["finite", "special"])
def test_block_entries_bit_for_bit(amd, k, data):
    n = 1003 if k != 3 else 2 ** 16 + 5
    rng = np.random.default_rng(40 + k)
    if data == "finite":
        X0, R0, P0, W0 = (rng.standard_normal((n, k)) for _ in range(4))
    else:
        X0, R0, P0, W0 = (special_vector(n * k, 20 + i).reshape(n, k) for i in range(4))
    d0 = np.exp(rng.standard_normal(n) * 3.0)
    alpha = rng.standard_normal(8)[:k]
    beta = rng.standard_normal(8)[:k]
    full = (1 << k) - 1
    ctx = amd.HIPContext("none", "csr")
    try:
        X, R, P, W = (ctx.create_block(n, k) for _ in range(4))
        d = ctx.create_vector(n)
        ctx.upload(d, d0)
        for mask in sorted({full, 0b10110101 & full, 0b01001010 & full, 0}):
            on = np.array([(mask >> j) & 1 for j in range(k)], dtype=bool)
            for v, a in ((X, X0), (R, R0), (P, P0), (W, W0)):
                ctx.upload(v, a)
            with np.errstate(all="ignore"):
                # precond_start_block: P rewritten in the masked columns only, sums of every column
                rz, rr = ctx.precond_start_block(R, d, P, k, mask)
                Z = d0[:, None] * R0
                want = np.where(on[None, :], Z, P0)
                assert ieee_equal(ctx.download(P), want), (mask, ieee_diff(ctx.download(P), want))
                assert bits_equal(ctx.download(P)[:, ~on], P0[:, ~on]) and bits_equal(ctx.download(R), R0)
                if data == "finite":
                    for j in range(k):
                        assert close(rz[j], R0[:, j] * Z[:, j]) and close(rr[j], R0[:, j] * R0[:, j]), (mask, j)
                    assert bits_equal(rr, ctx.dot_block(R, R, k))
                # calc_xr_precond_block, calc_p_precond_block
                ctx.upload(P, P0)
                rz, rr = ctx.calc_xr_precond_block(X, R, P, W, d, k, alpha, mask)
                X1 = np.where(on[None, :], X0 + alpha[None, :] * P0, X0)
                R1 = np.where(on[None, :], R0 - alpha[None, :] * W0, R0)
                Z1 = d0[:, None] * R1
                ctx.calc_p_precond_block(P, R, d, k, beta, mask)
                P1 = np.where(on[None, :], Z1 + beta[None, :] * P0, P0)
                for name, v, want, orig in (("x", X, X1, X0), ("r", R, R1, R0), ("p", P, P1, P0)):
                    got = ctx.download(v)
                    assert ieee_equal(got, want), (mask, name, ieee_diff(got, want))
                    assert bits_equal(got[:, ~on], orig[:, ~on]), (mask, name)  # NaN payloads and all
                assert bits_equal(ctx.download(W), W0) and bits_equal(ctx.download(d), d0)
                if data == "finite":
                    for j in range(k):
                        assert close(rz[j], R1[:, j] * Z1[:, j]) and close(rr[j], R1[:, j] * R1[:, j]), (mask, j)
        if data == "finite":
            # dinv == 1.0: the bits calc_xr_block / calc_p_block leave and return
            ones = ctx.create_vector(n)
            ctx.upload(ones, np.ones(n))
            mask = 0b10110101 & full
            for v, a in ((X, X0), (R, R0), (P, P0), (W, W0)):
                ctx.upload(v, a)
            want_rr = ctx.calc_xr_block(X, R, P, W, k, alpha, mask)
            ctx.calc_p_block(P, R, k, beta, mask)
            Xa, Ra, Pa = ctx.download(X), ctx.download(R), ctx.download(P)
            for v, a in ((X, X0), (R, R0), (P, P0), (W, W0)):
                ctx.upload(v, a)
            rz, rr = ctx.calc_xr_precond_block(X, R, P, W, ones, k, alpha, mask)
            ctx.calc_p_precond_block(P, R, ones, k, beta, mask)
            assert bits_equal(rz, want_rr) and bits_equal(rr, want_rr)
            assert bits_equal(ctx.download(X), Xa) and bits_equal(ctx.download(R), Ra) and bits_equal(ctx.download(P), Pa)
        # arguments: dinv of the wrong length, dinv inside a written block, k out of range
        with pytest.raises(amd.AbftError):
            ctx.precond_start_block(R, ctx.create_vector(n + 1), P, k, full)
        with pytest.raises(amd.AbftError):
            ctx.calc_p_precond_block(P, R, ctx.view_vector(P, 0, n), k, beta, full)
        with pytest.raises(amd.AbftError):
            ctx.calc_xr_precond_block(X, R, P, W, ctx.view_vector(R, 0, n), k, alpha, full)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3. the deferral is transparent --

DEFER_PROBE = r'''
import hashlib, sys
sys.path.insert(0, "tests")
import numpy as np
import abft_sparse_cg_amd as amd

def bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))

n = 5003
rng = np.random.default_rng(9)
x0, r0, p0, w0, q0 = (rng.standard_normal(n) for _ in range(5))
d0 = np.exp(rng.standard_normal(n))
alpha, beta = 0.37, -1.25
ctx = amd.HIPContext("none", "csr")
def fresh():
    vs = [ctx.create_vector(n) for _ in range(6)]
    for v, a in zip(vs, (x0, r0, p0, w0, q0, d0)):
        ctx.upload(v, a)
    return vs
xr, rn = x0 + alpha * p0, r0 - alpha * w0
zn = d0 * rn
pn = zn + beta * p0

# (1) the loop's order: one kernel does both halves
x, r, p, w, q, d = fresh()
ctx.calc_xr_precond(x, r, p, w, d, alpha)
ctx.calc_p_precond(p, r, d, beta)
assert bits_equal(ctx.download(x), xr) and bits_equal(ctx.download(r), rn) and bits_equal(ctx.download(p), pn)
# (2) x downloaded between the two calls
x, r, p, w, q, d = fresh()
ctx.calc_xr_precond(x, r, p, w, d, alpha)
assert bits_equal(ctx.download(x), xr)
ctx.calc_p_precond(p, r, d, beta)
assert bits_equal(ctx.download(p), pn) and bits_equal(ctx.download(x), xr)
# (3) other entries in between: p overwritten, a dot, a plain calc_p on another vector, a residual-style copy
x, r, p, w, q, d = fresh()
ctx.calc_xr_precond(x, r, p, w, d, alpha)
ctx.copy_vector(p, q)
assert bits_equal(ctx.download(x), xr) and bits_equal(ctx.download(p), q0)
x, r, p, w, q, d = fresh()
ctx.calc_xr_precond(x, r, p, w, d, alpha)
ctx.dot(x, x)
ctx.calc_p_precond(p, r, d, beta)
assert bits_equal(ctx.download(x), xr) and bits_equal(ctx.download(p), pn)
x, r, p, w, q, d = fresh()
ctx.calc_xr_precond(x, r, p, w, d, alpha)
ctx.calc_p_precond(q, r, d, beta)      # not the pair: q, not p
assert bits_equal(ctx.download(q), zn + beta * q0) and bits_equal(ctx.download(x), xr) and bits_equal(ctx.download(p), p0)
# (4) the plain calc_p absorbs a preconditioned calc_xr's x half, and the other way round
x, r, p, w, q, d = fresh()
ctx.calc_xr_precond(x, r, p, w, d, alpha)
ctx.calc_p(p, r, beta)
assert bits_equal(ctx.download(x), xr) and bits_equal(ctx.download(p), rn + beta * p0)
x, r, p, w, q, d = fresh()
ctx.calc_xr(x, r, p, w, alpha)
ctx.calc_p_precond(p, r, d, beta)
assert bits_equal(ctx.download(x), xr) and bits_equal(ctx.download(p), pn)
# (5) two calc_xr_precond in a row
x, r, p, w, q, d = fresh()
ctx.calc_xr_precond(x, r, p, w, d, alpha)
ctx.calc_xr_precond(x, r, p, w, d, alpha)
ctx.calc_p_precond(p, r, d, beta)
r2 = rn - alpha * w0
assert bits_equal(ctx.download(x), xr + alpha * p0) and bits_equal(ctx.download(p), d0 * r2 + beta * p0)
# (6) a vector whose address was handed out, and a view: never deferred, same bits
x, r, p, w, q, d = fresh()
assert x.device_ptr
ctx.calc_xr_precond(x, r, p, w, d, alpha)
ctx.calc_p_precond(p, r, d, beta)
assert bits_equal(ctx.download(x), xr) and bits_equal(ctx.download(p), pn)
# (7) operands that alias each other run undeferred; what they leave is compared between the two settings
h = hashlib.sha256()
for which in ("x=p", "x=w", "r=p", "p=w"):
    x, r, p, w, q, d = fresh()
    if which == "x=p": a = (x, r, x, w)
    if which == "x=w": a = (x, r, p, x)
    if which == "r=p": a = (x, r, r, w)
    if which == "p=w": a = (x, r, p, p)
    rz, rr = ctx.calc_xr_precond(*a, d, alpha)
    ctx.calc_p_precond(a[2], r, d, beta) if a[2] is not r else None
    for v in (x, r, p, w):
        h.update(ctx.download(v).tobytes())
    h.update(np.array([rz, rr]).tobytes())
x, r, p, w, q, d = fresh()
rz, rr = ctx.calc_xr_precond(x, r, r, w, d, alpha)   # p = r: x sees r as it was
assert bits_equal(ctx.download(x), x0 + alpha * r0) and bits_equal(ctx.download(r), rn)
ctx.close()
print("ok", h.hexdigest())
'''


def test_deferred_x_update_is_transparent_under_precond():
    outs = []
    for fuse in (None, "0"):
        env = dict(os.environ)
        env.pop("ABFT_HIP_FUSE_X", None)
        if fuse is not None:
            env["ABFT_HIP_FUSE_X"] = fuse
        p = subprocess.run([sys.executable, "-c", DEFER_PROBE], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout + p.stderr
        outs.append(p.stdout)
    assert outs[0] == outs[1]  # the aliased calls left the same bits with and without the deferral


# ------------------------------------------------------------------ 4-8. solves --

def solve(amd, ctx, A, n, b, conv, itrs, dinv=None, flips=(), keep=False, **kw):
    """-> (itr, history, x, r, p, checks); flips: (iteration, vector name or Vector, index, bits)"""
    vb, x, r, p, w = (ctx.create_vector(n) for _ in range(5))
    vecs = {"x": x, "r": r, "p": p}
    ctx.upload(vb, b)
    ctx.upload(x, np.zeros(n))
    hist, checks = [], []

    def on_it(i, rr):
        hist.append(rr)
        for fi, name, idx, bits in flips:
            if fi == i:
                ctx.flip_vector(vecs.get(name, name) if isinstance(name, str) else name, idx, bits)

    it, _ = amd.cg_solve(ctx, A, vb, x, r, p, w, itrs, conv, on_iteration=on_it,
                         on_check=lambda *c: checks.append(c), precond=dinv, **kw)
    out = it, hist, ctx.download(x), ctx.download(r), ctx.download(p), checks
    for v in (vb, x, r, p, w):
        ctx.destroy_vector(v)
    return out


def solve_block(amd, ctx, A, n, Bs, conv, itrs, dinv=None, flips=(), **kw):
    k = Bs.shape[1]
    B, X, R, P, W = (ctx.create_block(n, k) for _ in range(5))
    ctx.upload(B, Bs)
    ctx.upload(X, np.zeros((n, k)))
    hist, checks = [], []

    def on_it(i, rr, act):
        hist.append((rr, act))
        for fi, idx, bits in flips:
            if fi == i:
                ctx.flip_vector(X, idx, bits)

    itrs_, _ = amd.cg_solve_block(ctx, A, B, X, R, P, W, itrs, conv, on_iteration=on_it,
                                  on_check=lambda *c: checks.append(c), precond=dinv, **kw)
    out = itrs_, hist, ctx.download(X), ctx.download(R), ctx.download(P), checks
    for v in (B, X, R, P, W):
        ctx.destroy_vector(v)
    return out


def reference_rhs(n, seed=1):
    from abft_sparse_cg_amd import generators
    return generators.reference_rhs(n, seed)


@pytest.mark.parametrize("fmt", ["csr", "coo"])
@pytest.mark.parametrize("mode", SOLVE_MODES)
def test_identity_preconditioner_is_plain_cg(amd, fmt, mode):
    cols, rows, vals, n = random_spd(2000, 10, 7)
    b = reference_rhs(n)
    ctx = amd.HIPContext(mode, fmt)
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream" if fmt == "csr" else None)
        ones = ctx.create_vector(n)
        ctx.upload(ones, np.ones(n))
        for kw in ({}, {"check_every": 7}):
            it0, h0, x0, r0, p0, c0 = solve(amd, ctx, A, n, b, 1e-20, 400, **kw)
            it1, h1, x1, r1, p1, c1 = solve(amd, ctx, A, n, b, 1e-20, 400, dinv=ones, **kw)
            assert it1 == it0 and it0 > 5 and h1 == h0
            assert bits_equal(x1, x0) and bits_equal(r1, r0) and bits_equal(p1, p0) and c1 == c0
        if fmt == "csr":
            Bs = np.stack([reference_rhs(n, 1 + j) for j in range(3)], axis=1)
            i0, h0, X0, R0, P0, _ = solve_block(amd, ctx, A, n, Bs, 1e-20, 400)
            i1, h1, X1, R1, P1, _ = solve_block(amd, ctx, A, n, Bs, 1e-20, 400, dinv=ones)
            assert i1 == i0 and len(h1) == len(h0)
            assert all(bits_equal(a[0], c[0]) and a[1] == c[1] for a, c in zip(h0, h1))
            assert bits_equal(X1, X0) and bits_equal(R1, R0) and bits_equal(P1, P0)
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", ["csr", "coo"])
@pytest.mark.parametrize("mode", SOLVE_MODES)
def test_exact_scaling_by_a_power_of_two(amd, fmt, mode):
    """laplace5:40,40 has dinv == 0.25 everywhere: z = r / 4 is exact, so x, r and every rr are plain CG's
    bits and p is exactly a quarter of plain CG's p"""
    cols, rows, vals, n = laplace5(40, 40)
    b = reference_rhs(n)
    ctx = amd.HIPContext(mode, fmt)
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        dinv = ctx.jacobi(A)
        assert bits_equal(ctx.download(dinv), np.full(n, 0.25))
        it0, h0, x0, r0, p0, _ = solve(amd, ctx, A, n, b, 1e-10, 400)
        it1, h1, x1, r1, p1, _ = solve(amd, ctx, A, n, b, 1e-10, 400, dinv=dinv)
        assert it1 == it0 and it0 > 50 and h1 == h0
        assert bits_equal(x1, x0) and bits_equal(r1, r0) and bits_equal(p1, 0.25 * p0)
    finally:
        ctx.close()


def scaled_system():
    cols, rows, vals, n = scaled(*laplace5(40, 40))
    b = reference_rhs(n)
    return cols, rows, vals, n, b


def residual_bound_holds(cols, rows, vals, n, b, x, conv):
    """||b - A x|| <= sqrt(threshold) + 1e-7 ||b||: what a passed final check and the stop test imply together"""
    res = float(np.linalg.norm(b - matvec(cols, rows, vals, n, x)))
    return res <= math.sqrt(conv) + 1e-7 * float(np.linalg.norm(b)), res


@pytest.mark.parametrize("fmt", ["csr", "coo"])
@pytest.mark.parametrize("mode", SOLVE_MODES)
def test_jacobi_solves_the_badly_scaled_system(amd, fmt, mode):
    """The scaled laplace5:40,40 (S A S, s_i = 2^((7919 i mod 13) - 6)), threshold 1e-3, 1000 iterations at most,
    a residual check every 10: plain CG is still far away at max_itrs, PCG converges in at most twice the numpy
    model's count (about 98; the summation order differs on a system this badly scaled, hence the factor)."""
    cols, rows, vals, n, b = scaled_system()
    dref = 1.0 / diagonal(cols, rows, vals, n)
    model, _, _ = model_cg(cols, rows, vals, n, b, 1e-3, 1000, dref)
    assert model < 200  # (98 where this was written; numpy's own summation order may move it by a few)
    ctx = amd.HIPContext(mode, fmt)
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        it0, h0, x0, _, _, c0 = solve(amd, ctx, A, n, b, 1e-3, 1000, check_every=10)
        assert it0 == 1000 and h0[-1] > 1e-3 and all(c[2] for c in c0), (it0, h0[-1])
        dinv = ctx.jacobi(A)
        assert bits_equal(ctx.download(dinv), dref)
        it, h, x, _, _, checks = solve(amd, ctx, A, n, b, 1e-3, 1000, dinv=dinv, check_every=10)
        print("scaled laplace5:40,40 %s %s: PCG %d iterations (model %d), plain CG rr = %.3e at 1000" % (fmt, mode, it, model, h0[-1]))
        assert it < 1000 and h[-1] <= 1e-3 and checks and all(c[2] for c in checks), (it, checks)
        ok, res = residual_bound_holds(cols, rows, vals, n, b, x, 1e-3)
        assert ok, res
        assert it <= 2 * model, (it, model)
    finally:
        ctx.close()


def test_jacobi_needs_fewer_iterations_on_powerlaw_coo_sec7(amd):
    from abft_sparse_cg_amd import generators
    cols, rows, vals, n = generators.generate("powerlaw:65536,1")
    b = reference_rhs(n)
    ctx = amd.HIPContext("sec7", "coo")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        it0, h0, x0, _, _, _ = solve(amd, ctx, A, n, b, 1e-3, 1000)
        dinv = ctx.jacobi(A)
        it, h, x, _, _, checks = solve(amd, ctx, A, n, b, 1e-3, 1000, dinv=dinv, check_every=10)
        print("powerlaw:65536,1 coo sec7: CG %d iterations, PCG %d" % (it0, it))
        assert it < it0 < 1000 and h[-1] <= 1e-3 and all(c[2] for c in checks), (it, it0)
        ok, res = residual_bound_holds(cols, rows, vals, n, b, x, 1e-3)
        assert ok, res
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", ["csr", "coo"])
@pytest.mark.parametrize("mode", SOLVE_MODES)
def test_damaged_dinv_changes_the_rate_not_the_answer(amd, fmt, mode):
    """bit 51 of one dinv entry flipped after iteration 5: M changes, r stays consistent with b - A x"""
    cols, rows, vals, n, b = scaled_system()
    ctx = amd.HIPContext(mode, fmt)
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        dinv = ctx.jacobi(A)
        before = ctx.download(dinv)
        i = n // 2 + 7
        it, h, x, _, _, checks = solve(amd, ctx, A, n, b, 1e-3, 1000, dinv=dinv, check_every=10,
                                       flips=[(5, dinv, i, [51])])
        after = ctx.download(dinv)
        assert after[i] == flipped(before[i], 51) and after[i] != before[i]
        assert it < 1000 and h[-1] <= 1e-3 and checks and all(c[2] for c in checks), (it, checks)
        ok, res = residual_bound_holds(cols, rows, vals, n, b, x, 1e-3)
        assert ok, res
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", ["csr", "coo"])
@pytest.mark.parametrize("mode", SOLVE_MODES)
def test_rollback_under_pcg(amd, fmt, mode):
    """the x flip of test_gpu_residual_check.py (bit 55 after iteration 10, a check every 5) under PCG"""
    cols, rows, vals, n, b = scaled_system()
    ctx = amd.HIPContext(mode, fmt)
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        dinv = ctx.jacobi(A)
        it0, h0, x0, _, _, c0 = solve(amd, ctx, A, n, b, 1e-3, 1000, dinv=dinv, check_every=5)
        it, h, x, _, _, checks = solve(amd, ctx, A, n, b, 1e-3, 1000, dinv=dinv, check_every=5,
                                       flips=[(10, "x", n // 2 + 7, [55])])
        fails = [c for c in checks if not c[2]]
        assert [(c[0], c[3]) for c in fails] == [(14, 9)], checks
        assert h[:11] == h0[:11] and it > it0 and h[-1] <= 1e-3 and checks[-1][2]
        ok, res = residual_bound_holds(cols, rows, vals, n, b, x, 1e-3)
        assert ok, res
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", SOLVE_MODES)
def test_block_rollback_under_pcg_touches_one_column(amd, mode):
    cols, rows, vals, n, _ = scaled_system()
    k = 3
    Bs = np.stack([reference_rhs(n, 1 + j) for j in range(k)], axis=1)
    ctx = amd.HIPContext(mode, "csr")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        dinv = ctx.jacobi(A)
        i0, h0, X0, R0, P0, c0 = solve_block(amd, ctx, A, n, Bs, 1e-3, 1000, dinv=dinv, check_every=5)
        assert all(c[2] for c in c0) and max(i0) < 1000
        # each column is the single preconditioned solve's, but for the tree sums' shape
        i1, h1, X1, R1, P1, c1 = solve_block(amd, ctx, A, n, Bs, 1e-3, 1000, dinv=dinv, check_every=5,
                                             flips=[(10, (n // 2 + 7) * k + 1, [55])])
        fails = [c for c in c1 if not c[2]]
        assert [(c[0], c[3], c[4]) for c in fails] == [(14, 9, 1)], fails
        for j in (0, 2):
            assert i1[j] == i0[j], j
            assert bits_equal(X1[:, j], X0[:, j]) and bits_equal(R1[:, j], R0[:, j]) and bits_equal(P1[:, j], P0[:, j]), j
            assert [h[0][j] for h in h1 if (h[1] >> j) & 1] == [h[0][j] for h in h0 if (h[1] >> j) & 1], j
        assert i1[1] > i0[1]
        for j in range(k):
            ok, res = residual_bound_holds(cols, rows, vals, n, Bs[:, j], np.ascontiguousarray(X1[:, j]), 1e-3)
            assert ok, (j, res)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 9. the CLI --

def cli(args, rc=0):
    p = subprocess.run([sys.executable, "-m", "abft_sparse_cg_amd.cg", "-t", "hip"] + args, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == rc, p.stdout + p.stderr
    return re.sub(r"time taken = .*", "time taken", p.stdout)


def iterations(out):
    return [int(v) for v in re.findall(r"ran for (\d+) iterations", out)]


@pytest.mark.parametrize("fmt,mode", [("csr", "none"), ("coo", "sec7"), ("csr", "secded"), ("coo", "sed")])
def test_cli(fmt, mode):
    base = ["-s", "powerlaw:65536,1", "-m", mode, "--format", fmt]
    plain = cli(base)
    assert cli(base + ["--precond", "none"]) == plain and "preconditioner" not in plain
    out = cli(base + ["--precond", "jacobi"])
    lines = out.splitlines()
    at = lines.index("preconditioner: jacobi")
    assert at < next(i for i, l in enumerate(lines) if l.startswith("iteration "))
    assert lines.count("preconditioner: jacobi") == 1
    assert iterations(out)[0] < iterations(plain)[0], (iterations(out), iterations(plain))
    # without the line, and but for the iterations themselves, the transcript has today's shape
    strip = lambda t: [l for l in t.splitlines() if not l.startswith(("iteration ", "ran for", "total error", "max error"))]
    assert strip(out.replace("preconditioner: jacobi\n", "")) == strip(plain)
    bad = cli(base + ["--precond", "ilu"], rc=1)
    assert bad == "Invalid preconditioner (want none or jacobi)\n"
    if fmt == "csr":
        plain_k = cli(base + ["--rhs", "3"])
        out_k = cli(base + ["--rhs", "3", "--precond", "jacobi", "--check-every", "5"])
        assert "preconditioner: jacobi" in out_k and "preconditioner" not in plain_k
        assert all(a < c for a, c in zip(iterations(out_k), iterations(plain_k))), (iterations(out_k), iterations(plain_k))
        assert re.search(r"residual checks: \d+ passed, 0 failed", out_k)
