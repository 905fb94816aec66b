"""Every SpMV kernel the library can select, the vector kernels and the reductions, and the CG loop
under every context knob, on IEEE special values: +-0, subnormals, +-Inf, NaN, DBL_MAX, products
that overflow or underflow (tests/_ieee.py).  SpMV results and element-wise outputs must equal the
CPU oracle bit for bit (NaN payloads aside: _ieee.ieee_equal); reductions must equal the exact sum
where it is exact in every order, have its IEEE class otherwise, and lie within the error bound of
their summation tree when finite.  Also the exact thresholds of the layouts: the 16-bit column span
of the compact CSR blocks, the single-tile / tile-by-tile cut of the streaming CSR kernel, and the
fold of more than 8192 fused-dot partials."""
import ctypes as C
import math

import numpy as np
import pytest

import _ieee as I
from _ieee import ieee_diff, ieee_equal, value_class
from _oracle import COO, CSR, MODES, OracleMatrix, laplace5, ora_calc_p, ora_calc_xr, rhs

pytestmark = pytest.mark.gpu

FNAME = {CSR: "csr", COO: "coo"}


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


@pytest.fixture(scope="module")
def special():
    B = I.special_matrix()
    # for the bound of the fused p.w: no non-finite stored values, no DBL_MAX or overflowing rows, so
    # every term of x.y is of ordinary size and any partial dropped or counted twice exceeds the bound
    return B, B.without(["value_nonfinite", "max_order", "edge", "underflow"])


# name, format, environment, create_matrix keyword arguments, layout matrix_info must report,
# modes beyond none / sed / secded ("all": every mode; "constraints": that one too)
VARIANTS = [
    ("csr-stream", CSR, {}, {}, "stream", "all"),
    ("csr-stream-wide", CSR, {"ABFT_HIP_COMPACT_COLS": "0"}, {}, "stream", "all"),
    ("csr-panels-16-c0", CSR, {"ABFT_HIP_LAYOUT": "panels", "ABFT_HIP_PANEL_WIDTH": "16", "ABFT_HIP_PANEL_CHUNK": "0"},
     {}, "panels", ""),  # (constraints mode: CSR panels fall back to the streaming layout)
    ("csr-panels-257-c2", CSR, {"ABFT_HIP_LAYOUT": "panels", "ABFT_HIP_PANEL_WIDTH": "257", "ABFT_HIP_PANEL_CHUNK": "2"},
     {}, "panels", ""),
    ("csr-sweep-8-lag0", CSR, {"ABFT_HIP_LAYOUT": "sweep", "ABFT_HIP_PANEL_WIDTH": "16", "ABFT_HIP_SWEEP_RPT": "8",
                               "ABFT_HIP_SWEEP_LAG": "0"}, {}, "sweep", "constraints"),
    ("csr-sweep-16-lag2", CSR, {"ABFT_HIP_LAYOUT": "sweep", "ABFT_HIP_PANEL_WIDTH": "257", "ABFT_HIP_SWEEP_RPT": "16",
                                "ABFT_HIP_SWEEP_LAG": "2"}, {}, "sweep", "constraints"),
    ("csr-slice-16", CSR, {"ABFT_HIP_LAYOUT": "slice", "ABFT_HIP_PANEL_WIDTH": "16", "ABFT_HIP_SLICE_ROWS": "16"},
     {}, "slice", ""),
    ("csr-slice-1024", CSR, {"ABFT_HIP_LAYOUT": "slice", "ABFT_HIP_PANEL_WIDTH": "257", "ABFT_HIP_SLICE_ROWS": "1024"},
     {}, "slice", ""),
    ("coo-stream", COO, {}, {}, "stream", "all"),
    ("coo-panels-chunked", COO, {"ABFT_HIP_LAYOUT": "panels", "ABFT_HIP_PANEL_WIDTH": "64", "ABFT_HIP_PANEL_LAG": "0"},
     {}, "panels", "constraints"),
    ("coo-panels-paced-grid1", COO, {"ABFT_HIP_LAYOUT": "panels", "ABFT_HIP_PANEL_WIDTH": "64", "ABFT_HIP_PANEL_LAG": "2",
                                     "ABFT_HIP_PANEL_GRID": "1"}, {}, "panels", "constraints"),
    ("coo-panels-paced", COO, {"ABFT_HIP_LAYOUT": "panels", "ABFT_HIP_PANEL_WIDTH": "64", "ABFT_HIP_PANEL_LAG": "2"},
     {}, "panels", "constraints"),
    ("coo-pc", COO, {"ABFT_HIP_LAYOUT": "panels", "ABFT_HIP_PANEL_WIDTH": "64", "ABFT_HIP_COO_PC": "1"}, {}, "panels", ""),
    ("coo-lean", COO, {"ABFT_HIP_LAYOUT": "panels", "ABFT_HIP_PANEL_WIDTH": "64", "ABFT_HIP_COO_LEAN": "1"}, {}, "panels", ""),
    ("coo-xpf", COO, {"ABFT_HIP_LAYOUT": "panels", "ABFT_HIP_PANEL_WIDTH": "64", "ABFT_HIP_PANEL_XPF": "1"}, {}, "panels", ""),
]


def variant_modes(extra):
    if extra == "all":
        return MODES
    return ["none", "sed", "secded"] + (["constraints"] if extra == "constraints" else [])


CASES = [pytest.param(v, m, id="%s-%s" % (v[0], m)) for v in VARIANTS for m in variant_modes(v[5])]
# a fused SpMV partial sums at most a workgroup's rows (streaming: 4 * 256 row segments per block;
# slice: ABFT_HIP_SLICE_ROWS <= 1024), each thread a share of them: 1024 bounds every layout here
ROWS_PER_THREAD = 1024


class Run:
    """one HIPContext (events collected, not printed), a matrix, x and y"""

    def __init__(self, amd, fmt, mode, mat, **kw):
        self.events, self.fatal = [], False
        self.ctx = amd.HIPContext(mode, FNAME[fmt], on_event=self._on)
        cols, rows, vals, n = mat
        self.n = n
        self.A = self.ctx.create_matrix(cols, rows, vals, n, len(vals), **kw)
        self.vx, self.vy = self.ctx.create_vector(n), self.ctx.create_vector(n)

    def _on(self, ev, fatal):
        self.events += ev
        self.fatal |= fatal

    def spmv(self, x, A=None):
        """-> (y, the fused x.y the dot behind the SpMV returns)"""
        self.ctx.upload(self.vx, x)
        self.ctx.upload(self.vy, np.full(self.n, np.nan))
        self.ctx.spmv(A or self.A, self.vx, self.vy)
        d = self.ctx.dot(self.vx, self.vy)
        return self.ctx.download(self.vy), d

    def take_events(self):
        self.ctx._drain()
        ev, f = self.events, self.fatal
        self.events, self.fatal = [], False
        return ev, f

    def close(self):
        self.ctx.close()


def check_fused(d, x, y, nblk=8192):
    with np.errstate(over="ignore", invalid="ignore"):
        terms = x * y
    want = I.exact_sum(terms)
    assert value_class(d) == value_class(want), (d, want)
    if math.isfinite(want):
        assert abs(d - want) <= I.sum_bound(terms, I.fused_depth(ROWS_PER_THREAD, nblk)), (d, want)


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("variant,mode", CASES)
def test_spmv_on_special_values(amd, special, variant, mode, monkeypatch):
    name, fmt, env, kw, layout, _ = variant
    set_env(monkeypatch, env)
    B, F = special
    mat = B.mat(fmt)
    o = OracleMatrix(fmt, mode, *mat)
    h = Run(amd, fmt, mode, mat, **kw)
    try:
        assert h.ctx.matrix_info(h.A)[0] == layout
        assert np.array_equal(h.ctx.stored_words(h.A), o.stored_words())
        want = o.spmv(B.x)
        assert o.events() == ([], False)
        for _ in range(2):
            y, d = h.spmv(B.x)
            assert ieee_equal(y, want), ieee_diff(y, want)
            assert h.take_events() == ([], False)
            check_fused(d, B.x, want)
        assert np.array_equal(h.ctx.stored_words(h.A), o.stored_words())
        # the same rows with every product finite: the fused p.w within the bound of its tree
        xf = F.finite_x()
        of = OracleMatrix(fmt, mode, *F.mat(fmt))
        Af = h.ctx.create_matrix(*F.mat(fmt)[:3], F.n, len(F.vals))
        wantf = of.spmv(xf)
        assert np.isfinite(wantf).all()
        yf, df = h.spmv(xf, Af)
        assert ieee_equal(yf, wantf), ieee_diff(yf, wantf)
        assert h.take_events() == ([], False)
        assert math.isfinite(df)
        check_fused(df, xf, wantf)
    finally:
        h.close()


@pytest.mark.parametrize("fmt", [CSR, COO])
@pytest.mark.parametrize("mode", ["sec7", "secded"])
def test_single_flip_on_a_nonfinite_value_is_repaired(amd, special, fmt, mode):
    """the hot-path parity test must not depend on the value being finite"""
    B, _ = special
    mat = B.mat(fmt)
    h = Run(amd, fmt, mode, mat)
    o = OracleMatrix(fmt, mode, *mat)
    try:
        c, r, v, n = mat
        targets = [int(i) for i in np.flatnonzero(~np.isfinite(v))]
        assert len(targets) >= 3
        vbit0 = 0 if fmt == CSR else 64  # first bit of the value
        for i in targets:
            for bit in (vbit0 + 3, vbit0 + 51, vbit0 + 62, vbit0 + 63):  # mantissa, quiet bit, exponent, sign
                o = OracleMatrix(fmt, mode, *mat)  # a fresh event list each time
                o.inject(i, [bit])
                h.ctx.inject_at(h.A, i, [bit])
                y, _ = h.spmv(B.x)
                want = o.spmv(B.x)
                ev = o.events()
                assert ieee_equal(y, want), (i, bit, ieee_diff(y, want))
                assert h.take_events() == ev and len(ev[0]) == 1 and not ev[1], (i, bit, ev)
                assert np.array_equal(h.ctx.stored_words(h.A), o.stored_words()), (i, bit)  # repaired, written back
    finally:
        h.close()


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v[0] in ("csr-stream", "csr-stream-wide", "csr-sweep-8-lag0",
                                                                        "coo-stream", "coo-panels-chunked")],
                         ids=lambda v: v[0])
def test_column_flip_past_n_in_on_a_nonfinite_value(amd, special, variant, monkeypatch):
    """mode none: a gather index moved past n_in reads x as 0.0, and Inf * 0.0 / NaN * 0.0 is NaN --
    the product is formed, not skipped (kernels.hip csr_consume, oracle gather)"""
    name, fmt, env, kw, layout, _ = variant
    set_env(monkeypatch, env)
    B, _ = special
    mat = B.mat(fmt)
    c, r, v, n = mat
    targets = [int(i) for i in np.flatnonzero(~np.isfinite(v))]
    gbit = 64 + 20 if fmt == CSR else 32 + 20  # gather index: CSR column word, COO row word
    o = OracleMatrix(fmt, "none", *mat)
    h = Run(amd, fmt, "none", mat, **kw)
    try:
        for i in targets:
            o.inject(i, [gbit])
            h.ctx.inject_at(h.A, i, [gbit])
        want = o.spmv(B.x)
        outs = [int(r[i] if fmt == CSR else c[i]) for i in targets]
        assert all(math.isnan(want[k]) for k in outs)
        for _ in range(2):
            y, _ = h.spmv(B.x)
            assert ieee_equal(y, want), ieee_diff(y, want)
        assert h.take_events() == ([], False)
        assert np.array_equal(h.ctx.stored_words(h.A), o.stored_words())
    finally:
        h.close()


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("mode", ["none", "constraints", "sed", "secded"])
def test_spmm_on_special_values(amd, special, k, mode):
    """spmm on the streaming layout: every column equals the oracle's SpMV of that column, the special
    x in a different column each time and ordinary or finite-special columns beside it"""
    B, _ = special
    mat = B.csr()
    n = B.n
    o = OracleMatrix(CSR, mode, *mat)
    h = Run(amd, CSR, mode, mat, layout="stream")
    try:
        X = np.empty((n, k))
        for j in range(k):
            X[:, j] = I.special_vector(n, 100 + j, I.FINITE_SPECIALS)
        X[:, (k - 1) // 2] = B.x
        vX, vY = h.ctx.create_block(n, k), h.ctx.create_block(n, k)
        h.ctx.upload(vX, X)
        h.ctx.upload(vY, np.full((n, k), np.nan))
        h.ctx.spmm(h.A, vX, vY, k)
        Y = h.ctx.download(vY)
        for j in range(k):
            want = o.spmv(np.ascontiguousarray(X[:, j]))
            assert ieee_equal(Y[:, j], want), (j, ieee_diff(Y[:, j], want))
        assert h.take_events() == ([], False)
    finally:
        h.close()


@pytest.mark.parametrize("mode", ["none", "secded"])
def test_spmv_in_two_parts_on_special_values(amd, special, mode):
    from abft_sparse_cg_amd import capi
    B, _ = special
    mat = B.csr()
    want = OracleMatrix(CSR, mode, *mat).spmv(B.x)
    h = Run(amd, CSR, mode, mat)
    try:
        h.ctx.set_interior(h.A, 40, B.n - 300)
        h.ctx.upload(h.vx, B.x)
        h.ctx.upload(h.vy, np.full(B.n, np.nan))
        h.ctx.spmv(h.A, h.vx, h.vy, capi.PART_INTERIOR)
        h.ctx.spmv(h.A, h.vx, h.vy, capi.PART_BOUNDARY)
        y = h.ctx.download(h.vy)
        assert ieee_equal(y, want), ieee_diff(y, want)
        assert h.take_events() == ([], False)
    finally:
        h.close()


@pytest.mark.parametrize("layout", ["sweep", "slice"])
@pytest.mark.parametrize("mode", ["none", "secded"])
def test_spmv_by_panel_ranges_on_special_values(amd, special, layout, mode, monkeypatch):
    from abft_sparse_cg_amd import capi
    monkeypatch.setenv("ABFT_HIP_LAYOUT", layout)
    monkeypatch.setenv("ABFT_HIP_PANEL_WIDTH", "64")
    B, _ = special
    mat = B.csr()
    want = OracleMatrix(CSR, mode, *mat).spmv(B.x)
    h = Run(amd, CSR, mode, mat)
    try:
        L, hc = h.ctx.L, h.ctx.h
        npan, width = C.c_int(0), C.c_int(0)
        capi.check(L.abft_hip_matrix_panels(h.A.h, C.byref(npan), C.byref(width)))
        sc = h.ctx.create_vector(2)
        h.ctx.upload(h.vx, B.x)
        h.ctx.upload(h.vy, np.full(B.n, np.nan))
        cuts = [0, 1, npan.value // 2, npan.value - 1, npan.value]
        for a, b in zip(cuts, cuts[1:]):
            capi.check(L.abft_hip_spmv_dot_range_dev(hc, h.A.h, h.vx.h, h.vy.h, 0, sc.device_ptr, a, b))
        y = h.ctx.download(h.vy)
        assert ieee_equal(y, want), ieee_diff(y, want)
        s = h.ctx.download(sc)[0]
        with np.errstate(over="ignore", invalid="ignore"):
            assert value_class(s) == value_class(I.exact_sum(B.x * want))
        assert h.take_events() == ([], False)
    finally:
        h.close()


# ------------------------------------------------------------ vector kernels --

SIZES = [1, 63, 64, 65, 255, 256, 257, 4097, 2 ** 20 + 3]


def vectors(ctx, n, *arrays):
    out = []
    for a in arrays:
        v = ctx.create_vector(n)
        ctx.upload(v, a)
        out.append(v)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_elementwise_kernels_on_special_values(amd, n):
    ctx = amd.HIPContext("none", "csr")
    try:
        x, r, p, w = (I.special_vector(n, s) for s in (1, 2, 3, 4))
        vx, vr, vp, vw, vc = vectors(ctx, n, x, r, p, w, np.zeros(n))
        for alpha in (0.37, -0.0, I.INF, 1e300):
            x1, r1 = x.copy(), r.copy()
            rr = ora_calc_xr(x1, r1, p, w, alpha)
            ctx.upload(vx, x)
            ctx.upload(vr, r)
            got = ctx.calc_xr(vx, vr, vp, vw, alpha)
            assert ieee_equal(ctx.download(vx), x1) and ieee_equal(ctx.download(vr), r1), alpha
            assert value_class(got) == value_class(rr)
        for beta in (1.7, -0.0, I.INF):
            p1 = p.copy()
            ora_calc_p(p1, r, beta)
            ctx.upload(vp, p)
            ctx.upload(vr, r)
            ctx.calc_p(vp, vr, beta)
            assert ieee_equal(ctx.download(vp), p1), beta
        ctx.copy_vector(vc, vx)
        assert np.array_equal(ctx.download(vc).view(np.uint64), ctx.download(vx).view(np.uint64))
    finally:
        ctx.close()


@pytest.mark.parametrize("n", SIZES)
def test_reductions_exact_and_classes(amd, n):
    ctx = amd.HIPContext("none", "csr")
    try:
        for kind in ("int", "sub", "negzero"):
            a, b = I.exact_pair(n, 7, kind)
            want = I.exact_sum(a * b)
            va, vb, vx, vw = vectors(ctx, n, a, b, np.zeros(n), np.zeros(n))
            got = ctx.dot(va, vb)
            assert I.ieee_equal([got], [want]), (kind, got, want)
            # calc_xr with alpha = 0: r stays a (a - 0 * w), x stays 0, the reduction is a.a
            want_rr = I.exact_sum(a * a)
            got_rr = ctx.calc_xr(vx, va, vb, vw, 0.0)
            assert I.ieee_equal([got_rr], [want_rr]), (kind, got_rr, want_rr)
            assert ieee_equal(ctx.download(va), a - 0.0 * np.zeros(n))
            for v in (va, vb, vx, vw):
                ctx.destroy_vector(v)
        # classes: one +Inf, +Inf with -Inf, a NaN (magnitudes well away from overflow)
        rng = np.random.default_rng(n)
        base = rng.standard_normal(n)
        for spec, cls in (([I.INF], "+inf"), ([-I.INF], "-inf"), ([I.INF, -I.INF], "nan"), ([I.QNAN], "nan"),
                          ([I.INF, I.QNAN], "nan")):
            if len(spec) > n:
                continue
            a = base.copy()
            pos = rng.choice(n, size=len(spec), replace=False)
            a[pos] = spec
            va, vo = vectors(ctx, n, a, np.ones(n))
            assert value_class(ctx.dot(va, vo)) == cls, spec
            ctx.destroy_vector(va)
            ctx.destroy_vector(vo)
        # heavy cancellation: within the bound of dot_kernel's tree
        a = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, size=n)
        b = rng.standard_normal(n)
        a[a == 0] = 1.0
        b[n // 2:] = -a[: n - n // 2] * b[: n - n // 2] / a[n // 2:]  # products cancel pairwise, nearly
        va, vb = vectors(ctx, n, a, b)
        got = ctx.dot(va, vb)
        t = a * b
        assert abs(got - I.exact_sum(t)) <= I.sum_bound(t, I.dot_depth(n))
    finally:
        ctx.close()


@pytest.mark.parametrize("n", SIZES)
def test_block_reductions_and_copies_on_special_values(amd, n):
    """dot_block, calc_xr_block, calc_p_block, copy_block with masks: each active column as its single
    kernel (reductions exact where exact, of the oracle's class otherwise; ieee_equal element-wise),
    inactive columns bit-identical"""
    k = 5
    rng = np.random.default_rng(n)
    ctx = amd.HIPContext("none", "csr")
    try:
        A = np.empty((n, k))
        Bv = np.empty((n, k))
        for j, kind in enumerate(("int", "sub", "negzero", "int", "sub")):
            A[:, j], Bv[:, j] = I.exact_pair(n, 20 + j, kind)
        vA, vB = ctx.create_block(n, k), ctx.create_block(n, k)
        ctx.upload(vA, A)
        ctx.upload(vB, Bv)
        d = ctx.dot_block(vA, vB, k)
        for j in range(k):
            assert I.ieee_equal([d[j]], [I.exact_sum(A[:, j] * Bv[:, j])]), j
        # calc_xr_block: columns 0 and 3 integers (r.r an exact sum of squares), column 1 r = -0.0 - 1 * (+0.0)
        # (every square +0.0: r.r must be +0.0), column 2 special values with alpha = +Inf, column 4 special values
        # with an ordinary alpha (a fused multiply-add would change r and x there); column 3 inactive
        ints = lambda: rng.integers(-8, 9, size=n).astype(np.float64)  # noqa: E731
        X = np.stack([I.special_vector(n, 40 + j) for j in range(k)], axis=1)
        R = np.stack([ints(), np.full(n, -0.0), I.special_vector(n, 50), ints(), I.special_vector(n, 60)], axis=1)
        P = np.stack([ints(), ints(), I.special_vector(n, 51), ints(), I.special_vector(n, 61)], axis=1)
        W = np.stack([ints(), np.zeros(n), I.special_vector(n, 52), ints(), I.special_vector(n, 62)], axis=1)
        vX, vR, vP, vW, vC = (ctx.create_block(n, k) for _ in range(5))
        for v, a in ((vX, X), (vR, R), (vP, P), (vW, W), (vC, np.zeros((n, k)))):
            ctx.upload(v, a)
        alpha = [2.0, 1.0, I.INF, -1.0, 0.37]
        active = 0b10111
        rr = ctx.calc_xr_block(vX, vR, vP, vW, k, alpha, active)
        gx, gr = ctx.download(vX), ctx.download(vR)
        for j in range(k):
            xj, rj = X[:, j].copy(), R[:, j].copy()
            if (active >> j) & 1:
                with np.errstate(all="ignore"):
                    rr_o = ora_calc_xr(xj, rj, np.ascontiguousarray(P[:, j]), np.ascontiguousarray(W[:, j]), alpha[j])
                if j < 2:
                    with np.errstate(all="ignore"):
                        want = I.exact_sum(rj * rj)
                    assert I.ieee_equal([rr[j]], [want]) and I.ieee_equal([rr_o], [want]), (j, rr[j], want)
                else:
                    assert value_class(rr[j]) == value_class(rr_o), (j, rr[j], rr_o)
                    assert j != 2 or value_class(rr_o) != "finite"
            assert ieee_equal(gx[:, j], xj) and ieee_equal(gr[:, j], rj), j
            if not (active >> j) & 1:
                assert np.array_equal(gx[:, j].view(np.uint64), X[:, j].view(np.uint64))
                assert np.array_equal(gr[:, j].view(np.uint64), R[:, j].view(np.uint64))
        assert math.copysign(1.0, rr[1]) == 1.0
        beta = [1.5, I.INF, -0.0, 0.25, 0.37]
        ctx.calc_p_block(vP, vR, k, beta, 0b10111)
        gp = ctx.download(vP)
        for j in range(k):
            pj = P[:, j].copy()
            if (0b10111 >> j) & 1:
                with np.errstate(all="ignore"):
                    ora_calc_p(pj, np.ascontiguousarray(gr[:, j]), beta[j])
                assert ieee_equal(gp[:, j], pj), j
            else:
                assert np.array_equal(gp[:, j].view(np.uint64), P[:, j].view(np.uint64))
        ctx.copy_block(vC, vX, k, 0b0101)
        gc = ctx.download(vC)
        for j in range(k):
            assert np.array_equal(gc[:, j].view(np.uint64), (gx[:, j] if (0b0101 >> j) & 1 else np.zeros(n)).view(np.uint64))
    finally:
        ctx.close()


def tridiagonal(n):
    """integer tridiagonal matrix (2 on the diagonal, -1 beside it), elements sorted by (row, col)"""
    i = np.arange(n)
    rows = np.concatenate([i[1:], i, i[:-1]])
    cols = np.concatenate([i[:-1], i, i[1:]])
    vals = np.concatenate([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)])
    order = np.lexsort((cols, rows))
    return cols[order].astype(np.uint32), rows[order].astype(np.uint32), vals[order], n


BAD_STATES = (("x", I.QNAN), ("x", I.INF), ("r", I.QNAN), ("r", -I.INF))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fmt", [CSR, COO])
def test_residual_checks_see_nonfinite_vectors(amd, fmt, n):
    """residual_gap on an x or r that holds NaN or Inf returns a non-finite gap, so the check fails; on
    integer data whose r is b - A x it returns exactly +0.0 and the exact sum of squares;
    residual_restart's r.r is dot(r, r)'s bits and r, p are b - A x element for element"""
    mat = tridiagonal(n)
    rng = np.random.default_rng(n)
    b = rng.integers(-9, 10, size=n).astype(np.float64)
    x0 = rng.integers(-9, 10, size=n).astype(np.float64)
    o = OracleMatrix(fmt, "none", *mat)
    ctx = amd.HIPContext("none", FNAME[fmt])
    try:
        A = ctx.create_matrix(*mat[:3], n, len(mat[2]))
        t = b - o.spmv(x0)
        vb, vx, vr, vs = vectors(ctx, n, b, x0, t, np.zeros(n))
        gap2, tt2 = ctx.residual_gap(A, vb, vx, vr, vs)
        assert I.ieee_equal([gap2, tt2], [0.0, I.exact_sum(t * t)]), (gap2, tt2)
        for v in (vb, vx, vr, vs):
            ctx.destroy_vector(v)
        for which, bad in BAD_STATES:
            x = x0.copy()
            r = b - o.spmv(x)
            (x if which == "x" else r)[n // 3] = bad
            vb, vx, vr, vp, vs = vectors(ctx, n, b, x, r, np.zeros(n), np.zeros(n))
            gap2, tt2 = ctx.residual_gap(A, vb, vx, vr, vs)
            assert not math.isfinite(gap2), (which, bad, gap2)
            assert math.isfinite(tt2) == (which == "r"), (which, tt2)
            rr = ctx.residual_restart(A, vb, vx, vr, vp, vs)
            want_r = b - o.spmv(x)
            assert ieee_equal(ctx.download(vr), want_r) and ieee_equal(ctx.download(vp), want_r)
            assert I.ieee_equal([rr], [ctx.dot(vr, vr)])
            if which == "r":  # x is clean: r = b - A x again, r.r exact
                assert I.ieee_equal([rr], [I.exact_sum(want_r * want_r)])
            for v in (vb, vx, vr, vp, vs):
                ctx.destroy_vector(v)
    finally:
        ctx.close()


@pytest.mark.parametrize("n", SIZES)
def test_residual_block_forms_see_nonfinite_columns(amd, n):
    """residual_gap_block / residual_restart_block with masks: column 0 clean integers (gap exactly +0.0,
    sums exact), column 1 with a NaN in x, column 2 with an Inf in r (non-finite gaps); a column outside
    the mask reads 0.0 from the gap and keeps its R and P bits through the restart"""
    k = 3
    mat = tridiagonal(n)
    rng = np.random.default_rng(n + 1)
    o = OracleMatrix(CSR, "none", *mat)
    Bm = rng.integers(-9, 10, size=(n, k)).astype(np.float64)
    Xm = rng.integers(-9, 10, size=(n, k)).astype(np.float64)
    Xm[n // 2, 1] = I.QNAN
    Tm = np.stack([Bm[:, j] - o.spmv(np.ascontiguousarray(Xm[:, j])) for j in range(k)], axis=1)
    Rm = Tm.copy()
    Rm[n // 3, 2] = I.INF
    ctx = amd.HIPContext("none", "csr")
    try:
        A = ctx.create_matrix(*mat[:3], n, len(mat[2]))
        vB, vX, vR, vP, vS = (ctx.create_block(n, k) for _ in range(5))
        for v, a in ((vB, Bm), (vX, Xm), (vR, Rm), (vP, np.full((n, k), 5.0))):
            ctx.upload(v, a)
        gap2, tt2 = ctx.residual_gap_block(A, vB, vX, vR, vS, k, 0b111)
        assert I.ieee_equal([gap2[0], tt2[0]], [0.0, I.exact_sum(Tm[:, 0] ** 2)]), (gap2, tt2)
        assert not math.isfinite(gap2[1]) and not math.isfinite(tt2[1])
        assert not math.isfinite(gap2[2]) and I.ieee_equal([tt2[2]], [I.exact_sum(Tm[:, 2] ** 2)])
        gap2, tt2 = ctx.residual_gap_block(A, vB, vX, vR, vS, k, 0b101)
        assert I.ieee_equal([gap2[1], tt2[1]], [0.0, 0.0]) and not math.isfinite(gap2[2]) and gap2[0] == 0.0
        rr = ctx.residual_restart_block(A, vB, vX, vR, vP, vS, k, 0b110)
        gR, gP = ctx.download(vR), ctx.download(vP)
        assert np.array_equal(gR[:, 0].view(np.uint64), Rm[:, 0].view(np.uint64))
        assert np.all(gP[:, 0] == 5.0)
        for j in (1, 2):
            assert ieee_equal(gR[:, j], Tm[:, j]) and ieee_equal(gP[:, j], Tm[:, j]), j
        assert I.ieee_equal(rr, ctx.dot_block(vR, vR, k))
        assert I.ieee_equal([rr[0], rr[2]], [I.exact_sum(Rm[:, 0] ** 2), I.exact_sum(Tm[:, 2] ** 2)])
        assert math.isnan(rr[1])
    finally:
        ctx.close()


def nblk_of(ctx, A):
    c, t, m = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert ctx.L.abft_hip_matrix_compact_stats(A.h, C.byref(c), C.byref(t), C.byref(m)) == 0
    return c.value, t.value, m.value


def test_fused_dot_over_many_partials(amd):
    """more than 8192 SpMV row blocks: the fused p.w is folded by fold_partials_kernel.  Rows of
    TILE / 2 + 1 elements fill one block each (two do not fit a tile), the fewest elements that get
    there.  Exact inputs bit-equal to the exact sum, an exact 0 as +0.0, a NaN as NaN, cancellation
    within the bound."""
    tile = I.csr_tile()
    length = tile // 2 + 1
    n = 8200
    rows = np.repeat(np.arange(n, dtype=np.uint32), length)
    cols = ((rows.astype(np.int64) + np.tile(np.arange(length) * 13, n)) % n).astype(np.uint32)
    cols = cols.reshape(n, length)
    cols.sort(axis=1)
    cols = cols.reshape(-1)
    rng = np.random.default_rng(9)
    vals = rng.integers(-3, 4, size=len(cols)).astype(np.float64)
    o = OracleMatrix(CSR, "none", cols, rows, vals, n)
    h = Run(amd, CSR, "none", (cols, rows, vals, n))
    try:
        _, nblk, _ = nblk_of(h.ctx, h.A)
        assert nblk > 8192, nblk
        for kind in ("int", "negzero", "nan", "cancel"):
            if kind == "int":
                x = rng.integers(-4, 5, size=n).astype(np.float64)
            elif kind == "negzero":
                x = np.full(n, -0.0)
            elif kind == "nan":
                x = rng.integers(-4, 5, size=n).astype(np.float64)
                x[n - 3] = I.QNAN
            else:
                x = rng.standard_normal(n) * 10.0 ** rng.integers(-5, 6, size=n)
            want = o.spmv(x)
            y, d = h.spmv(x)
            assert ieee_equal(y, want), ieee_diff(y, want)
            terms = x * want
            ex = I.exact_sum(terms)
            if kind in ("int", "negzero"):
                assert I.ieee_equal([d], [ex]) and (kind != "negzero" or math.copysign(1.0, d) == 1.0), (kind, d, ex)
            elif kind == "nan":
                assert math.isnan(d)
            else:
                assert abs(d - ex) <= I.sum_bound(terms, I.fused_depth(4, nblk)), (d, ex)
        assert h.take_events() == ([], False)
    finally:
        h.close()


# ------------------------------------------------------------- layout edges --

def compact_matrix(extra_col, n=70000):
    """diagonal, plus row 1 reaching column extra_col: block 0 spans columns [0, extra_col]"""
    rows = np.arange(n, dtype=np.uint32)
    cols = np.arange(n, dtype=np.uint32)
    rows = np.insert(rows, 2, 1)
    cols = np.insert(cols, 2, extra_col)
    vals = 1.0 + np.random.default_rng(5).random(len(rows))
    return cols, rows.astype(np.uint32), vals, n


@pytest.mark.parametrize("span,compact", [(65535, True), (65536, False)])
def test_compact_column_span_threshold(amd, span, compact):
    cols, rows, vals, n = compact_matrix(span)
    x = I.special_vector(n, 8, I.FINITE_SPECIALS)
    x[65535], x[65536] = 3.0, -5.0
    h = Run(amd, CSR, "none", (cols, rows, vals, n), layout="stream")
    o = OracleMatrix(CSR, "none", cols, rows, vals, n)
    try:
        c, t, m = nblk_of(h.ctx, h.A)
        assert (c == t) == compact and c >= t - 1 and m == 0, (c, t, m)
        y, _ = h.spmv(x)
        assert ieee_equal(y, o.spmv(x))
    finally:
        h.close()


@pytest.mark.parametrize("bits,keeps", [(list(range(64, 80)), True), ([64 + 16], False)])
def test_compact_inject_at_the_span_threshold(amd, bits, keeps):
    """element (0, 0) of a block whose base is 0 moved to column 65535 (base + 65535: stays compact)
    or to 65536 (base + 65536: the block widens); y and events as the oracle's"""
    cols, rows, vals, n = compact_matrix(1000)
    x = I.special_vector(n, 9, I.FINITE_SPECIALS)
    x[65535], x[65536] = I.INF, I.QNAN
    h = Run(amd, CSR, "none", (cols, rows, vals, n), layout="stream")
    o = OracleMatrix(CSR, "none", cols, rows, vals, n)
    try:
        c0, t, _ = nblk_of(h.ctx, h.A)
        assert c0 == t
        h.ctx.inject_at(h.A, 0, bits)
        o.inject(0, bits)
        assert int(o.csr_arrays()[0][0]) == (65535 if keeps else 65536)
        c, t2, m = nblk_of(h.ctx, h.A)
        assert t2 == t and m == 0 and c == (t if keeps else t - 1), (c, t, m)
        for _ in range(2):
            y, _ = h.spmv(x)
            want = o.spmv(x)
            assert ieee_equal(y, want), ieee_diff(y, want)
            assert not math.isfinite(y[0])
        assert h.take_events() == o.events() == ([], False)
    finally:
        h.close()


@pytest.mark.parametrize("mode", MODES)
def test_tile_edges_on_csr_stream(amd, mode):
    """rows of TILE - 1 .. 2 TILE + 1 elements, blocks starting at even and odd elements: the single-tile
    branch and the tile-by-tile branch, special values at both ends of every tile"""
    T, named = I.tile_edge_matrix()
    mat = T.csr()
    o = OracleMatrix(CSR, mode, *mat)
    h = Run(amd, CSR, mode, mat, layout="stream")
    try:
        want = o.spmv(T.x)
        for r in named.values():
            assert want[r] == I.INF or math.isfinite(want[r])
        for _ in range(2):
            y, _ = h.spmv(T.x)
            assert ieee_equal(y, want), [(k, y[r], want[r]) for k, r in named.items() if not ieee_equal([y[r]], [want[r]])]
        assert h.take_events() == o.events() == ([], False)
        if mode in ("sec7", "secded"):
            c, r, v, n = mat
            rowptr = np.searchsorted(r, np.arange(n + 1))
            hits = {}
            for name in ("order/%d/odd" % I.csr_tile(), "last_inf/%d/even" % (2 * I.csr_tile() + 1)):
                row = named[name]
                for i in (rowptr[row], rowptr[row + 1] - 1, rowptr[row] + I.csr_tile() - 1):
                    hits[int(i)] = 1  # (each element once: two flips would be a double error)
            for k, i in enumerate(hits):
                o.inject(i, [5 + 11 * k])
                h.ctx.inject_at(h.A, i, [5 + 11 * k])
            y, _ = h.spmv(T.x)
            want = o.spmv(T.x)
            assert ieee_equal(y, want)
            assert sorted(h.take_events()[0]) == sorted(o.events()[0])
    finally:
        h.close()


# ------------------------------------------------------------ CG edge cases --

KNOBS = [{}, {"ABFT_HIP_TAIL": "0"}, {"ABFT_HIP_FUSE_DOT": "0"}, {"ABFT_HIP_FUSE_X": "0"}, {"ABFT_HIP_SYNC": "stream"},
         {"ABFT_HIP_SPECULATE": "1"}]


def knob_id(env):
    return ",".join("%s=%s" % kv for kv in env.items()) or "default"


def cg_gpu(amd, fmt, mat, b, conv, max_itrs=1000):
    cols, rows, vals, n = mat
    ctx = amd.HIPContext("none", FNAME[fmt])
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        x0 = np.full(n, 7.0)  # b = 0: x must be left as it is (never touched)
        vb, vx, vr, vp, vw = vectors(ctx, n, b, x0 if not np.any(b) else np.zeros(n), np.zeros(n), np.zeros(n),
                                     np.zeros(n))
        hist = []
        it, rr = amd.cg_solve(ctx, A, vb, vx, vr, vp, vw, max_itrs=max_itrs, conv_threshold=conv,
                              on_iteration=lambda i, r: hist.append(r))
        return it, rr, ctx.download(vx), hist
    finally:
        ctx.close()


def cg_cases(n):
    rng = np.random.default_rng(4)
    ints = rng.integers(-5, 6, size=n).astype(np.float64)
    b_nan = rhs(n, 2)
    b_nan[n // 2] = I.QNAN
    b_inf = rhs(n, 2)
    b_inf[n // 3] = I.INF
    return {"zero": np.zeros(n), "ints": ints, "nan": b_nan, "inf": b_inf}


@pytest.mark.parametrize("env", KNOBS, ids=knob_id)
@pytest.mark.parametrize("fmt", [CSR, COO])
def test_cg_edges_under_every_knob(amd, fmt, env, monkeypatch):
    set_env(monkeypatch, env)
    n = 257
    scaled = (np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.full(n, 2.0 ** 5), n)
    lap = laplace5(16, 16)
    B = cg_cases(n)
    for case, b in B.items():
        mat = scaled
        conv = 0.0 if case == "ints" else 1e-3
        it, rr, x, hist = cg_gpu(amd, fmt, mat, b, conv)
        o = OracleMatrix(fmt, "none", *mat)
        it_o, h_o, x_o, fatal = o.cg(b, conv=conv)
        assert it == it_o, (case, it, it_o)
        if case == "zero":
            assert it == 0 and np.all(x == 7.0)
        elif case == "ints":
            assert it == 1 and rr == 0.0 and math.copysign(1.0, rr) == 1.0
            assert ieee_equal(x, x_o) and np.array_equal(x, b * 2.0 ** -5)
        elif case == "nan":
            assert it == 0 and np.all(x == 0.0)
        else:
            assert ieee_equal(np.isnan(x), np.isnan(x_o)) and ieee_equal(np.isinf(x), np.isinf(x_o))
            assert ieee_equal(np.where(np.isfinite(x_o), 0.0, x), np.where(np.isfinite(x_o), 0.0, x_o))
    b = rhs(lap[3], 1)
    it, rr, x, hist = cg_gpu(amd, fmt, lap, b, 1e-3)
    it_o, h_o, x_o, _ = OracleMatrix(fmt, "none", *lap).cg(b)
    assert it == it_o
    assert np.all(np.abs(np.array(hist) - h_o) <= 1e-10 * np.abs(h_o))


@pytest.mark.parametrize("env", KNOBS, ids=knob_id)
def test_cg_solve_block_columns_in_edge_states(amd, env, monkeypatch):
    """one column per edge state (b = 0, exact 2^k I, NaN, Inf) beside a normal one: each column follows
    its own cg_solve"""
    set_env(monkeypatch, env)
    n = 257
    mat = (np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.full(n, 2.0 ** 5), n)
    cases = cg_cases(n)
    cols = [cases["zero"], cases["ints"], cases["nan"], cases["inf"], rhs(n, 6)]
    k = len(cols)
    Bm = np.stack(cols, axis=1)
    for conv in (0.0, 1e-3):
        ctx = amd.HIPContext("none", "csr")
        try:
            A = ctx.create_matrix(*mat[:3], n, n)
            vB, vX, vR, vP, vW = (ctx.create_block(n, k) for _ in range(5))
            ctx.upload(vB, Bm)
            X0 = np.zeros((n, k))
            X0[:, 0] = 7.0  # b = 0: the column must be left as it is, not zeroed
            ctx.upload(vX, X0)
            itrs, rr = amd.cg_solve_block(ctx, A, vB, vX, vR, vP, vW, conv_threshold=conv)
            X = ctx.download(vX)
        finally:
            ctx.close()
        for j in range(k):
            it_j, rr_j, x_j, _ = cg_gpu(amd, CSR, mat, np.ascontiguousarray(Bm[:, j]), conv)
            assert itrs[j] == it_j, (conv, j, itrs, it_j)
            assert I.ieee_equal([rr[j]], [rr_j]), (conv, j, rr[j], rr_j)
            if j == 0:
                assert np.all(X[:, 0] == 7.0) and itrs[0] == 0
            else:
                assert ieee_equal(X[:, j], x_j), (conv, j, ieee_diff(X[:, j], x_j))
