"""The guarded Jacobi iteration on protected vectors (abft_hip_pcg_vecc_iteration_until_dev) and the two solvers
built on it and on the host-scalar entries: cg_solve / cg_solve_device(vector_ecc=True, precond=ctx.jacobi(A,
protected=True)) -- DESIGN.md section 5l.

The yardsticks: a LIVE iteration is held bit for bit against the three host calls it stands for (spmv_vecc with its
fused product, calc_r_precond_vecc, calc_px_precond_vecc -- themselves held against the numpy model in
test_gpu_vecc_precond.py), a FROZEN one against its definition, the host solve against the model loop of
tests/_vecc_precond.py over the range test_vecc_precond_host.py fixed on the CPU, the device solve against the host
solve.  Every matrix is CSR in the streaming layout.

Events are (kind, index, bit | operand << 8); the guarded entry counts its vector arguments vec, x, r, p, w, dinv as
operands 0..5."""
import math

import numpy as np
import pytest

import _matrices
import _vecc
import _vecc_precond as P
from _oracle import rhs
from test_gpu_vector_ecc import CORRECTED, Box, bits_of, ragged
from test_vecc_precond_host import HISTORY_BAR, HISTORY_THRESHOLD, MAX_ITRS, SYSTEM, model_run

pytestmark = pytest.mark.gpu

U = np.uint64
IN, PW, OUT = 0, 4, 8  # the record read, the SpMV's pair, the record written: doubles 0..3, 4..5, 8..11


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


class Loop:
    """x, r, p, w, a protected dinv and twelve scalars {rr, ev, rz, 0 | pw, ev, -, - | rr', ev, rz', 0} on a Box"""

    def __init__(self, amd, mode, mat, seed=1, fmt="csr", layout="stream", start=True):
        cols, rows, vals, n = mat
        self.n, self.box = n, Box(amd, mode, fmt)
        self.ctx = self.box.ctx
        self.A = self.ctx.create_matrix(cols, rows, vals, n, len(vals), layout=layout)
        rng = np.random.default_rng(seed)
        self.start = [_vecc.encode(rng.standard_normal(n)) for _ in range(3)] + [np.zeros(n, U)]
        self.dw = _vecc.encode(10.0 ** rng.uniform(-2, 2, n))
        self.x, self.r, self.p, self.w = (self.box.vec(a) for a in self.start)
        self.d = self.box.vec(self.dw)
        self.sc = self.ctx.create_vector(12)
        if start:  # one eager preconditioned call: the context holds its block partials from here on
            self.ctx.precond_start_vecc(self.r, self.d, self.w)

    def vecs(self):
        return self.x, self.r, self.p, self.w

    def reset(self, rr, rz):
        for v, a in zip(self.vecs(), self.start):
            self.ctx.upload(v, a.view(np.float64))
        self.ctx.upload(self.d, self.dw.view(np.float64))
        self.ctx.upload(self.sc, np.array([rr, 0, rz, 0] + [0.0] * 8))

    def words(self):
        return [self.box.words(v) for v in self.vecs()]

    def scalars(self):
        return self.ctx.download(self.sc).view(U).copy()

    def until(self, thr, **kw):
        self.ctx.pcg_vecc_iteration_until_dev(self.A, self.p, self.x, self.r, self.p, self.w, self.d, self.sc, IN, PW, OUT,
                                              thr, **kw)

    def host(self, rz):
        """the host-scalar calls the live iteration stands for -> (p.w, rz_new, rr_new)"""
        ctx = self.ctx
        ctx.spmv_vecc(self.A, self.p, self.w)
        pw = ctx.dot_vecc(self.p, self.w)  # served from the fused product
        alpha = P.fdiv(rz, pw)
        rz_new, rr_new = ctx.calc_r_precond_vecc(self.r, self.w, self.d, alpha)
        ctx.calc_px_precond_vecc(self.x, self.p, self.r, self.d, alpha, P.fdiv(rz_new, rz))
        return pw, rz_new, rr_new

    def close(self):
        self.ctx.close()


# lap40 is the matrix of the sibling test (test_gpu_device_loop_vecc.py: laplace5(40, 40)), lap37x41 the odd length
# whose walk by pairs has a tail; `ragged` is the sibling's second matrix (a row longer than a tile, empty rows)
MATRICES = {"lap40": lambda: _matrices.matrix("lap40"), "lap37x41": lambda: _matrices.matrix("lap37x41"), "ragged": ragged}


@pytest.mark.parametrize("mode", ["none", "secded"])
@pytest.mark.parametrize("matrix", sorted(MATRICES))
def test_live_iteration_is_the_three_host_calls_bit_for_bit(amd, mode, matrix):
    lp = Loop(amd, mode, MATRICES[matrix]())
    rr, rz = 3.25, 2.75
    lp.reset(rr, rz)
    pw, rz_new, rr_new = lp.host(rz)
    want = lp.words()
    assert lp.box.take() == []
    lp.reset(rr, rz)
    lp.until(0.0)
    got, sc = lp.words(), lp.scalars()
    for name, g, w in zip("xrpw", got, want):
        assert np.array_equal(g, w), (matrix, mode, name)
    assert sc[PW] == bits_of(pw) and sc[OUT] == bits_of(rr_new) and sc[OUT + 2] == bits_of(rz_new), (sc, pw, rz_new, rr_new)
    assert sc[IN] == bits_of(rr) and sc[IN + 2] == bits_of(rz)  # what was read is left alone
    assert sc[IN + 1] == 0 and sc[PW + 1] == 0 and sc[OUT + 1] == 0 and sc[OUT + 3] == 0  # nothing queued; 0.0
    assert np.array_equal(lp.box.words(lp.d), lp.dw) and lp.box.take() == []
    assert lp.ctx.tail_stats() == (0, 0, 0, [0, 0, 0, 0])  # left alone
    # the words of the model, fed with the device's three sums
    m = P.iteration(_vecc.csr_of(*MATRICES[matrix]()), *lp.start[:3], lp.dw, (rr, rz), 0.0, p_dot_w=pw, sums=(rz_new, rr_new))
    for name, g in zip("xrpw", got):
        _vecc.assert_words(g, m[name], name)
    # a second iteration from there, the record read where the first left it
    lp.ctx.upload(lp.sc, np.array([rr_new, 0, rz_new, 0] + [0.0] * 8))
    lp.until(0.0)
    got2, sc2 = lp.words(), lp.scalars()
    for v, a in zip(lp.vecs(), want):
        lp.ctx.upload(v, a.view(np.float64))
    pw2, rz2, rr2 = lp.host(rz_new)
    for name, g, w in zip("xrpw", got2, lp.words()):
        assert np.array_equal(g, w), (matrix, mode, name, "second")
    assert sc2[PW] == bits_of(pw2) and sc2[OUT] == bits_of(rr2) and sc2[OUT + 2] == bits_of(rz2)
    lp.close()


def test_live_iteration_reports_flips_under_the_entrys_ordinals(amd):
    """x 1, r 2, p 3 (and 0: the SpMV gathers it), dinv 5.  (w, 4, is rewritten by the SpMV before the r half reads
    it: no flip planted before the call survives to be reported; its cold path is the host-scalar entry's, whose
    ordinal for w test_gpu_vecc_precond.py checks)"""
    lp = Loop(amd, "secded", _matrices.matrix("lap40"))
    rr, rz, at = 3.25, 2.75, 20 * 40 + 20
    lp.reset(rr, rz)
    lp.until(0.0)
    want, sc0 = lp.words(), lp.scalars()
    assert lp.box.take() == []
    vec = dict(x=lp.x, r=lp.r, p=lp.p, w=lp.w, dinv=lp.d)
    for name, bit, ops in (("p", 55, [0, 3]), ("p", 0, [0, 3]), ("x", 3, [1]), ("r", 62, [2]), ("dinv", 44, [5]),
                           ("dinv", 0, [5]), ("w", 9, [])):
        lp.reset(rr, rz)
        lp.ctx.flip_vector(vec[name], at, [bit])
        lp.until(0.0)
        got, sc = lp.words(), lp.scalars()
        for k, g, w in zip("xrpw", got, want):
            assert np.array_equal(g, w), (name, bit, k)  # x, r and p rewritten: the clean iteration's words
        assert sc[PW] == sc0[PW] and sc[OUT] == sc0[OUT] and sc[OUT + 2] == sc0[OUT + 2]
        assert np.array_equal(lp.box.words(lp.d), lp.dw), name  # dinv: the repaired word stored back
        assert lp.box.take() == [(CORRECTED, at, bit | op << 8) for op in ops], (name, bit)
    assert P.OPERAND == {"vec": 0, "x": 1, "r": 2, "p": 3, "w": 4, "dinv": 5}
    lp.close()


PAYLOAD = np.array([0x7FF8000000ABCDEF], U).view(np.float64)
RZ_PAYLOAD = np.array([0xFFF8000000012345], U).view(np.float64)


@pytest.mark.parametrize("case", ["equal", "above", "nan_payload"])
def test_frozen_iteration_keeps_every_word_and_hands_the_record_on(amd, case):
    rr, thr = {"equal": (0.1 + 0.2, 0.1 + 0.2), "above": (5.0, math.inf), "nan_payload": (float(PAYLOAD[0]), 0.0)}[case]
    lp = Loop(amd, "secded", _matrices.matrix("lap40"))
    at = 20 * 40 + 20
    lp.reset(rr, 1.5)
    first = np.concatenate([PAYLOAD if case == "nan_payload" else [rr], [0.0], RZ_PAYLOAD, [7.0]])
    lp.ctx.upload(lp.sc, np.concatenate([first, [7.0] * 8]))
    for v, bit in ((lp.x, 12), (lp.r, 0), (lp.d, 55)):  # one flipped word in each: a frozen launch repairs nothing
        lp.ctx.flip_vector(v, at, [bit])
    pre, pre_d, pre_sc = lp.words(), lp.box.words(lp.d), lp.scalars()
    assert not np.array_equal(pre[0], lp.start[0]) and not np.array_equal(pre_d, lp.dw)

    def check(what):
        post, sc = lp.words(), lp.scalars()
        for name, a, b in zip("xrp", post, pre):
            assert np.array_equal(a, b), (case, what, name)
        assert np.array_equal(lp.box.words(lp.d), pre_d), (case, what)
        assert sc[OUT] == pre_sc[IN] and sc[OUT + 2] == pre_sc[IN + 2]  # the record's bits moved on ...
        assert np.array_equal(sc[IN:IN + 4], pre_sc[IN:IN + 4])  # ... what was read left alone
        assert sc[OUT + 1] == 0 and sc[OUT + 3] == 0  # no event queued; 0.0
        assert lp.box.take() == [], (case, what)  # no vector event: p is clean, the two vector kernels returned at once

    lp.until(thr)
    check("eager")
    lp.ctx.graph_begin()
    try:
        lp.until(thr)
    finally:
        g = lp.ctx.graph_end()
    for replay in range(3):  # captured and replayed: nothing changes
        lp.ctx.graph_launch(g)
        check(replay)
    lp.ctx.graph_destroy(g)
    lp.close()


def test_capture_needs_one_eager_precond_start_vecc(amd):
    mat = _matrices.matrix("lap40")
    rr, rz = 3.25, 2.75
    lp = Loop(amd, "none", mat)
    lp.reset(rr, rz)
    lp.until(0.0)
    want, sc0 = lp.words(), lp.scalars()
    lp.close()
    lp = Loop(amd, "none", mat, start=False)  # a fresh context: no preconditioned call yet
    lp.reset(rr, rz)
    spare = lp.ctx.create_vector(lp.n)
    lp.ctx.graph_begin()
    try:
        lp.ctx.copy_vector(spare, lp.r)  # (something to capture: the refused call adds nothing)
        with pytest.raises(amd.AbftError, match="pcg_vecc_iteration_until: .*graph capture.*abft_hip_precond_start_vecc"):
            lp.until(0.0)
    finally:
        lp.ctx.graph_destroy(lp.ctx.graph_end())
    assert all(np.array_equal(a, b) for a, b in zip(lp.words(), lp.start))
    lp.ctx.precond_start_vecc(lp.r, lp.d, lp.w)  # the remedy
    lp.reset(rr, rz)
    lp.ctx.graph_begin()
    try:
        lp.until(0.0)
    finally:
        g = lp.ctx.graph_end()
    lp.ctx.graph_launch(g)
    for name, a, b in zip("xrpw", lp.words(), want):
        assert np.array_equal(a, b), name
    assert np.array_equal(lp.scalars(), sc0)
    lp.ctx.graph_destroy(g)
    lp.close()


def test_refusals_leave_every_vector_and_record_untouched(amd, monkeypatch):
    mat = _matrices.matrix("lap40")

    def refused(lp, call, text, extra=()):
        vs = list(lp.vecs()) + [lp.d] + list(extra)
        pre, pre_sc = [lp.box.words(v) for v in vs], lp.scalars()
        with pytest.raises(amd.AbftError, match=text):
            call()
        assert all(np.array_equal(lp.box.words(v), a) for v, a in zip(vs, pre)), text
        assert np.array_equal(lp.scalars(), pre_sc) and lp.box.take() == [], text

    # everything abft_hip_cg_vecc_iteration_until_dev refuses about the matrix
    lp = Loop(amd, "secded", mat, fmt="coo", layout=None)
    lp.reset(3.25, 2.75)
    refused(lp, lambda: lp.until(0.0), "pcg_vecc_iteration_until: .*COO")
    lp.close()
    for layout, name in (("panels", "panel"), ("sweep", "sweep")):
        monkeypatch.setenv("ABFT_HIP_LAYOUT", layout)
        lp = Loop(amd, "secded", mat, layout=None)
        assert lp.ctx.matrix_info(lp.A)[0] == layout
        lp.reset(3.25, 2.75)
        refused(lp, lambda: lp.until(0.0), "pcg_vecc_iteration_until: .*" + name)
        lp.close()
    monkeypatch.delenv("ABFT_HIP_LAYOUT")

    lp = Loop(amd, "secded", mat)
    lp.reset(3.25, 2.75)
    ctx, n, A = lp.ctx, lp.n, lp.A
    marks = _vecc.encode(np.arange(1.0, n + 1.0))
    short = lp.box.vec(marks[:-1])
    both = lp.box.vec(np.concatenate([marks, marks]))
    lo, hi = ctx.view_vector(both, 0, n), ctx.view_vector(both, n - 1, n)  # one entry shared
    extra = [short, both]
    x, r, p, w = lp.vecs()

    def call(vecs=None, at=(IN, PW, OUT), vec=None, dinv=None, **kw):
        vx, vr, vp, vw = vecs or (x, r, p, w)
        return lambda: ctx.pcg_vecc_iteration_until_dev(A, vec or vp, vx, vr, vp, vw, dinv or lp.d, lp.sc, at[0], at[1],
                                                        at[2], 0.0, **kw)

    for k in range(4):
        v = [x, r, p, w]
        v[k] = short
        refused(lp, call(v), "lengths differ|entries", extra)
    refused(lp, call((lo, hi, p, w)), "overlap", extra)
    refused(lp, call((x, r, p, x)), "overlap", extra)
    refused(lp, call(vec=x), "overlap", extra)  # the input vector is x
    refused(lp, call(part=amd.capi.PART_INTERIOR), "interior", extra)
    refused(lp, call(vec_offset=1), "window", extra)
    # everything abft_hip_pcg_iteration_until_dev refuses about dinv and the records
    refused(lp, call(dinv=short), "dinv of %d entries" % (n - 1), extra)
    for k in range(4):
        refused(lp, call(dinv=[x, r, p, w][k]), "dinv overlaps", extra)
    refused(lp, call((lo, r, p, w), dinv=hi), "dinv overlaps", extra)
    for at in ((IN, PW, IN), (IN, PW, IN + 3), (IN, IN + 3, OUT), (IN, PW, PW + 1), (IN, OUT + 3, OUT)):
        refused(lp, call(at=at), "records overlap", extra)
    base = lp.sc.device_ptr
    args = (ctx.h, A.h, p.h, 0, amd.capi.PART_ALL, x.h, r.h, p.h, w.h)
    for ptrs in ((None, base + 32, base + 64), (base, None, base + 64), (base, base + 32, None)):
        refused(lp, lambda: amd.capi.check(ctx.L.abft_hip_pcg_vecc_iteration_until_dev(*args, lp.d.h, *ptrs, 0.0)),
                "null device scalar", extra)
    refused(lp, lambda: amd.capi.check(ctx.L.abft_hip_pcg_vecc_iteration_until_dev(*args, None, base, base + 32, base + 64, 0.0)),
            "null argument", extra)
    lp.until(0.0)  # and the call itself is fine
    assert not np.array_equal(lp.box.words(x), lp.start[0])
    lp.close()


# ------------------------------------------------------------------------------ the solvers --

class Solver:
    """scaled_laplace(32, 32, 6) with b = rhs(1024, 1) on one context: the system whose compared range
    test_vecc_precond_host.py fixed.  Every run starts from x = 0 and a fresh b; dinv is made once (every solve
    scrubs it before returning)."""

    def __init__(self, amd, collect=True):
        self.amd = amd
        cols, rows, vals, n = self.mat = P.scaled_laplace(*SYSTEM)
        self.n, self.b0, self.events = n, rhs(n, 1), []
        self.ctx = ctx = amd.HIPContext("secded", "csr", on_event=(lambda ev, fatal: self.events.extend(ev)) if collect else None)
        self.A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        self.v = dict(zip("bxrpw", (ctx.create_vector(n) for _ in range(5))))
        self.dinv = ctx.jacobi(self.A, protected=True)
        self.v["dinv"] = self.dinv

    def run(self, stride=None, graph=True, precond=True, flip=None, max_itrs=MAX_ITRS):
        """stride None: cg_solve; else cg_solve_device; both with vector_ecc=True.  flip: (vector name, index, bits,
        iteration): planted from the callback of that iteration -- between batches
        -> (itr, rr, history, x as downloaded, events)"""
        ctx, v = self.ctx, self.v
        ctx.upload(v["b"], self.b0)
        ctx.upload(v["x"], np.zeros(self.n))
        hist, self.events = [], []

        def cb(i, rr):
            assert i == len(hist)
            hist.append(rr)
            if flip and i == flip[3]:
                ctx.flip_vector(v[flip[0]], flip[1], flip[2])
        vecs = [v[k] for k in "bxrpw"]
        kw = dict(on_iteration=cb, vector_ecc=True, precond=self.dinv if precond else None)
        if stride is None:
            itr, rr = self.amd.cg_solve(ctx, self.A, *vecs, max_itrs, HISTORY_THRESHOLD, **kw)
        else:
            itr, rr = self.amd.cg_solve_device(ctx, self.A, *vecs, max_itrs, HISTORY_THRESHOLD, stride=stride, graph=graph, **kw)
        return itr, rr, hist, ctx.download(v["x"]), list(self.events)

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def solver(amd):
    s = Solver(amd)
    yield s
    s.close()


@pytest.fixture(scope="module")
def host_solve(solver):
    return solver.run()


def hist_bits(h):
    return np.array(h, dtype=np.float64).view(U)


def history_error(hist, ref):
    return max(abs(a - b) / abs(b) for a, b in zip(hist, ref))


def test_jacobi_protected_is_the_encoded_inverse_diagonal(solver):
    d = solver.ctx.download(solver.dinv).view(U)
    assert solver.dinv.protected is True and solver.dinv.bad == 0
    assert np.array_equal(d, _vecc.encode(P.jacobi(solver.mat)))


def test_host_solve_is_the_model_loop(solver, host_solve):
    itr, rr, hist, x, events = host_solve
    it_m, hist_m = model_run()
    err = history_error(hist, hist_m)
    print("   cg_solve(vector_ecc=True, precond=dinv): %d iterations (model %d), history within %.3g of the model's"
          % (itr, it_m, err))
    assert itr == it_m == len(hist), (itr, it_m)
    assert err <= HISTORY_BAR, err
    assert bits_of(rr) == bits_of(hist[-1]) and rr <= HISTORY_THRESHOLD
    assert not _vecc.decode(x.view(U))[1].any()  # what the caller downloads are codewords
    assert events == []
    # and it solves the system: the true residual of the downloaded x is small against b
    cols, rows, vals, n = solver.mat
    A = np.zeros((n, n))
    A[rows, cols] = vals
    from abft_sparse_cg_amd.context import vecc_strip
    res = solver.b0 - A @ vecc_strip(x)
    assert float(res @ res) <= 1e-4 * float(solver.b0 @ solver.b0)


def test_unpreconditioned_protected_solve_does_what_the_model_says(solver, host_solve):
    it_m, hist_m = model_run(precond=False)
    itr, rr, hist, x, events = solver.run(precond=False)
    converged_m = hist_m[-1] <= HISTORY_THRESHOLD
    print("   without Jacobi: %d iterations, last r.r %.3g (model: %d, %s); with it %d"
          % (itr, rr, it_m, "converged" if converged_m else "not converged", host_solve[0]))
    if converged_m:
        assert itr == it_m
    else:  # non-convergence within max_itrs, as for the model
        assert itr == MAX_ITRS == it_m and not (rr <= HISTORY_THRESHOLD)
    assert itr > host_solve[0] and events == []


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("stride", [1, 3, 16])
def test_device_solve_agrees_with_the_host_solve(solver, host_solve, stride, graph):
    from abft_sparse_cg_amd.context import vecc_strip
    itr, rr, hist, x, events = solver.run(stride, graph)
    itr_h, rr_h, hist_h, x_h, _ = host_solve
    assert itr == itr_h == len(hist), (stride, graph, itr, itr_h)
    err = history_error(hist, hist_h)
    same = np.array_equal(hist_bits(hist), hist_bits(hist_h))
    print("   stride %d graph %s: %d iterations, history %s the host solve's bit for bit (max relative difference %.3g)"
          % (stride, graph, itr, "==" if same else "!=", err))
    assert err <= HISTORY_BAR, (stride, graph, err)
    assert bits_of(rr) == bits_of(hist[-1])
    if same:
        assert np.array_equal(vecc_strip(x).view(U), vecc_strip(x_h).view(U)), (stride, graph)
    assert not _vecc.decode(x.view(U))[1].any()
    assert events == []


FLIP_AT = 9  # the last iteration of the second batch of five: the third batch's replay meets the flip
SOLVER_FLIPS = [("p", 777, [55], [0, 3]), ("x", 801, [62], [1]), ("r", 802, [52], [2]), ("dinv", 513, [50], [5])]


@pytest.mark.parametrize("flip", SOLVER_FLIPS, ids=lambda f: "%s%d" % (f[0], f[2][0]))
def test_device_solve_under_a_flip_is_the_clean_solve(solver, flip):
    from abft_sparse_cg_amd.context import vecc_strip
    name, index, bits, ops = flip
    clean = solver.run(5, True)
    assert clean[4] == [] and clean[0] > FLIP_AT + 5
    hit = solver.run(5, True, flip=(name, index, bits, FLIP_AT))
    assert hit[0] == clean[0] and np.array_equal(hist_bits(hit[2]), hist_bits(clean[2]))
    assert np.array_equal(vecc_strip(hit[3]).view(U), vecc_strip(clean[3]).view(U))
    assert hit[4] == [(CORRECTED, index, bits[0] | op << 8) for op in ops], hit[4]
    assert np.array_equal(solver.ctx.download(solver.dinv).view(U), _vecc.encode(P.jacobi(solver.mat)))


def test_double_flip_in_dinv_is_fatal_at_the_batchs_download(amd, capfd):
    s = Solver(amd, collect=False)  # events are printed and a fatal one raises, as for any caller without a handler
    try:
        seen = []
        with pytest.raises(amd.FatalEvent):
            ctx, v = s.ctx, s.v
            ctx.upload(v["b"], s.b0)
            ctx.upload(v["x"], np.zeros(s.n))

            def cb(i, rr):
                seen.append(i)
                if i == FLIP_AT:
                    ctx.flip_vector(s.dinv, 513, [50, 17])
            amd.cg_solve_device(ctx, s.A, *[v[k] for k in "bxrpw"], MAX_ITRS, HISTORY_THRESHOLD, on_iteration=cb, stride=5,
                                vector_ecc=True, precond=s.dinv)
        assert seen == list(range(FLIP_AT + 1))  # raised before any callback of the batch that met it
        assert "[ECC] double-bit error detected in vector operand 5 at index 513\n" in capfd.readouterr().out
    finally:
        s.close()
