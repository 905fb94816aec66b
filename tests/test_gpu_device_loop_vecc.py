"""The device-resident loop on protected vectors: the two-kernel tail abft_hip_calc_r_vecc +
abft_hip_calc_px_vecc, the guarded iteration abft_hip_cg_vecc_iteration_until_dev and
cg_solve_device(vector_ecc=True).

The yardsticks are calls this feature does not touch: the tail is held bit for bit against calc_xr_vecc +
calc_p_vecc (and its words against the numpy model of tests/_devloop_vecc.py), a LIVE guarded iteration against
spmv_vecc + dot_vecc + calc_r_vecc + calc_px_vecc, a FROZEN one against its definition, and the solver against
cg_solve(vector_ecc=True).  Every matrix is CSR in the streaming layout.

Events are (kind, index, bit | operand << 8); the guarded entry counts its vector arguments vec, x, r, p, w as
operands 0..4, the host-scalar entries count their own arguments."""
import math

import numpy as np
import pytest

import _devloop_vecc as M
import _vecc
from _oracle import laplace5, rhs
from test_gpu_vector_ecc import CORRECTED, DOUBLE, Box, bits_of, ragged

pytestmark = pytest.mark.gpu

U = np.uint64
TAIL_LENGTHS = [1, 2, 255, 1025, 4099]  # one and three workgroups; an odd tail in the walk by pairs
ALPHA, BETA = 0.71, 0.125


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def operands(n, seed=0, family=None):
    if family:
        return [_vecc.family(family, n, _vecc.operand_seed(n, k) + seed) for k in range(4)]
    rng = np.random.default_rng(n + seed)
    return [_vecc.encode(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)) for _ in range(4)]


# ------------------------------------------ 1. the two-kernel tail against the two existing calls --

@pytest.mark.parametrize("offset", [0, 1])  # whole vectors (the walk by pairs) or views at offset 1 (entry by entry)
@pytest.mark.parametrize("n", TAIL_LENGTHS)
def test_tail_is_calc_xr_vecc_and_calc_p_vecc_bit_for_bit(amd, n, offset):
    box = Box(amd)
    # (ordinary values, and values with infinities among them; no NaN goes in: which payload an addition of two NaNs
    # keeps is the instruction's choice, and two kernels need not make the same one)
    for family in (None, "inf"):
        xw, rw, pw, ww = operands(n, family=family)

        def same(got, want, what):
            if family:  # Inf - Inf and 0 * Inf make NaNs: _vecc's rule for words (a NaN where the other has one)
                _vecc.assert_words(got, want, what)
            else:
                assert np.array_equal(got, want), what
        for alpha, beta in ((0.37251, -1.3125e-3), (-1.0, 0.0)):
            x0, r0, p0, w0 = (box.vec(a, offset) for a in (xw, rw, pw, ww))
            rr0 = box.ctx.calc_xr_vecc(x0, r0, p0, w0, alpha)
            box.ctx.calc_p_vecc(p0, r0, beta)
            x, r, p, w = (box.vec(a, offset) for a in (xw, rw, pw, ww))
            rr = box.ctx.calc_r_vecc(r, w, alpha)
            same(box.words(r), box.words(r0), (n, family, "r alone"))
            assert np.array_equal(box.words(x), xw) and np.array_equal(box.words(p), pw)  # not touched yet
            assert bits_of(rr) == bits_of(rr0) or (math.isnan(rr) and math.isnan(rr0)), (n, family, rr, rr0)
            box.ctx.calc_px_vecc(x, p, r, alpha, beta)
            for name, got, want in (("x", x, x0), ("r", r, r0), ("p", p, p0), ("w", w, w0)):
                same(box.words(got), box.words(want), (n, family, name))
            assert np.array_equal(box.words(w), ww)
            # and the words of the model
            rs, _ = M.calc_r(rw, ww, alpha)
            xs, ps = M.calc_px(xw, pw, rs, alpha, beta)
            _vecc.assert_words(box.words(r), rs, "r")
            _vecc.assert_words(box.words(x), xs, "x")
            _vecc.assert_words(box.words(p), ps, "p")
    assert box.take() == []
    box.ctx.close()


# ----------------------------------------------------------------------------------- 2. flips --

def flip_sites(n):
    return [0, n // 2, n - 1]


FLIP_BITS = [0, 3, 55]  # the overall parity, a check bit, a data bit


@pytest.mark.parametrize("n", [1025, 4099])
def test_a_flip_in_any_operand_of_the_tail_is_repaired_and_reported_once(amd, n):
    box = Box(amd)
    xw, rw, pw, ww = operands(n)
    x, r, p, w = (box.vec(a) for a in (xw, rw, pw, ww))
    rr0 = box.ctx.calc_r_vecc(r, w, ALPHA)
    r0 = box.words(r)
    box.ctx.calc_px_vecc(x, p, r, ALPHA, BETA)
    x0, p0 = box.words(x), box.words(p)
    assert box.take() == []

    def put(v, words):
        box.ctx.upload(v, words.view(np.float64))

    for at in flip_sites(n):
        for bit in FLIP_BITS:
            for op in range(2):  # calc_r_vecc(r, w): r comes out repaired, w keeps the flip
                put(r, rw), put(w, ww)
                box.ctx.flip_vector((r, w)[op], at, [bit])
                assert bits_of(box.ctx.calc_r_vecc(r, w, ALPHA)) == bits_of(rr0), (at, bit, op)
                assert box.take() == [(CORRECTED, at, bit | op << 8)], (at, bit, op)
                assert np.array_equal(box.words(r), r0)
                assert np.array_equal(box.words(w), M.flipped(ww, at, [bit]) if op else ww)
            for op in range(3):  # calc_px_vecc(x, p, r): x and p come out repaired, r keeps the flip
                put(x, xw), put(p, pw), put(r, r0)
                box.ctx.flip_vector((x, p, r)[op], at, [bit])
                box.ctx.calc_px_vecc(x, p, r, ALPHA, BETA)
                assert box.take() == [(CORRECTED, at, bit | op << 8)], (at, bit, op)
                assert np.array_equal(box.words(x), x0) and np.array_equal(box.words(p), p0), (at, bit, op)
                assert np.array_equal(box.words(r), M.flipped(r0, at, [bit]) if op == 2 else r0)
    box.ctx.close()


def test_two_flipped_bits_in_one_word_are_fatal_as_in_calc_xr_vecc(amd):
    n, at, two = 1025, 600, [52, 17]
    xw, rw, pw, ww = operands(n)
    box = Box(amd)
    x, r, p, w = (box.vec(a) for a in (xw, rw, pw, ww))
    box.ctx.flip_vector(r, at, two)
    box.ctx.calc_xr_vecc(x, r, p, w, ALPHA)
    assert box.fatal
    ref = box.take()
    assert ref == [(DOUBLE, at, 1 << 8)]  # r is calc_xr_vecc's operand 1
    x, r, p, w = (box.vec(a) for a in (xw, rw, pw, ww))
    box.ctx.flip_vector(r, at, two)
    box.ctx.calc_r_vecc(r, w, ALPHA)
    assert box.fatal and box.take() == [(DOUBLE, at, 0 << 8)]  # the same event under this entry's ordinal
    x, r, p, w = (box.vec(a) for a in (xw, rw, pw, ww))
    box.ctx.flip_vector(p, at, two)
    box.ctx.calc_px_vecc(x, p, r, ALPHA, BETA)
    box.ctx.synchronize()
    assert box.take() == [(DOUBLE, at, 1 << 8)]
    box.ctx.close()


# ------------------------------------------------------------------------ 3. the guarded entry --

class Loop:
    """x, r, p, w and six scalars {rr, ev, pw, ev, rr_new, ev} on a Box"""

    def __init__(self, amd, mode, mat, seed=1, fmt="csr", layout="stream"):
        cols, rows, vals, n = mat
        self.n, self.box = n, Box(amd, mode, fmt)
        self.ctx = self.box.ctx
        self.A = self.ctx.create_matrix(cols, rows, vals, n, len(vals), layout=layout)
        rng = np.random.default_rng(seed)
        self.start = [_vecc.encode(rng.standard_normal(n)) for _ in range(3)] + [np.zeros(n, U)]
        self.x, self.r, self.p, self.w = (self.box.vec(a) for a in self.start)
        self.sc = self.ctx.create_vector(6)

    def vecs(self):
        return self.x, self.r, self.p, self.w

    def reset(self, rr):
        for v, a in zip(self.vecs(), self.start):
            self.ctx.upload(v, a.view(np.float64))
        self.ctx.upload(self.sc, np.array([rr, 0, 0, 0, 0, 0.0]))

    def words(self):
        return [self.box.words(v) for v in self.vecs()]

    def scalars(self):
        return self.ctx.download(self.sc).view(U).copy()

    def until(self, thr, **kw):
        self.ctx.cg_vecc_iteration_until_dev(self.A, self.p, self.x, self.r, self.p, self.w, self.sc, 0, 2, 4, thr, **kw)

    def host(self, rr):
        """the four host-scalar calls the live iteration stands for -> (p.w, rr_new)"""
        ctx = self.ctx
        ctx.spmv_vecc(self.A, self.p, self.w)
        pw = ctx.dot_vecc(self.p, self.w)  # served from the fused product
        alpha = M.fdiv(rr, pw)
        rr_new = ctx.calc_r_vecc(self.r, self.w, alpha)
        ctx.calc_px_vecc(self.x, self.p, self.r, alpha, M.fdiv(rr_new, rr))
        return pw, rr_new

    def close(self):
        self.ctx.close()


MATRICES = {"laplace": lambda: laplace5(40, 40), "ragged": ragged}


@pytest.mark.parametrize("mode", ["none", "secded"])
@pytest.mark.parametrize("matrix", sorted(MATRICES))
def test_live_iteration_is_the_four_host_calls_bit_for_bit(amd, mode, matrix):
    mat = MATRICES[matrix]()
    if matrix == "ragged":
        assert np.bincount(mat[1], minlength=mat[3]).max() >= 1025  # a row longer than a tile
    lp = Loop(amd, mode, mat)
    rr = 3.25
    lp.reset(rr)
    pw, rr_new = lp.host(rr)
    want = lp.words()
    assert lp.box.take() == []
    lp.reset(rr)
    lp.until(0.0)
    got, sc = lp.words(), lp.scalars()
    for name, g, w in zip("xrpw", got, want):
        assert np.array_equal(g, w), (matrix, mode, name)
    assert sc[2] == bits_of(pw) and sc[4] == bits_of(rr_new), (sc, pw, rr_new)
    assert sc[0] == bits_of(rr) and sc[1] == 0 and sc[3] == 0 and sc[5] == 0  # the events words: nothing queued
    assert lp.box.take() == []
    assert lp.ctx.tail_stats() == (0, 0, 0, [0, 0, 0, 0])  # left alone
    # the words of the model, fed with the device's two sums
    m = M.iteration(_vecc.csr_of(*mat), *lp.start[:3], rr, 0.0, p_dot_w=pw, rr_new=rr_new)
    for name, g in zip("xrpw", got):
        _vecc.assert_words(g, m[name], name)
    # a second iteration from there, the scalars read where the first left them
    lp.ctx.upload(lp.sc, np.array([rr_new, 0, 0, 0, 0, 0.0]))
    lp.until(0.0)
    got2, sc2 = lp.words(), lp.scalars()
    for v, a in zip(lp.vecs(), want):
        lp.ctx.upload(v, a.view(np.float64))
    pw2, rr2 = lp.host(rr_new)
    for name, g, w in zip("xrpw", got2, lp.words()):
        assert np.array_equal(g, w), (matrix, mode, name, "second")
    assert sc2[2] == bits_of(pw2) and sc2[4] == bits_of(rr2)
    lp.close()


def test_live_iteration_reports_flips_under_the_entrys_ordinals(amd):
    lp = Loop(amd, "secded", laplace5(40, 40))
    rr, at = 3.25, 20 * 40 + 20
    lp.reset(rr)
    lp.until(0.0)
    want, sc0 = lp.words(), lp.scalars()
    assert lp.box.take() == []
    for name, bit, ops in (("p", 55, [0, 3]), ("p", 0, [0, 3]), ("x", 3, [1]), ("r", 62, [2])):
        lp.reset(rr)
        lp.ctx.flip_vector(dict(x=lp.x, r=lp.r, p=lp.p)[name], at, [bit])
        lp.until(0.0)
        got, sc = lp.words(), lp.scalars()
        for k, g, w in zip("xrpw", got, want):
            assert np.array_equal(g, w), (name, bit, k)  # x, r and p rewritten: the clean iteration's words
        assert sc[2] == sc0[2] and sc[4] == sc0[4]
        # the SpMV's report is queued before its fold, the r half's before its finish
        queued = {"p": (1.0, 1.0), "x": (0.0, 0.0), "r": (0.0, 1.0)}[name]
        assert (sc[3:4].view(np.float64)[0], sc[5:6].view(np.float64)[0]) == queued, (name, sc)
        assert lp.box.take() == [(CORRECTED, at, bit | op << 8) for op in ops], (name, bit)
    lp.close()


PAYLOAD = np.array([0x7FF8000000ABCDEF], U).view(np.float64)


@pytest.mark.parametrize("case", ["equal", "above", "nan_payload"])
def test_frozen_iteration_keeps_every_word_and_hands_the_pair_on(amd, case):
    rr, thr = {"equal": (0.1 + 0.2, 0.1 + 0.2), "above": (5.0, math.inf), "nan_payload": (float(PAYLOAD[0]), 0.0)}[case]
    lp = Loop(amd, "secded", laplace5(40, 40))
    at = 20 * 40 + 20
    lp.reset(rr)
    lp.ctx.upload(lp.sc, np.concatenate([PAYLOAD if case == "nan_payload" else [rr], [0, 7.0, 7.0, 7.0, 7.0]]))
    for v, bit in ((lp.x, 12), (lp.r, 0), (lp.p, 55)):  # one flipped word in each: a frozen launch repairs nothing
        lp.ctx.flip_vector(v, at, [bit])
    pre, pre_sc = lp.words(), lp.scalars()
    assert not np.array_equal(pre[0], lp.start[0])
    lp.until(thr)
    post, sc = lp.words(), lp.scalars()
    for name, a, b in zip("xrp", post, pre):
        assert np.array_equal(a, b), (case, name)
    assert sc[4] == pre_sc[0] and np.array_equal(sc[0:2], pre_sc[0:2])  # the pair's bits moved on, what was read left alone
    # the SpMV ran: its gather met the flip in p and reported it (operand 0), and that is all that is reported
    assert sc[5:6].view(np.float64)[0] == 1.0
    assert lp.box.take() == [(CORRECTED, at, 55)]
    # captured and replayed three times: nothing changes
    lp.ctx.graph_begin()
    try:
        lp.until(thr)
    finally:
        g = lp.ctx.graph_end()
    for replay in range(3):
        lp.ctx.graph_launch(g)
        post, sc = lp.words(), lp.scalars()  # (the download drains: every replay's gather reports the flip in p again)
        for name, a, b in zip("xrp", post, pre):
            assert np.array_equal(a, b), (case, replay, name)
        assert sc[4] == pre_sc[0] and np.array_equal(sc[0:2], pre_sc[0:2])
        assert lp.box.take() == [(CORRECTED, at, 55)], replay
    lp.ctx.graph_destroy(g)
    lp.close()


def test_guarded_entry_captures_on_a_fresh_context(amd):
    """nothing the call needs is allocated on first use: a context whose first call it is can capture it"""
    lp = Loop(amd, "none", laplace5(40, 40))
    rr = 3.25
    lp.reset(rr)
    lp.until(0.0)
    want, sc0 = lp.words(), lp.scalars()
    lp.close()
    lp = Loop(amd, "none", laplace5(40, 40))
    lp.reset(rr)
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


def test_refusals_leave_every_vector_and_pair_untouched(amd, monkeypatch):
    mat = laplace5(40, 40)

    def refused(lp, call, text, extra=()):
        pre, pre_sc = lp.words() + [lp.box.words(v) for v in extra], lp.scalars()
        with pytest.raises(amd.AbftError, match=text):
            call()
        post = lp.words() + [lp.box.words(v) for v in extra]
        assert all(np.array_equal(a, b) for a, b in zip(post, pre)) and np.array_equal(lp.scalars(), pre_sc), text
        assert lp.box.take() == []

    lp = Loop(amd, "secded", mat, fmt="coo", layout=None)
    lp.reset(3.25)
    refused(lp, lambda: lp.until(0.0), "cg_vecc_iteration_until: .*COO")
    lp.close()
    for layout, name in (("panels", "panel"), ("sweep", "sweep")):
        monkeypatch.setenv("ABFT_HIP_LAYOUT", layout)
        lp = Loop(amd, "secded", mat, layout=None)
        assert lp.ctx.matrix_info(lp.A)[0] == layout
        lp.reset(3.25)
        refused(lp, lambda: lp.until(0.0), "cg_vecc_iteration_until: .*" + name)
        lp.close()
    monkeypatch.delenv("ABFT_HIP_LAYOUT")

    lp = Loop(amd, "secded", mat)
    lp.reset(3.25)
    ctx, n, A = lp.ctx, lp.n, lp.A
    marks = _vecc.encode(np.arange(1.0, n + 1.0))
    short = lp.box.vec(marks[:-1])
    both = lp.box.vec(np.concatenate([marks, marks]))
    lo, hi = ctx.view_vector(both, 0, n), ctx.view_vector(both, n - 1, n)  # one entry shared
    extra = [short, both]
    x, r, p, w = lp.vecs()

    def call(vecs=None, at=(0, 2, 4), vec=None, **kw):
        vx, vr, vp, vw = vecs or (x, r, p, w)
        return lambda: ctx.cg_vecc_iteration_until_dev(A, vec or vp, vx, vr, vp, vw, lp.sc, at[0], at[1], at[2], 0.0, **kw)

    # everything abft_hip_cg_iteration_until_dev refuses
    for k in range(4):
        v = [x, r, p, w]
        v[k] = short
        refused(lp, call(v), "lengths differ|entries", extra)
    refused(lp, call((lo, hi, p, w)), "overlap", extra)
    refused(lp, call((x, r, p, x)), "overlap", extra)
    refused(lp, call(vec=x), "overlap", extra)  # the input vector is x
    refused(lp, call(at=(0, 2, 0)), "pairs overlap", extra)
    refused(lp, call(at=(0, 1, 4)), "pairs overlap", extra)
    refused(lp, call(part=amd.capi.PART_INTERIOR), "interior", extra)
    refused(lp, call(vec_offset=1), "window", extra)
    base = lp.sc.device_ptr
    for ptrs in ((None, base + 16, base + 32), (base, None, base + 32), (base, base + 16, None)):
        refused(lp, lambda: amd.capi.check(ctx.L.abft_hip_cg_vecc_iteration_until_dev(
            ctx.h, A.h, p.h, 0, amd.capi.PART_ALL, x.h, r.h, p.h, w.h, *ptrs, 0.0)), "null device scalar", extra)
    # the host-scalar entries: lengths and overlaps
    refused(lp, lambda: ctx.calc_r_vecc(r, short, 0.5), "calc_r_vecc: lengths differ", extra)
    refused(lp, lambda: ctx.calc_r_vecc(short, w, 0.5), "calc_r_vecc: lengths differ", extra)
    refused(lp, lambda: ctx.calc_r_vecc(lo, hi, 0.5), "calc_r_vecc: .*overlap", extra)
    for k in range(3):
        v = [x, p, r]
        v[k] = short
        refused(lp, lambda: ctx.calc_px_vecc(*v, 0.5, 0.5), "calc_px_vecc: lengths differ", extra)
    for v in ((lo, hi, r), (lo, p, hi), (x, lo, hi)):
        refused(lp, lambda: ctx.calc_px_vecc(*v, 0.5, 0.5), "calc_px_vecc: .*overlap", extra)
    lp.until(0.0)  # and the call itself is fine
    assert not np.array_equal(lp.box.words(x), lp.start[0])
    lp.close()


# ------------------------------------------------------------------------------ 4. the solver --

class Solver:
    """laplace5:40,40 with the reference's b on one context; every run starts from x = 0 and a fresh b"""

    def __init__(self, amd, collect=True):
        self.amd = amd
        cols, rows, vals, n = laplace5(40, 40)
        self.n, self.b0, self.events = n, rhs(n, 1), []
        self.ctx = ctx = amd.HIPContext("secded", "csr", on_event=(lambda ev, fatal: self.events.extend(ev)) if collect else None)
        self.A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        self.v = dict(zip("bxrpw", (ctx.create_vector(n) for _ in range(5))))

    def run(self, thr, stride=None, graph=True, ecc=True, flip=None, max_itrs=1000):
        """stride None: cg_solve(vector_ecc=True); else cg_solve_device.  flip: (vector name, index, bits, iteration): planted
        from the callback of that iteration -- between batches -> (itr, rr, history, x as downloaded, events)"""
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
        if stride is None:
            itr, rr = self.amd.cg_solve(ctx, self.A, *vecs, max_itrs, thr, on_iteration=cb, vector_ecc=True)
        else:
            itr, rr = self.amd.cg_solve_device(ctx, self.A, *vecs, max_itrs, thr, on_iteration=cb, stride=stride,
                                               graph=graph, **({"vector_ecc": True} if ecc else {}))
        return itr, rr, hist, ctx.download(v["x"]), list(self.events)

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def solver(amd):
    s = Solver(amd)
    yield s
    s.close()


@pytest.fixture(scope="module")
def host_solves(solver):
    return {thr: solver.run(thr) for thr in (1e-3, 1e-10)}


def hist_bits(h):
    return np.array(h, dtype=np.float64).view(U)


def against_host(got, ref, what):
    from abft_sparse_cg_amd.context import vecc_strip
    itr, rr, hist, x, events = got
    itr_h, rr_h, hist_h, x_h, _ = ref
    assert itr == itr_h == len(hist), (what, itr, itr_h)
    err = max(abs(a - b) / abs(b) for a, b in zip(hist, hist_h))
    same = np.array_equal(hist_bits(hist), hist_bits(hist_h))
    print("   %s: %d iterations, history %s cg_solve(vector_ecc=True)'s bit for bit (max relative difference %.3g)"
          % (what, itr, "==" if same else "!=", err))
    assert err <= 1e-10, (what, err)
    assert bits_of(rr) == bits_of(hist[-1])
    if same:
        assert np.array_equal(vecc_strip(x).view(U), vecc_strip(x_h).view(U)), what
    assert not _vecc.decode(x.view(U))[1].any()  # what the caller downloads are codewords
    assert events == []
    return same


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("stride", [1, 3, 16])
@pytest.mark.parametrize("thr", [1e-3, 1e-10])
def test_protected_device_solve_agrees_with_the_protected_host_solve(solver, host_solves, thr, stride, graph):
    against_host(solver.run(thr, stride, graph), host_solves[thr], "thr %g stride %d graph %s" % (thr, stride, graph))


def test_protected_device_solve_that_stops_on_a_batchs_last_iteration(solver, host_solves):
    ref = host_solves[1e-3]
    itr_h = ref[0]
    assert itr_h > 1
    for graph in (True, False):  # one batch of exactly itr_h iterations, then a batch of frozen ones
        against_host(solver.run(1e-3, itr_h, graph), ref, "stride = the iteration count, graph %s" % graph)
    # and with max_itrs the iteration count: no look beyond it
    got = solver.run(1e-3, itr_h, True, max_itrs=itr_h)
    assert got[0] == itr_h and np.array_equal(hist_bits(got[2]), hist_bits(solver.run(1e-3, itr_h, True)[2]))


FLIP_AT = 9  # the last iteration of the second batch of five: the third batch's replay meets the flip
SOLVER_FLIPS = [("p", 777, [55], [0, 3]), ("x", 801, [62], [1]), ("r", 802, [52], [2])]


@pytest.mark.parametrize("flip", SOLVER_FLIPS, ids=lambda f: "%s%d" % (f[0], f[2][0]))
def test_protected_device_solve_under_a_flip_is_the_clean_solve(solver, flip):
    name, index, bits, ops = flip
    clean = solver.run(1e-10, 5, True)
    assert clean[4] == [] and clean[0] > FLIP_AT + 5
    hit = solver.run(1e-10, 5, True, flip=(name, index, bits, FLIP_AT))
    assert hit[0] == clean[0] and np.array_equal(hist_bits(hit[2]), hist_bits(clean[2]))
    assert np.array_equal(hit[3].view(U), clean[3].view(U))
    assert hit[4] == [(CORRECTED, index, bits[0] | op << 8) for op in ops], hit[4]
    # the same flip in the unprotected device loop changes the run: the test can see a flip
    plain = solver.run(1e-10, 5, True, ecc=False)
    plain_hit = solver.run(1e-10, 5, True, ecc=False, flip=(name, index, bits, FLIP_AT))
    assert plain_hit[4] == []
    assert not (plain_hit[0] == plain[0] and np.array_equal(hist_bits(plain_hit[2]), hist_bits(plain[2])) and
                np.array_equal(plain_hit[3].view(U), plain[3].view(U)))


def test_double_flip_in_r_is_fatal_at_the_batchs_download(amd, capfd):
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
                    ctx.flip_vector(v["r"], 802, [52, 17])
            amd.cg_solve_device(ctx, s.A, *[v[k] for k in "bxrpw"], 1000, 1e-10, on_iteration=cb, stride=5, vector_ecc=True)
        assert seen == list(range(FLIP_AT + 1))  # raised before any callback of the batch that met it
        assert "[ECC] double-bit error detected in vector operand 2 at index 802\n" in capfd.readouterr().out
    finally:
        s.close()
