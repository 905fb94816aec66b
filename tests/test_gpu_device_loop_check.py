"""Residual checks with rollback in the device-resident loop, on the GPU (abft_hip_residual_check_dev,
abft_hip_residual_check_reserve, cg_solve_device(check_every=)):

    the entry        against abft_hip_residual_gap on the same operands: the SpMV's result and the two sums bit for
                     bit, the verdict at the edges of the rule, what the guard kernel copies where; whole vectors and
                     views at an odd offset, CSR streaming / COO / CSR sweep, capture and replay
    clean runs       a check changes no bit of the rr history or of x; the records are cg_solve(check_every=)'s
    detection        one flipped bit of x or r: the same failed check, rollback, count and history as cg_solve
    a fault that repeats, and Jacobi
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from _oracle import CSR, OracleMatrix, laplace5, rhs
from _precond import scaled

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV = 1e-25  # test_gpu_residual_check.py: laplace5(40, 40) with rhs(n, 1) runs about 170 iterations to it
INF = float("inf")


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def bits_equal(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ 1. the entry --

class Operands:
    """b, x, r, scratch, x_ckpt and a trail of 8 doubles (the slot at 2) on one matrix; align='odd': every vector a
    view at offset 1 of a parent one longer (no operand 16-byte aligned: the VEC = 1 walk, the unaligned copy)"""

    CHK = 2

    def __init__(self, amd, ctx, mat, align="whole", layout=None, seed=3):
        self.amd, self.ctx = amd, ctx
        cols, rows, vals, n = mat
        self.n = n
        self.A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout=layout)
        if align == "whole":
            self.v = {k: ctx.create_vector(n) for k in "bxrwcy"}
        else:
            self.parents = [ctx.create_vector(n + 1) for _ in "bxrwcy"]
            self.v = {k: ctx.view_vector(p, 1, n) for k, p in zip("bxrwcy", self.parents)}
        self.trail = ctx.create_vector(8)
        rng = np.random.default_rng(seed)
        self.h = {k: rng.standard_normal(n) for k in "bxrc"}

    def load(self, **over):
        h = dict(self.h, **over)
        for k in "bxrc":
            self.ctx.upload(self.v[k], h[k])
        self.ctx.upload(self.v["w"], np.full(self.n, 7.0))
        self.ctx.upload(self.trail, np.full(8, -3.0))
        return h

    def gap(self):
        """-> (gap2, tt2, A x) from abft_hip_residual_gap (scratch: the spare vector y)"""
        v = self.v
        g2, t2 = self.ctx.residual_gap(self.A, v["b"], v["x"], v["r"], v["y"])
        return g2, t2, self.ctx.download(v["y"])

    def check(self, limit):
        v = self.v
        self.ctx.residual_check_dev(self.A, v["b"], v["x"], v["r"], v["w"], v["c"], self.trail, self.CHK, limit)

    def state(self):
        d = {k: self.ctx.download(self.v[k]) for k in "bxrwc"}
        d["t"] = self.ctx.download(self.trail)
        return d


def expect(o, h, g2, t2, ys, passed, what):
    """after one check on the operands h: scratch, slot, b and r, and the copy the verdict commands"""
    s = o.state()
    assert bits_equal(s["w"], ys), what
    assert bits_equal(s["t"][2:4], [g2, t2]), (what, s["t"], g2, t2)
    assert s["t"][4] == (1.0 if passed else 2.0) and s["t"][5] == 0.0, (what, s["t"])
    assert bits_equal(s["t"][:2], [-3.0, -3.0]) and bits_equal(s["t"][6:], [-3.0, -3.0]), what
    assert bits_equal(s["b"], h["b"]) and bits_equal(s["r"], h["r"]), what
    if passed:
        assert bits_equal(s["c"], h["x"]) and bits_equal(s["x"], h["x"]), what
    else:
        assert bits_equal(s["x"], h["c"]) and bits_equal(s["c"], h["c"]), what


def entry_cases(amd, ctx, mat, align, layout=None, want=None):
    o = Operands(amd, ctx, mat, align, layout)
    assert want is None or ctx.matrix_info(o.A)[0] == want, ctx.matrix_info(o.A)
    n = o.n
    h = o.load()
    g2, t2, ys = o.gap()
    assert g2 > 0.0 and math.isfinite(g2) and math.isfinite(t2)
    # the edges of the rule: limit equal to gap2 passes, the next double below fails
    o.check(g2)
    expect(o, h, g2, t2, ys, True, "limit == gap2")
    h = o.load()
    o.check(float(np.nextafter(g2, 0.0)))
    expect(o, h, g2, t2, ys, False, "limit just below gap2")
    h = o.load()
    o.check(INF)
    expect(o, h, g2, t2, ys, True, "limit inf, finite sums")
    # r = b - A x exactly: gap2 == 0 passes limit 0
    h = o.load(r=o.h["b"] - ys)
    o.check(0.0)
    s = o.state()
    assert s["t"][2] == 0.0 and s["t"][4] == 1.0 and bits_equal(s["c"], h["x"])
    # a NaN in r: gap2 is NaN, which fails every comparison
    rn = o.h["r"].copy()
    rn[n // 3] = float("nan")
    h = o.load(r=rn)
    gn, tn, _ = o.gap()
    assert gn != gn and math.isfinite(tn)
    o.check(INF)
    expect(o, h, gn, tn, ys, False, "NaN in r")
    # an Inf in b: tt2 is not finite
    bi = o.h["b"].copy()
    bi[n - 1] = INF
    h = o.load(b=bi)
    gi, ti, _ = o.gap()
    assert ti == INF
    o.check(INF)
    expect(o, h, gi, ti, ys, False, "Inf in b")
    # a failed check moves an Inf (and a NaN) of the checkpoint into x as it is
    ci = o.h["c"].copy()
    ci[0], ci[n - 1], ci[n // 2] = INF, -INF, float("nan")
    h = o.load(c=ci)
    o.check(float(np.nextafter(g2, 0.0)))
    expect(o, h, g2, t2, ys, False, "Inf in the checkpoint")
    assert ctx.event_log == [], ctx.event_log[:4]


@pytest.mark.parametrize("fmt", ["csr", "coo"])
@pytest.mark.parametrize("mode", ["none", "secded"])
@pytest.mark.parametrize("align", ["whole", "odd"])
def test_entry_is_residual_gap_with_the_verdict_acted_on(amd, fmt, mode, align):
    for mat in (laplace5(77, 13), laplace5(40, 33)):  # n = 1001 (an odd tail) and 1320
        ctx = amd.HIPContext(mode, fmt)
        try:
            if fmt == "csr":
                entry_cases(amd, ctx, mat, align, "stream", "stream")
            else:
                entry_cases(amd, ctx, mat, align)
        finally:
            ctx.close()


def test_an_inf_in_x_survives_both_copies(amd):
    """a column no row reads: x[j] = Inf leaves A x finite, the check passes and the checkpoint gets the Inf; then a
    failed check brings it back into x"""
    cols, rows, vals, n = laplace5(77, 13)
    j = 500
    keep = cols != j
    mat = (cols[keep], rows[keep], vals[keep], n)
    for align in ("whole", "odd"):
        ctx = amd.HIPContext("none", "csr")
        try:
            o = Operands(amd, ctx, mat, align)
            xi = o.h["x"].copy()
            xi[j] = INF
            h = o.load(x=xi)
            g2, t2, ys = o.gap()
            assert math.isfinite(g2) and math.isfinite(t2)
            o.check(g2)
            expect(o, h, g2, t2, ys, True, "Inf in x, passed")
            assert o.state()["c"][j] == INF
            ci = o.h["c"].copy()
            ci[j] = INF
            h = o.load(c=ci)
            o.check(0.0)
            expect(o, h, g2, t2, ys, False, "Inf in the checkpoint, failed")
            assert o.state()["x"][j] == INF
        finally:
            ctx.close()


def test_capture_needs_the_reserve_call_and_a_replay_is_the_eager_call(amd):
    mat = laplace5(77, 13)
    ctx = amd.HIPContext("secded", "csr")
    try:
        o = Operands(amd, ctx, mat, "whole")
        h = o.load()
        assert o.trail.device_ptr
        ctx.graph_begin()
        try:
            ctx.copy_vector(o.v["y"], o.v["b"])  # (something to capture)
            with pytest.raises(amd.AbftError, match="abft_hip_residual_check_reserve"):
                o.check(1.0)
            with pytest.raises(amd.AbftError, match="capture"):
                ctx.residual_check_reserve()
        finally:
            ctx.graph_destroy(ctx.graph_end())
        s = o.state()
        assert bits_equal(s["w"], np.full(o.n, 7.0)) and bits_equal(s["t"], np.full(8, -3.0))  # nothing was enqueued
        assert bits_equal(s["x"], h["x"]) and bits_equal(s["c"], h["c"])
        ctx.residual_check_reserve()
        ctx.residual_check_reserve()  # idempotent
        ctx.graph_begin()
        try:
            o.check(1.0)
        finally:
            g = ctx.graph_end()
        try:
            g2, t2, ys = o.gap()
            assert g2 > 1.0
            h = o.load()
            ctx.graph_launch(g)
            expect(o, h, g2, t2, ys, False, "replay, failed")
            # the same graph on operands that pass: r = b - A x
            h = o.load(r=o.h["b"] - ys)
            ctx.graph_launch(g)
            s = o.state()
            assert s["t"][2] == 0.0 and s["t"][4] == 1.0 and bits_equal(s["c"], h["x"]) and bits_equal(s["x"], h["x"])
            assert bits_equal(s["t"][3:4], [t2]) and bits_equal(s["w"], ys)
        finally:
            ctx.graph_destroy(g)
    finally:
        ctx.close()


def test_refusals_enqueue_nothing(amd):
    ctx = amd.HIPContext("none", "csr")
    try:
        o = Operands(amd, ctx, laplace5(40, 33), "whole")
        h = o.load()
        v, A, n = o.v, o.A, o.n
        short = ctx.create_vector(n - 1)
        inside = ctx.view_vector(v["x"], 0, n)
        bad = [(v["b"], v["x"], v["r"], v["w"], short),        # the checkpoint's length
               (v["b"], v["x"], v["r"], v["w"], inside),       # the checkpoint overlaps x
               (v["b"], v["x"], v["r"], v["w"], v["b"]),
               (v["b"], v["x"], v["r"], v["x"], v["c"]),       # the scratch overlaps an operand
               (v["b"], short, v["r"], v["w"], v["c"])]        # x's length
        for b, x, r, w, c in bad:
            with pytest.raises(amd.AbftError):
                ctx.residual_check_dev(A, b, x, r, w, c, o.trail, 2, 1.0)
        with pytest.raises(amd.AbftError):                       # the slot inside a vector of the call
            ctx.residual_check_dev(A, v["b"], v["x"], v["r"], v["w"], v["c"], v["r"], 2, 1.0)
        s = o.state()
        assert bits_equal(s["w"], np.full(n, 7.0)) and bits_equal(s["t"], np.full(8, -3.0))
        assert all(bits_equal(s[k], h[k]) for k in "bxrc")
    finally:
        ctx.close()


# the entry and one clean solve in the sweep layout; run in a child so that the layout can be forced
SWEEP = r'''
import sys
sys.path.insert(0, "tests")
import numpy as np
import abft_sparse_cg_amd as amd
from _oracle import laplace5, random_spd, rhs
import test_gpu_device_loop_check as T

for mode in ("none", "secded"):
    for align in ("whole", "odd"):
        ctx = amd.HIPContext(mode, "csr")
        T.entry_cases(amd, ctx, random_spd(3000, 12, 5), align, None, "sweep")
        ctx.close()
s = T.Solver(amd, laplace5(40, 40))
assert s.ctx.matrix_info(s.A)[0] == "sweep", s.ctx.matrix_info(s.A)
T.clean_case(s, 3, 16)
s.close()
print("ok")
'''


def test_entry_and_a_clean_solve_in_the_sweep_layout():
    env = dict(os.environ, ABFT_HIP_LAYOUT="sweep", ABFT_HIP_PANEL_WIDTH="16")
    p = subprocess.run([sys.executable, "-c", SWEEP], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout + p.stderr


# ------------------------------------------------------------------ 2. solves --

class Solver:
    """one context and matrix, the five vectors of the loop and a checkpoint vector; every run starts from x = 0.
    flips: (iteration, 'x' | 'r', index, bits) applied from on_iteration, check_flips: the same from on_check (the
    iteration the check follows); bits may be a callable (downloaded vector, index) -> bits"""

    def __init__(self, amd, mat, mode="none", fmt="csr", jacobi=False):
        self.amd = amd
        cols, rows, vals, n = mat
        self.n = n
        self.ctx = ctx = amd.HIPContext(mode, fmt, on_event=lambda ev, fatal: None)
        self.A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        self.dinv = ctx.jacobi(self.A) if jacobi else None
        self.b, self.x, self.r, self.p, self.w, self.ck = (ctx.create_vector(n) for _ in range(6))
        self.bs = rhs(n, 1)
        ctx.upload(self.b, self.bs)
        self.cache = {}

    def run(self, device, max_itrs=1000, conv=CONV, flips=(), check_flips=(), **kw):
        """-> (itr, history, x, checks); raises what the solve raises"""
        ctx = self.ctx
        ctx.upload(self.x, np.zeros(self.n))
        vecs = {"x": self.x, "r": self.r}
        hist, checks = [], []

        def apply(which, at):
            for fi, name, idx, fb in which:
                if fi == at:
                    ctx.flip_vector(vecs[name], idx, fb(ctx.download(vecs[name]), idx) if callable(fb) else fb)

        def on_it(i, rr):
            hist.append(rr)
            apply(flips, i)

        def on_ck(*c):
            checks.append(c)
            apply(check_flips, c[0])

        if self.dinv is not None:
            kw["precond"] = self.dinv
        if kw.get("check_every"):
            kw["on_check"] = on_ck
        solve = self.amd.cg_solve_device if device else self.amd.cg_solve
        it, _ = solve(ctx, self.A, self.b, self.x, self.r, self.p, self.w, max_itrs, conv, on_iteration=on_it, **kw)
        return it, hist, ctx.download(self.x), checks

    def cached(self, key, **kw):
        if key not in self.cache:
            self.cache[key] = self.run(**kw)
        return self.cache[key]

    def close(self):
        self.ctx.close()


def records(checks):
    return [(c[0], c[2], c[3]) for c in checks]


def clean_case(s, stride, ce):
    """cg_solve_device(check_every=ce) at this stride, graph on and off: the rr history and x of the loop without
    checks bit for bit, no failed check, cg_solve(check_every=ce)'s records"""
    it0, h0, x0, _ = s.cached(("plain", stride), device=True, stride=stride)
    ith, hh, xh, ch = s.cached(("host", ce), device=False, check_every=ce)
    assert ch and all(c[2] for c in ch)
    for graph in (True, False):
        it, h, x, checks = s.run(True, stride=stride, graph=graph, check_every=ce)
        assert it == it0 and bits_equal(h, h0) and bits_equal(x, x0), (stride, ce, graph)
        assert all(c[2] for c in checks) and records(checks) == records(ch), (stride, ce, graph, checks, ch)


@pytest.fixture(scope="module")
def lap(amd):
    s = Solver(amd, laplace5(40, 40))
    yield s
    s.close()


@pytest.mark.parametrize("ce", [5, 16, 50])
@pytest.mark.parametrize("stride", [1, 3, 16])
def test_clean_runs_change_nothing(lap, stride, ce):
    clean_case(lap, stride, ce)


def test_clean_runs_in_mode_secded(amd):
    s = Solver(amd, laplace5(40, 40), mode="secded")
    try:
        s.ctx.inject_at(s.A, 1000, [37])  # corrected by the first SpMV
        clean_case(s, 3, 5)
        clean_case(s, 16, 50)
    finally:
        s.close()


def true_res(o, b, x):
    return float(np.linalg.norm(b - o.spmv(x)))


@pytest.fixture(scope="module")
def oracle():
    cols, rows, vals, n = laplace5(40, 40)
    return OracleMatrix(CSR, "none", cols, rows, vals, n)


def held_against_cg_solve(s, oracle, fails_want, **kw):
    """the same flips in both loops: the same check records, the same total count, rr histories within 1e-10, a final
    true residual within 10 x the clean solve's"""
    _, _, x0, _ = s.cached(("host-plain",), device=False)
    clean = true_res(oracle, s.bs, x0)
    ith, hh, xh, ch = s.run(False, **kw)
    it, h, x, checks = s.run(True, stride=4, **kw)
    assert records(checks) == records(ch), (checks, ch)
    fails = [(c[0], c[3]) for c in checks if not c[2]]
    assert len(fails) == 1 and fails[0][1] == fails_want[0][1], checks
    assert fails_want[0][0] is None or fails == fails_want, checks
    assert it == ith and len(h) == len(hh), (it, ith)
    for a, b in zip(h, hh):
        assert (a != a and b != b) or a == b or abs(a - b) <= 1e-10 * abs(b), (a, b)
    assert checks[-1][2]
    res = true_res(oracle, s.bs, x)
    print("   true residual %.3e (cg_solve %.3e, clean %.3e), %d iterations" % (res, true_res(oracle, s.bs, xh), clean, it))
    assert res <= 10 * clean, (res, clean)


@pytest.mark.parametrize("bit", [62, 55, 52, 45])
def test_detection_is_cg_solves(lap, oracle, bit):
    from abft_sparse_cg_amd.context import _check_batch
    assert _check_batch(10, 1000, 4, 5) == (4, False)  # iterations 10 .. 13: one batch without a check
    i = lap.n // 2 + 7
    for vec in ("x", "r"):
        # (a) from on_iteration at the last iteration of a batch that carries no check
        held_against_cg_solve(lap, oracle, [(14, 9)], check_every=5, flips=[(13, vec, i, [bit])])
        # (b) from on_check: the state behind a batch that carried one
        # (the failed check is the one after iteration 14, or, once r.r is no number, the one on the final state)
        held_against_cg_solve(lap, oracle, [(None, 9)], check_every=5, check_flips=[(9, vec, i, [bit])])


def test_a_residual_that_is_no_number_freezes_the_loop_and_the_final_check_restarts_it(lap, oracle):
    """r[j]'s exponent set to all ones after iteration 3 (stride 4, a check every 16: the next batch carries none): r.r is
    no number from iteration 4 on, the loop freezes, the check on that final state -- enqueued on its own -- fails"""
    def all_ones(v, j):
        e = int(bits(v[j:j + 1])[0] >> np.uint64(52)) & 0x7FF
        return [52 + t for t in range(11) if not (e >> t) & 1]

    j = lap.n // 2 + 7
    ith, hh, xh, ch = lap.run(False, check_every=16, flips=[(3, "r", j, all_ones)])
    fails = [(c[0], c[3]) for c in ch if not c[2]]
    assert len(fails) == 1 and fails[0][0] in (4, 5) and fails[0][1] == -1, ch
    assert not math.isfinite(hh[fails[0][0]])
    held_against_cg_solve(lap, oracle, fails, check_every=16, flips=[(3, "r", j, all_ones)])


def test_a_fault_that_repeats_raises_and_x_is_the_last_checkpoint(lap):
    amd, s = lap.amd, lap
    i = s.n // 2 + 7
    flips = [(k, "r", i, [55]) for k in range(4, 100, 5)]  # from every on_check
    for m in (0, 2):
        s.ctx.upload(s.ck, np.full(s.n, 9.0))
        with pytest.raises(amd.ResidualCheckFailed) as e:
            s.run(True, stride=4, check_every=5, max_rollbacks=m, x_ckpt=s.ck, check_flips=flips)
        recs = records(e.value.checks)
        assert recs == [(4, True, None)] + [(9 + 5 * t, False, 4) for t in range(m + 1)], recs
        assert "after %d rollbacks" % m in str(e.value)
        x, ck = s.ctx.download(s.x), s.ctx.download(s.ck)
        assert bits_equal(x, ck)
        # ... which is x after the five clean iterations the first check saw
        it, _, x5, _ = s.cached(("five",), device=True, max_itrs=5, stride=4)
        assert it == 5 and bits_equal(x, x5)
    # a failure at max_itrs raises as well, x the checkpoint
    with pytest.raises(amd.ResidualCheckFailed, match="max_itrs"):
        s.run(True, max_itrs=12, stride=4, check_every=5, x_ckpt=s.ck, flips=[(10, "x", i, [55])])
    it, _, x10, _ = s.cached(("ten",), device=True, max_itrs=10, stride=4)
    assert bits_equal(s.ctx.download(s.x), x10) and bits_equal(s.ctx.download(s.ck), x10)


def test_jacobi(amd):
    s = Solver(amd, scaled(*laplace5(40, 40)), jacobi=True)
    try:
        conv = 1e-10
        # clean: bit for bit the preconditioned device loop without checks
        for stride, ce in ((4, 5), (16, 50)):
            it0, h0, x0, _ = s.run(True, conv=conv, stride=stride)
            ith, hh, xh, ch = s.run(False, conv=conv, check_every=ce)
            for graph in (True, False):
                it, h, x, checks = s.run(True, conv=conv, stride=stride, graph=graph, check_every=ce)
                assert it == it0 and bits_equal(h, h0) and bits_equal(x, x0), (stride, ce, graph)
                assert all(c[2] for c in checks) and records(checks) == records(ch)
        # one x flip: cg_solve(precond=, check_every=)'s records and count
        i = s.n // 2 + 7
        kw = dict(conv=conv, check_every=5, flips=[(13, "x", i, [55])])
        ith, hh, xh, ch = s.run(False, **kw)
        it, h, x, checks = s.run(True, stride=4, **kw)
        assert records(checks) == records(ch) and it == ith, (checks, ch, it, ith)
        assert [(c[0], c[3]) for c in checks if not c[2]] == [(14, 9)], checks
        err = max(abs(a - b) / abs(b) for a, b in zip(h, hh))
        assert err <= 1e-10, err
    finally:
        s.close()


def test_vector_ecc_with_checks_is_refused_before_anything_runs(lap):
    before = lap.ctx.download(lap.b)
    with pytest.raises(ValueError, match="vector_ecc with check_every"):
        lap.run(True, check_every=5, vector_ecc=True)
    assert bits_equal(lap.ctx.download(lap.b), before)  # not encoded
