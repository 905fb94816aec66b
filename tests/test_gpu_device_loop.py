"""The device-scalar loop that stops at the threshold: abft_hip_cg_iteration_until_dev (the guarded iteration) and
cg_solve_device on top of it.

The yardstick of a LIVE iteration is abft_hip_cg_iteration_dev, which this feature does not touch (held against an
independent model in test_gpu_devloop.py): the same bits in x, r, p, w and all six scalars.  A FROZEN iteration is
held against its definition: x, r, p keep every bit, the new pair's value has the old pair's bits, its events word
the queued-event count.  cg_solve_device is held against the unguarded loop (bit for bit) and against cg_solve (the
same iteration count, histories within the README's 1e-10 relative)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _oracle import laplace5, rhs
from test_gpu_devloop import SENTINEL, Dev, bits, same_bits, start, tri

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def until(dev, thr, cur=None, nxt=None, pw=None, parity=0, A=None, part=None, vecs=None):
    """one guarded iteration on a Dev; by default on its six scalars with the slots of `parity`; -> the return code"""
    c = dev.capi
    cur = dev.base + 16 * parity if cur is None else cur
    nxt = dev.base + 16 * (1 - parity) if nxt is None else nxt
    pw = dev.base + 32 if pw is None else pw
    x, r, p, w = vecs or (dev.x, dev.r, dev.p, dev.w)
    return dev.L.abft_hip_cg_iteration_until_dev(dev.h, (A or dev.A).h, dev.pfull.h, dev.off,
                                                 c.PART_ALL if part is None else part, x.h, r.h, p.h, w.h, cur, pw, nxt, thr)


def states(dev, state, iters, guarded, thr=0.0):
    """`iters` iterations from `state`, the scalar slots swapping parity -> the downloaded states after each"""
    dev.load(state)
    out = []
    for k in range(iters):
        if guarded:
            dev.capi.check(until(dev, thr, parity=k & 1))
        else:
            dev.launch("one", k & 1)
        out.append(dev.snapshot())
    return out


# ------------------------------------------------------------ 1. live == unguarded --

def live_case(mat, state, monkeypatch, **kw):
    """Five guarded iterations with threshold 0.0 against five unguarded ones, with and without ABFT_HIP_TAIL=0: equal
    bits everywhere after every iteration.  (Threshold 0.0 makes an iteration live while its rr > 0.0; should a
    run reach rr == 0.0 exactly -- n = 1 solves its system in one step -- the guarded iteration behind it is frozen by
    definition where the unguarded one divides 0 by 0, so from there on the frozen contract is what is asserted.)"""
    for tail in (None, "0"):
        if tail:
            monkeypatch.setenv("ABFT_HIP_TAIL", tail)
        else:
            monkeypatch.delenv("ABFT_HIP_TAIL", raising=False)
        ref_dev = Dev(mat, **kw)
        try:
            ref = states(ref_dev, state, 5, False)
            assert not tail or ref_dev.ctx.tail_stats()[0] == 0  # ABFT_HIP_TAIL=0: the three kernels
        finally:
            ref_dev.close()
        dev = Dev(mat, **kw)
        try:
            got = states(dev, state, 5, True)
            assert dev.ctx.tail_stats() == (0, 0, 0, [0, 0, 0, 0])  # left as it was
        finally:
            dev.close()
        monkeypatch.delenv("ABFT_HIP_TAIL", raising=False)
        rr, live = state["rr"], 0
        for k in range(5):
            if not rr > 0.0:
                break
            same_bits(ref[k:k + 1], got[k:k + 1])
            rr = ref[k]["sc"][2 * (1 - (k & 1))]
            live += 1
        print("   n %d tail %s: %d live iterations equal bit for bit" % (mat[3], tail, live))
        assert live >= 1
        for k in range(live, 5):  # frozen behind an rr of exactly 0.0 (or NaN)
            for name in ("x", "r", "pfull"):
                assert np.array_equal(bits(got[k][name]), bits(got[live - 1][name])), (k, name)
            cur, nxt = 2 * (k & 1), 2 * (1 - (k & 1))
            assert bits(got[k]["sc"][nxt:nxt + 1]) == bits(got[k]["sc"][cur:cur + 1])


@pytest.mark.parametrize("n", [1, 2, 255, 257, 2049, 6145])
def test_live_iteration_is_the_unguarded_one(n, monkeypatch):
    live_case(tri(n), start(n), monkeypatch)


@pytest.mark.parametrize("n", [257, 2049])
@pytest.mark.parametrize("align", ["odd", "w_odd"])
def test_live_iteration_on_views_at_an_odd_offset(n, align, monkeypatch):
    """all four operands views one entry into their parents (the entry-by-entry walk), then w alone (the r half walks
    entry by entry, the x / p half by pairs); the parents' edge entries are checked by Dev.close"""
    live_case(tri(n), start(n), monkeypatch, align=align)


# ------------------------------------------------------------------- 2. frozen --

PAYLOAD = np.array([0x7FF8000000ABCDEF, 0xFFF0000000000123, 0x7FF4000000000001], dtype=np.uint64).view(np.float64)


def special_state(n, rr):
    s = start(n)
    for name, at in (("x", 0), ("r", 1 % n), ("p", 2 % n)):
        s[name] = s[name].copy()
        s[name][at::7] = -0.0
        s[name][(at + 3) % n::11] = PAYLOAD[at]
    s["rr"] = rr
    return s


@pytest.mark.parametrize("align", ["aligned", "odd"])
@pytest.mark.parametrize("n", [257, 2049])
@pytest.mark.parametrize("case", ["inf_threshold", "equal", "nan_rr", "nan_payload_rr"])
def test_frozen_iteration_keeps_every_bit(case, n, align):
    rr, thr = {"inf_threshold": (5.0, math.inf), "equal": (0.1 + 0.2, 0.1 + 0.2), "nan_rr": (math.nan, 1.0),
               "nan_payload_rr": (float(PAYLOAD[0]), 0.0)}[case]
    dev = Dev(tri(n), align=align)
    try:
        dev.load(special_state(n, rr))
        if case == "nan_payload_rr":  # (the payload, bit for bit, whatever a float conversion would do to it)
            dev.ctx.upload(dev.sc, np.concatenate([PAYLOAD[:1], np.zeros(5)]))
        pre = dev.snapshot()
        for replay in range(3):
            dev.capi.check(until(dev, thr))
            post = dev.snapshot()
            for name in ("x", "r", "pfull"):
                assert np.array_equal(bits(post[name]), bits(pre[name])), (replay, name)
            assert bits(post["sc"][2:3]) == bits(pre["sc"][0:1]), (post["sc"], pre["sc"])  # the old pair's bits
            assert post["sc"][3] == 0.0                                                     # no event queued
            assert np.array_equal(bits(post["sc"][0:2]), bits(pre["sc"][0:2]))              # what it read: left alone
        assert dev.L.abft_hip_pending_events(dev.h) == 0
        for parent in dev.parents:  # (and again in close)
            a = dev.ctx.download(parent)
            assert (a[0], a[-1]) == (SENTINEL, SENTINEL)
    finally:
        dev.close()


@pytest.mark.parametrize("n", [257, 2049])
def test_infinite_rr_above_a_finite_threshold_is_live(n):
    """(from the loop's ordinary start: with NaNs already in x and p, alpha = inf meets two NaN operands in one
    addition, and which payload survives is the instruction's choice -- seen on an MI355X: the one-launch form of
    abft_hip_cg_iteration_dev and this entry's kernels then keep different payloads; the NaNs this state produces are
    all generated ones)"""
    s = dict(start(n), rr=math.inf)
    ref_dev = Dev(tri(n))
    try:
        ref = states(ref_dev, s, 1, False)
    finally:
        ref_dev.close()
    dev = Dev(tri(n))
    try:
        got = states(dev, s, 1, True, thr=1e300)
    finally:
        dev.close()
    same_bits(ref, got)
    assert not np.array_equal(bits(got[0]["x"]), bits(s["x"]))  # it ran


# --------------------------------------------- 3. the transition inside one graph --

def test_transition_from_live_to_frozen_inside_one_graph():
    """Six guarded iterations captured with threshold rr3 over a trail of seven pairs, the graph starting -- as
    cg_solve_device's does -- with the copy pair 0 <- pair 6 (where rr0 is put first).  One replay: three live
    iterations, three frozen.  A second replay starts from rr3 and changes nothing in x, r, p or the pairs 3..6."""
    n = 2049
    mat, s = tri(n), start(n)
    ref_dev = Dev(mat)
    try:
        ref = states(ref_dev, s, 6, False)
    finally:
        ref_dev.close()
    rrs = [s["rr"]] + [ref[k]["sc"][2 * (1 - (k & 1))] for k in range(6)]
    assert all(a > 0.0 for a in rrs) and rrs[3] < min(rrs[:3])  # live up to rr3, which is new ground
    dev = Dev(mat)
    ctx = dev.ctx
    try:
        dev.load(s)
        trail = ctx.create_vector(16)  # pairs 0..6, then {p.w, events}
        t0 = np.zeros(16)
        t0[12] = rrs[0]
        ctx.upload(trail, t0)
        first, last = ctx.view_vector(trail, 0, 2), ctx.view_vector(trail, 12, 2)
        base = trail.device_ptr
        ctx.graph_begin()
        ctx.copy_vector(first, last)
        for k in range(6):
            dev.capi.check(until(dev, rrs[3], cur=base + 16 * k, nxt=base + 16 * (k + 1), pw=base + 112))
        g = ctx.graph_end()
        ctx.graph_launch(g)
        one = dev.snapshot()
        t = ctx.download(trail)
        for name in ("x", "r", "pfull"):
            assert np.array_equal(bits(one[name]), bits(ref[2][name])), name  # the unguarded state after three
        assert np.array_equal(bits(t[0:14:2]), bits(rrs[:4] + [rrs[3]] * 3)), (t, rrs)
        assert not t[1:14:2].any()
        ctx.graph_launch(g)
        two = dev.snapshot()
        t2 = ctx.download(trail)
        for name in ("x", "r", "pfull"):
            assert np.array_equal(bits(two[name]), bits(one[name])), name
        assert np.array_equal(bits(t2[6:14]), bits(t[6:14]))
        assert np.array_equal(bits(t2[0:14:2]), bits([rrs[3]] * 7))
        ctx.graph_destroy(g)
    finally:
        dev.close()


# --------------------------------------------------------- 4, 5. cg_solve_device --

class Solver:
    """one context and matrix, the five vectors of the loop; every run starts from x = 0"""

    def __init__(self, mat, fmt="csr", mode="none", flip=None, on_event=True):
        import abft_sparse_cg_amd as amd
        from abft_sparse_cg_amd import capi
        self.amd, self.capi, self.events = amd, capi, []
        cols, rows, vals, n = mat
        self.n = n
        self.ctx = ctx = amd.HIPContext(mode, fmt, on_event=(lambda ev, fatal: self.events.extend(ev)) if on_event else None)
        self.A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        if flip:
            ctx.inject_at(self.A, *flip)
        self.b, self.x, self.r, self.p, self.w = (ctx.create_vector(n) for _ in range(5))
        ctx.upload(self.b, rhs(n, 1))
        self.sc = ctx.create_vector(6)

    def vecs(self):
        return self.b, self.x, self.r, self.p, self.w

    def host(self, max_itrs, thr):
        self.ctx.upload(self.x, np.zeros(self.n))
        hist = []
        itr, rr = self.amd.cg_solve(self.ctx, self.A, *self.vecs(), max_itrs, thr, on_iteration=lambda i, v: hist.append(v))
        return itr, rr, hist, self.ctx.download(self.x)

    def device(self, max_itrs, thr, stride, graph, on_iteration=None):
        self.ctx.upload(self.x, np.zeros(self.n))
        hist = []

        def cb(i, v):
            assert i == len(hist)
            hist.append(v)
            if on_iteration:
                on_iteration(i, v)
        itr, rr = self.amd.cg_solve_device(self.ctx, self.A, *self.vecs(), max_itrs, thr, on_iteration=cb, stride=stride,
                                           graph=graph)
        return itr, rr, hist, self.ctx.download(self.x)

    def unguarded(self, itrs):
        """the loop's start, then `itrs` calls of abft_hip_cg_iteration_dev -> (history, x)"""
        ctx, L, c = self.ctx, self.ctx.L, self.capi
        ctx.upload(self.x, np.zeros(self.n))
        ctx.copy_vector(self.r, self.b)
        ctx.copy_vector(self.p, self.r)
        rr0 = ctx.dot(self.r, self.r)
        ctx.upload(self.sc, np.array([rr0, 0, 0, 0, 0, 0.0]))
        base, hist = self.sc.device_ptr, []
        for k in range(itrs):
            cur, nxt = base + 16 * (k & 1), base + 16 * (1 - (k & 1))
            c.check(L.abft_hip_cg_iteration_dev(ctx.h, self.A.h, self.p.h, 0, c.PART_ALL, self.x.h, self.r.h, self.p.h,
                                                self.w.h, cur, base + 32, nxt))
            hist.append(float(ctx.download(self.sc)[2 * (1 - (k & 1))]))
        return hist, ctx.download(self.x)

    def close(self):
        self.ctx.close()


def solve_case(s, thr, strides, limits, want_itr=None):
    """cg_solve_device over every stride, graph setting and max_itrs: one result, the unguarded loop's bit for bit and
    cg_solve's within 1e-10; -> whether it was cg_solve's bit for bit as well"""
    from abft_sparse_cg_amd.context import threshold_ambiguous
    bitwise = True
    for max_itrs in limits:
        itr_h, rr_h, hist_h, x_h = s.host(max_itrs, thr)
        if want_itr is not None:
            assert itr_h == min(want_itr, max_itrs), (itr_h, want_itr, max_itrs)
        assert not any(threshold_ambiguous(v, thr) for v in hist_h)
        hist_u, x_u = s.unguarded(itr_h)
        runs = [s.device(max_itrs, thr, stride, graph) for stride in strides for graph in (True, False)]
        for itr, rr, hist, x in runs:
            assert itr == itr_h == len(hist), (itr, itr_h)
            assert not any(threshold_ambiguous(v, thr) for v in hist)
            assert np.array_equal(bits(hist), bits(hist_u)) and np.array_equal(bits(x), bits(x_u))
            assert bits([rr]) == bits(hist[-1:]) if hist else True
            err = max(abs(a - b) / abs(b) for a, b in zip(hist, hist_h)) if hist else 0.0
            assert err <= 1e-10, err
        same = np.array_equal(bits(runs[0][2]), bits(hist_h)) and np.array_equal(bits(runs[0][3]), bits(x_h))
        print("   thr %g max_itrs %d: %d iterations; device loop %s cg_solve bit for bit" %
              (thr, max_itrs, itr_h, "==" if same else "!="))
        bitwise = bitwise and same
    return bitwise


@pytest.mark.parametrize("nx,ny,thr,want", [(40, 40, 1e-3, 59), (40, 40, 1e-10, 107), (37, 29, 1e-3, 56),
                                            (37, 29, 1e-10, 95)])
def test_cg_solve_device_is_the_unguarded_loop_and_agrees_with_cg_solve(nx, ny, thr, want):
    s = Solver(laplace5(nx, ny))
    try:
        solve_case(s, thr, (1, 5, 16), (1000, 23), want)
        assert s.events == []
    finally:
        s.close()


@pytest.mark.parametrize("spec,fmt,mode,layout", [("powerlaw:2048,3", "coo", "sec7", None),
                                                  ("random:1024,8,1", "csr", "secded", "panels"),
                                                  ("random:1024,8,1", "csr", "secded", "sweep")])
def test_cg_solve_device_on_other_matrices(spec, fmt, mode, layout, monkeypatch):
    from abft_sparse_cg_amd import generators
    if layout:
        monkeypatch.setenv("ABFT_HIP_LAYOUT", layout)
        monkeypatch.setenv("ABFT_HIP_PANEL_WIDTH", "256")
    s = Solver(generators.generate(spec), fmt, mode)
    try:
        if layout:
            assert s.ctx.matrix_info(s.A)[0] == layout
        solve_case(s, 1e-10, (1, 5, 16), (200, 23))
        assert s.events == []
    finally:
        s.close()


# ------------------------------------------------------------------- 6. events --

def test_one_repaired_bit_is_reported_once_as_in_the_host_loop():
    mat = laplace5(40, 40)
    clean = Solver(mat, "csr", "secded")
    try:
        ref = clean.device(1000, 1e-3, 5, True)
        assert clean.events == []
    finally:
        clean.close()
    s = Solver(mat, "csr", "secded", flip=(1000, [37]))
    try:
        itr_h, rr_h, hist_h, x_h = s.host(1000, 1e-3)
        host_events, s.events = s.events, []
        assert len(host_events) == 1
    finally:
        s.close()
    s = Solver(mat, "csr", "secded", flip=(1000, [37]))
    try:
        seen = []
        itr, rr, hist, x = s.device(1000, 1e-3, 5, True, on_iteration=lambda i, v: seen.append(len(s.events)))
        assert s.events == host_events, (s.events, host_events)
        assert seen and all(k == 1 for k in seen)  # drained before the first callback
        assert itr == ref[0] and np.array_equal(bits(hist), bits(ref[2])) and np.array_equal(bits(x), bits(ref[3]))
    finally:
        s.close()


def test_a_fatal_event_is_raised_before_any_callback():
    from abft_sparse_cg_amd import FatalEvent
    s = Solver(laplace5(40, 40), "csr", "sed", flip=(1000, [37]), on_event=False)
    try:
        called = []
        with pytest.raises(FatalEvent):
            s.amd.cg_solve_device(s.ctx, s.A, *s.vecs(), 1000, 1e-3, on_iteration=lambda i, v: called.append(i), stride=5)
        assert called == []
    finally:
        s.close()


# ----------------------------------------------------------- 7. zero iterations --

def test_zero_iterations():
    s = Solver(laplace5(40, 40))
    try:
        ctx = s.ctx
        ctx.upload(s.b, np.zeros(s.n))
        x0 = np.random.default_rng(1).standard_normal(s.n)
        ctx.upload(s.x, x0)
        assert s.amd.cg_solve_device(ctx, s.A, *s.vecs()) == (0, 0.0)
        assert np.array_equal(bits(ctx.download(s.x)), bits(x0))
        ctx.upload(s.b, rhs(s.n, 1))
        called = []
        itr, rr = s.amd.cg_solve_device(ctx, s.A, *s.vecs(), max_itrs=0, on_iteration=lambda i, v: called.append(i))
        assert itr == 0 and rr == ctx.dot(s.b, s.b) and called == []
        assert np.array_equal(bits(ctx.download(s.x)), bits(x0))
    finally:
        s.close()


# -------------------------------------------------------------------- 8. refusals --

def test_refusals_leave_every_vector_untouched():
    n = 257
    mat = tri(n)
    dev = Dev(mat, board="host")
    try:
        dev.load(start(n))
        pre = dev.snapshot()
        assert until(dev, 0.0) != 0  # a board of one rank is a board
        same_bits([pre], [dev.snapshot()])
    finally:
        dev.close()
    dev = Dev(mat)
    ctx = dev.ctx
    try:
        dev.load(start(n))
        pre = dev.snapshot()
        short = ctx.create_vector(n - 1)
        both = ctx.create_vector(2 * n)
        ctx.upload(both, np.arange(2.0 * n))
        xa, rb = ctx.view_vector(both, 0, n), ctx.view_vector(both, n - 1, n)  # one entry shared
        both0 = ctx.download(both)
        b = dev.base
        bad = [dict(cur=0), dict(nxt=0), dict(pw=0), dict(part=dev.capi.PART_INTERIOR), dict(cur=b, nxt=b),
               dict(pw=b + 8), dict(vecs=(short, dev.r, dev.p, dev.w)), dict(vecs=(dev.x, short, dev.p, dev.w)),
               dict(vecs=(dev.x, dev.r, short, dev.w)), dict(vecs=(dev.x, dev.r, dev.p, short)),
               dict(vecs=(xa, rb, dev.p, dev.w)), dict(vecs=(dev.x, dev.r, dev.p, dev.x))]
        for kw in bad:
            assert until(dev, 0.0, **kw) != 0, kw
            with pytest.raises(dev.capi.AbftError):
                dev.capi.check(until(dev, 0.0, **kw))
            same_bits([pre], [dev.snapshot()])
            assert np.array_equal(bits(ctx.download(both)), bits(both0))
        dev.capi.check(until(dev, 0.0))  # and the call itself is fine
        assert not np.array_equal(bits(dev.snapshot()["x"]), bits(pre["x"]))
    finally:
        dev.close()


# ------------------------------------------------------------------------- 9. CLI --

def test_cli_transcript_is_the_host_loops_plus_one_line():
    def go(extra):
        p = subprocess.run([sys.executable, "-m", "abft_sparse_cg_amd.cg", "-t", "hip", "-m", "secded", "-s",
                            "laplace5:40,40", "-c", "1e-8"] + extra, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0, p.stdout + p.stderr
        return re.sub(r"time taken = .*", "time taken = <T> ms", p.stdout)
    host, device = go([]), go(["--device-loop", "8"])
    line = "iteration loop: device scalars, stride 8\n"
    assert device.count(line) == 1 and line not in host
    assert device.index(line) < device.index("iteration     0 :")
    assert device.replace(line, "") == host
    assert "ran for" in host and "iteration" in host
