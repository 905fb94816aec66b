"""The device-scalar loop with Jacobi preconditioning: abft_hip_pcg_iteration_until_dev (the guarded preconditioned
iteration) and cg_solve_device(precond=dinv) on top of it.

The yardstick of a LIVE iteration is the sequence of existing calls it stands for, run on a second context --
abft_hip_spmv_dot_dev and abft_hip_read_pair, alpha = r.z / p.w in numpy float64, abft_hip_calc_xr_precond,
beta = r.z' / r.z, abft_hip_calc_p_precond --: the same bits in x, r, p, w, p.w and both sums.  A FROZEN iteration
is held against its definition: x, r, p keep every bit, the record is handed on with the bits of r.r and r.z, its
events word the queued-event count.  cg_solve_device(precond=) is held against itself over every stride and graph
setting (bit for bit) and against cg_solve(precond=) (the same count, histories within the README's 1e-10)."""
import ctypes as C
import math

import numpy as np
import pytest

from _oracle import laplace5, rhs
from _precond import scaled, scaling
from test_gpu_devloop import SENTINEL, Dev, bits, same_bits, start, tri

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
REC_A, REC_B, PW = 0, 4, 8  # the two records and the pair {p.w, events} in PDev.sc


def tri_scaled(n):
    """tri(n) with rows and columns scaled by powers of two from 2^-6 to 2^6: dinv spans 2^24"""
    return scaled(*tri(n))


class PDev(Dev):
    """Dev with a preconditioner and the scalars of the preconditioned loop: two records {r.r, events, r.z, 0.0} and
    the pair {p.w, events}.  align: Dev's "aligned", "odd" (every operand, dinv too, a view one entry into its
    parent), "w_odd" (w alone), and "dinv_odd" (dinv alone: pairs of r and w, dinv entry by entry)"""

    def __init__(self, mat, align="aligned", ones=False, **kw):
        super().__init__(mat, align="aligned" if align == "dinv_odd" else align, **kw)
        ctx, n = self.ctx, self.n
        d = ctx.jacobi(self.A)
        if ones:
            ctx.upload(d, np.ones(n))
        if align in ("odd", "dinv_odd"):
            parent = ctx.create_vector(n + 2)
            ctx.upload(parent, np.full(n + 2, SENTINEL))
            self.parents.append(parent)
            self.dinv = ctx.view_vector(parent, 1, n)
            ctx.copy_vector(self.dinv, d)
        else:
            self.dinv = d
        self.sc = ctx.create_vector(10)
        self.base = self.sc.device_ptr

    def load(self, s):
        """the vectors of `s`; record A = {rr, 0, rz, 0}, the rest of the scalars filled with 9.0"""
        ctx = self.ctx
        for v, a in ((self.x, s["x"]), (self.r, s["r"]), (self.w, s["w"]), (self.p, s["p"])):
            ctx.upload(v, a)
        sc = np.full(10, 9.0)
        sc[0:4] = (s["rr"], 0.0, s["rz"], 0.0)
        ctx.upload(self.sc, sc)

    def begin(self, s):
        """the loop's start: precond_start on the r of `s` (p = dinv r), its two sums into record A -> (rz, rr)"""
        self.load(dict(s, rz=0.0))
        rz, rr = self.ctx.precond_start(self.r, self.dinv, self.p)
        self.ctx.upload(self.sc, np.array([rr, 0.0, rz, 0.0] + [9.0] * 6))
        return rz, rr

    def snapshot(self):
        s = super().snapshot()
        s["dinv"] = self.ctx.download(self.dinv)
        return s

    def until(self, thr, parity=0, at=None, part=None, vecs=None, dinv=None):
        """one guarded preconditioned iteration; at = (in, pw, out) device addresses -> the return code"""
        c = self.capi
        at = at or (self.base + 32 * parity, self.base + 8 * PW, self.base + 32 * (1 - parity))
        x, r, p, w = vecs or (self.x, self.r, self.p, self.w)
        dinv = dinv or self.dinv
        return self.L.abft_hip_pcg_iteration_until_dev(self.h, self.A.h, self.pfull.h, self.off,
                                                       c.PART_ALL if part is None else part, x.h, r.h, p.h, w.h,
                                                       dinv.h if dinv != "null" else None, at[0], at[1], at[2], thr)

    def host_calls(self, rz):
        """the iteration as existing calls -> (p.w, its events word, rz_new, rr_new)"""
        c, ctx = self.capi, self.ctx
        c.check(self.L.abft_hip_spmv_dot_dev(self.h, self.A.h, self.pfull.h, self.w.h, self.off, self.base + 8 * PW))
        pw, ev, _ = self.read_pair(PW)
        alpha = float(np.float64(rz) / np.float64(pw))
        rz_new, rr_new = ctx.calc_xr_precond(self.x, self.r, self.p, self.w, self.dinv, alpha)
        ctx.calc_p_precond(self.p, self.r, self.dinv, float(np.float64(rz_new) / np.float64(rz)))
        return pw, ev, rz_new, rr_new


VECS = ("x", "r", "pfull", "w", "dinv")


def equal_vectors(a, b, names=VECS):
    for name in names:
        assert np.array_equal(bits(a[name]), bits(b[name])), name


# -------------------------------------------------- 1. live == the host-call sequence --

def live_case(mat, state, iters=5, **kw):
    """`iters` guarded iterations with threshold 0.0 against the host-call sequence on a second context: equal bits
    after every iteration.  (An rr of exactly 0.0 -- n = 1 solves its system in one step -- freezes the guarded
    iteration where the host sequence would divide 0 by 0: from there on the frozen contract is asserted.)"""
    ref_dev = PDev(mat, **kw)
    ref = []
    try:
        rz, rr = ref_dev.begin(state)
        for k in range(iters):
            if not rr > 0.0:
                break
            pw, ev, rz, rr = ref_dev.host_calls(rz)
            ref.append((ref_dev.snapshot(), pw, rz, rr))
    finally:
        ref_dev.close()
    dev = PDev(mat, **kw)
    try:
        rz0, rr0 = dev.begin(state)
        stats = dev.ctx.tail_stats()
        prev = dev.snapshot()
        for k in range(iters):
            cur, nxt = 4 * (k & 1), 4 * (1 - (k & 1))
            dev.capi.check(dev.until(0.0, parity=k & 1))
            v, e, pend = dev.read_pair(nxt)
            got = dev.snapshot()
            sc = got["sc"]
            assert np.array_equal(bits(sc[cur:cur + 4]), bits(prev["sc"][cur:cur + 4]))  # what it read: left alone
            assert bits([v]) == bits(sc[nxt:nxt + 1]) and e == sc[nxt + 1] == pend == 0.0
            assert bits(sc[nxt + 3:nxt + 4]) == bits([0.0])
            if k < len(ref):
                want, pw, rz, rr = ref[k]
                equal_vectors(got, want)
                assert bits(sc[PW:PW + 1]) == bits([pw]), (k, sc[PW], pw)
                assert bits(sc[nxt:nxt + 1]) == bits([rr]) and bits(sc[nxt + 2:nxt + 3]) == bits([rz]), (k, sc, rr, rz)
            else:  # frozen behind an rr of exactly 0.0
                equal_vectors(got, prev, ("x", "r", "pfull", "dinv"))
                assert np.array_equal(bits(sc[[nxt, nxt + 2]]), bits(sc[[cur, cur + 2]]))
            prev = got
        assert dev.ctx.tail_stats() == stats == (0, 0, 0, [0, 0, 0, 0])  # left as it was
        assert dev.L.abft_hip_pending_events(dev.h) == 0
    finally:
        dev.close()
    print("   n %d: %d live iterations equal bit for bit" % (mat[3], len(ref)))
    assert len(ref) >= 1
    return ref


@pytest.mark.parametrize("n", [1, 2, 255, 257, 2049, 6145])
def test_live_iteration_is_the_host_call_sequence(n):
    ref = live_case(tri_scaled(n), start(n))
    d = ref[0][0]["dinv"]
    assert n == 1 or d.max() / d.min() >= 4.0  # far from the identity


@pytest.mark.parametrize("n", [257, 2049])
@pytest.mark.parametrize("align", ["odd", "w_odd", "dinv_odd"])
def test_live_iteration_on_views_at_an_odd_offset(n, align):
    """every operand a view one entry into its parent (<1, false> in both halves); w alone (the r half entry by
    entry, the x / p half by pairs); dinv alone (<2, false>: pairs of the vectors, dinv entry by entry).  The parents'
    edge entries are checked by Dev.close."""
    live_case(tri_scaled(n), start(n), align=align)


# --------------------------------------------------------------- 2. dinv == 1.0 --

@pytest.mark.parametrize("align", ["aligned", "odd"])
@pytest.mark.parametrize("n", [257, 2049])
def test_identity_preconditioner_is_the_plain_guarded_iteration(n, align):
    mat, s = tri(n), start(n)
    plain = Dev(mat, align=align)
    want = []
    try:
        plain.load(s)
        rr0 = plain.ctx.dot(plain.r, plain.r)  # the device's sum, as precond_start forms it (start()'s is numpy's)
        plain.ctx.upload(plain.sc, np.array([rr0, 0.0, 0.0, 0.0, 0.0, 0.0]))
        for k in range(5):
            cur, nxt = plain.base + 16 * (k & 1), plain.base + 16 * (1 - (k & 1))
            plain.capi.check(plain.L.abft_hip_cg_iteration_until_dev(
                plain.h, plain.A.h, plain.pfull.h, 0, plain.capi.PART_ALL, plain.x.h, plain.r.h, plain.p.h, plain.w.h,
                cur, plain.base + 32, nxt, 0.0))
            want.append(plain.snapshot())
    finally:
        plain.close()
    dev = PDev(mat, align=align, ones=True)
    try:
        rz, rr = dev.begin(s)
        assert bits([rz]) == bits([rr]) == bits([rr0])
        for k in range(5):
            nxt = 4 * (1 - (k & 1))
            dev.capi.check(dev.until(0.0, parity=k & 1))
            got = dev.snapshot()
            equal_vectors(got, want[k], ("x", "r", "pfull", "w"))
            assert bits(got["sc"][nxt:nxt + 1]) == bits(want[k]["sc"][2 * (1 - (k & 1)):][:1])
            assert bits(got["sc"][nxt + 2:nxt + 3]) == bits(got["sc"][nxt:nxt + 1])
            assert bits(got["sc"][PW:PW + 1]) == bits(want[k]["sc"][4:5])
    finally:
        dev.close()


# ------------------------------------------------------------------- 3. frozen --

PAYLOAD = np.array([0x7FF8000000ABCDEF, 0xFFF0000000000123, 0x7FF4000000000001], dtype=np.uint64).view(np.float64)


def special_state(n):
    s = start(n)
    for name, at in (("x", 0), ("r", 1 % n), ("p", 2 % n)):
        s[name] = s[name].copy()
        s[name][at::7] = -0.0
        s[name][(at + 3) % n::11] = PAYLOAD[at]
    return s


@pytest.mark.parametrize("align", ["aligned", "odd"])
@pytest.mark.parametrize("n", [257, 2049])
@pytest.mark.parametrize("case", ["inf_threshold", "equal", "nan_rr", "nan_payload_rr"])
def test_frozen_iteration_keeps_every_bit(case, n, align):
    rr, rz, thr = {"inf_threshold": (5.0, 3.0, math.inf), "equal": (0.1 + 0.2, -0.0, 0.1 + 0.2),
                   "nan_rr": (math.nan, 2.5, 1.0), "nan_payload_rr": (PAYLOAD[0], PAYLOAD[1], 0.0)}[case]
    dev = PDev(tri_scaled(n), align=align)
    try:
        dev.load(dict(special_state(n), rr=0.0, rz=0.0))
        sc = np.full(10, 9.0)
        sc[0:4] = (0.0, 0.0, 0.0, 0.0)
        sc[[0, 2]] = np.array([rr, rz], dtype=np.float64)  # (numpy moves the words: a payload stays)
        dev.ctx.upload(dev.sc, sc)
        pre = dev.snapshot()
        assert np.array_equal(bits(pre["sc"][[0, 2]]), bits(np.array([rr, rz])))
        for replay in range(3):
            dev.capi.check(dev.until(thr))
            post = dev.snapshot()
            equal_vectors(post, pre, ("x", "r", "pfull", "dinv"))
            assert np.array_equal(bits(post["sc"][[4, 6]]), bits(pre["sc"][[0, 2]])), (post["sc"], pre["sc"])
            assert np.array_equal(bits(post["sc"][[5, 7]]), bits([0.0, 0.0]))       # no event queued; the fourth word
            assert np.array_equal(bits(post["sc"][0:4]), bits(pre["sc"][0:4]))      # what it read: left alone
            v, e, pend = dev.read_pair(4)
            assert bits([v]) == bits(pre["sc"][0:1]) and e == pend == 0.0
        assert dev.L.abft_hip_pending_events(dev.h) == 0
        for parent in dev.parents:  # (and again in close)
            a = dev.ctx.download(parent)
            assert (a[0], a[-1]) == (SENTINEL, SENTINEL)
    finally:
        dev.close()


@pytest.mark.parametrize("n", [257, 2049])
def test_infinite_rr_above_a_finite_threshold_is_live(n):
    mat, s = tri_scaled(n), start(n)
    ref_dev = PDev(mat)
    try:
        rz, _ = ref_dev.begin(s)
        pw, ev, rz_new, rr_new = ref_dev.host_calls(rz)
        want = ref_dev.snapshot()
    finally:
        ref_dev.close()
    dev = PDev(mat)
    try:
        rz, _ = dev.begin(s)
        pre = dev.snapshot()
        dev.ctx.upload(dev.sc, np.array([math.inf, 0.0, rz, 0.0] + [9.0] * 6))
        dev.capi.check(dev.until(1e300))
        got = dev.snapshot()
    finally:
        dev.close()
    equal_vectors(got, want)
    assert np.array_equal(bits(got["sc"][4:8]), bits([rr_new, 0.0, rz_new, 0.0]))
    assert not np.array_equal(bits(got["x"]), bits(pre["x"]))  # it ran


# --------------------------------------------- 4. the transition inside one graph --

def test_transition_from_live_to_frozen_inside_one_graph():
    """Six guarded iterations captured with threshold rr_L over a trail of seven records, the graph starting -- as
    cg_solve_device's does -- with the copy record 0 <- record 6 (where the start is put first).  r.r is not
    monotone under a preconditioner (on this system it rises for the first iterations), so the graph starts behind
    the first `skip` iterations of the host-call sequence after which some rr_L, 1 <= L <= 5, lies below the L values
    before it.  One replay: L live iterations, 6 - L frozen.  A second replay starts from record L's bits and changes
    nothing in x, r, p or the records L..6."""
    n, horizon = 2049, 40
    mat, s = tri_scaled(n), start(n)
    ref_dev = PDev(mat)
    ref = []
    try:
        rz, rr = ref_dev.begin(s)
        all_recs = [(rr, rz)]
        for k in range(horizon):
            _, _, rz, rr = ref_dev.host_calls(rz)
            all_recs.append((rr, rz))
            ref.append({name: ref_dev.ctx.download(v) for name, v in
                        (("x", ref_dev.x), ("r", ref_dev.r), ("pfull", ref_dev.pfull), ("dinv", ref_dev.dinv))})
    finally:
        ref_dev.close()
    all_rrs = [a for a, _ in all_recs]
    assert all(a > 0.0 for a in all_rrs)
    skip, live = next((j, L) for j in range(horizon - 6) for L in (3, 2, 4, 1, 5)
                      if all_rrs[j + L] < min(all_rrs[j:j + L]))
    recs, rrs, ref = all_recs[skip:skip + 7], all_rrs[skip:skip + 7], ref[skip:skip + 6]
    print("   behind %d iterations: r.r" % skip, rrs, "-> %d live" % live)
    dev = PDev(mat)
    ctx = dev.ctx
    try:
        rz, rr = dev.begin(s)  # (the eager preconditioned call a capture needs)
        for k in range(skip):
            _, _, rz, rr = dev.host_calls(rz)
        assert (rr, rz) == recs[0]
        trail = ctx.create_vector(30)  # records 0..6, then {p.w, events}
        t0 = np.zeros(30)
        t0[24], t0[26] = recs[0]
        ctx.upload(trail, t0)
        first, last = ctx.view_vector(trail, 0, 4), ctx.view_vector(trail, 24, 4)
        base = trail.device_ptr
        ctx.graph_begin()
        ctx.copy_vector(first, last)
        for k in range(6):
            dev.capi.check(dev.until(rrs[live], at=(base + 32 * k, base + 8 * 28, base + 32 * (k + 1))))
        g = ctx.graph_end()
        ctx.graph_launch(g)
        one = dev.snapshot()
        t = ctx.download(trail)
        equal_vectors(one, ref[live - 1], ("x", "r", "pfull", "dinv"))  # the host sequence's state after `live`
        want = recs[:live + 1] + [recs[live]] * (6 - live)
        assert np.array_equal(bits(t[0:28:4]), bits([a for a, _ in want])), (t, recs)
        assert np.array_equal(bits(t[2:28:4]), bits([b for _, b in want])), (t, recs)
        assert not t[1:28:4].any() and not t[3:28:4].any()
        ctx.graph_launch(g)
        two = dev.snapshot()
        t2 = ctx.download(trail)
        equal_vectors(two, one, ("x", "r", "pfull", "dinv"))
        assert np.array_equal(bits(t2[4 * live:28]), bits(t[4 * live:28]))
        assert np.array_equal(bits(t2[0:28:4]), bits([rrs[live]] * 7))
        assert np.array_equal(bits(t2[2:28:4]), bits([recs[live][1]] * 7))
        ctx.graph_destroy(g)
    finally:
        dev.close()


# ------------------------------------------------------------ 5. cg_solve_device --

class Solver:
    """one context, matrix and dinv (taken before anything is flipped), the five vectors of the loop; every run
    starts from x = 0"""

    def __init__(self, mat, fmt="csr", mode="none", flip=None, on_event=True, b=None):
        import abft_sparse_cg_amd as amd
        self.amd, self.events = amd, []
        cols, rows, vals, n = mat
        self.n = n
        self.ctx = ctx = amd.HIPContext(mode, fmt, on_event=(lambda ev, fatal: self.events.extend(ev)) if on_event else None)
        self.A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        self.dinv = ctx.jacobi(self.A)
        if flip:
            ctx.inject_at(self.A, *flip)
        self.b, self.x, self.r, self.p, self.w = (ctx.create_vector(n) for _ in range(5))
        ctx.upload(self.b, rhs(n, 1) if b is None else b)

    def vecs(self):
        return self.b, self.x, self.r, self.p, self.w

    def host(self, max_itrs, thr):
        self.ctx.upload(self.x, np.zeros(self.n))
        hist = []
        itr, rr = self.amd.cg_solve(self.ctx, self.A, *self.vecs(), max_itrs, thr, on_iteration=lambda i, v: hist.append(v),
                                    precond=self.dinv)
        return itr, rr, hist, self.ctx.download(self.x)

    def device(self, max_itrs, thr, stride, graph, on_iteration=None, precond=True):
        self.ctx.upload(self.x, np.zeros(self.n))
        hist = []

        def cb(i, v):
            assert i == len(hist)
            hist.append(v)
            if on_iteration:
                on_iteration(i, v)
        itr, rr = self.amd.cg_solve_device(self.ctx, self.A, *self.vecs(), max_itrs, thr, on_iteration=cb, stride=stride,
                                           graph=graph, precond=self.dinv if precond else None)
        return itr, rr, hist, self.ctx.download(self.x)

    def close(self):
        self.ctx.close()


def solve_case(s, thr, strides, limits):
    """cg_solve_device(precond=) over every stride, graph setting and max_itrs: one result bit for bit, cg_solve(precond=)'s
    count and its history within 1e-10; -> whether it was cg_solve's bit for bit as well"""
    from abft_sparse_cg_amd.context import threshold_ambiguous
    bitwise = True
    for max_itrs in limits:
        itr_h, rr_h, hist_h, x_h = s.host(max_itrs, thr)
        assert not any(threshold_ambiguous(v, thr) for v in hist_h)
        runs = [s.device(max_itrs, thr, stride, graph) for stride in strides for graph in (True, False)]
        for itr, rr, hist, x in runs:
            assert itr == itr_h == len(hist), (itr, itr_h)
            assert np.array_equal(bits(hist), bits(runs[0][2])) and np.array_equal(bits(x), bits(runs[0][3]))
            assert bits([rr]) == bits(hist[-1:]) if hist else True
            err = max(abs(a - b) / abs(b) for a, b in zip(hist, hist_h)) if hist else 0.0
            assert err <= 1e-10, err
        same = np.array_equal(bits(runs[0][2]), bits(hist_h)) and np.array_equal(bits(runs[0][3]), bits(x_h))
        print("   thr %g max_itrs %d: %d iterations; device loop %s cg_solve(precond=) bit for bit" %
              (thr, max_itrs, itr_h, "==" if same else "!="))
        bitwise = bitwise and same
    return bitwise


@pytest.mark.parametrize("nx,ny", [(40, 40), (37, 29)])
@pytest.mark.parametrize("thr", [1e-3, 1e-10])
def test_cg_solve_device_precond_agrees_with_cg_solve_precond(nx, ny, thr):
    s = Solver(scaled(*laplace5(nx, ny)))
    try:
        solve_case(s, thr, (1, 5, 16), (1000, 23))
        assert s.events == []
    finally:
        s.close()


def test_jacobi_makes_the_device_loop_converge_on_the_badly_scaled_system():
    """test_gpu_precond.py's system: the scaled laplace5:40,40 with the reference's right-hand side, threshold 1e-3"""
    from abft_sparse_cg_amd import generators
    mat = scaled(*laplace5(40, 40))
    s = Solver(mat, b=generators.reference_rhs(mat[3], 1))
    try:
        itr_h, rr_h, hist_h, x_h = s.host(1000, 1e-3)
        itr, rr, hist, x = s.device(1000, 1e-3, 16, True)
        print("   PCG: cg_solve %d iterations, cg_solve_device %d" % (itr_h, itr))
        assert itr == itr_h < 1000 and rr <= 1e-3
        itr_p, rr_p, _, _ = s.device(1000, 1e-3, 16, True, precond=False)
        assert itr_p == 1000 and rr_p > 1e-3, (itr_p, rr_p)
    finally:
        s.close()


@pytest.mark.parametrize("spec,fmt,mode,layout", [("powerlaw:2048,3", "coo", "sec7", None),
                                                  ("random:1024,8,1", "csr", "secded", "panels"),
                                                  ("random:1024,8,1", "csr", "secded", "sweep")])
def test_cg_solve_device_precond_on_other_matrices(spec, fmt, mode, layout, monkeypatch):
    from abft_sparse_cg_amd import generators
    if layout:
        monkeypatch.setenv("ABFT_HIP_LAYOUT", layout)
        monkeypatch.setenv("ABFT_HIP_PANEL_WIDTH", "256")
    s = Solver(generators.generate(spec), fmt, mode)
    try:
        if layout:
            assert s.ctx.matrix_info(s.A)[0] == layout
        solve_case(s, 1e-10, (1, 16), (200, 23))
        assert s.events == []
    finally:
        s.close()


# ------------------------------------------------------------------- 6. events --

def test_one_repaired_bit_is_reported_once_as_in_the_host_loop():
    mat = scaled(*laplace5(40, 40))
    clean = Solver(mat, "csr", "secded")
    try:
        ref = clean.device(1000, 1e-3, 5, True)
        assert clean.events == []
    finally:
        clean.close()
    s = Solver(mat, "csr", "secded", flip=(1000, [37]))
    try:
        s.host(1000, 1e-3)
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
    s = Solver(scaled(*laplace5(40, 40)), "csr", "sed", flip=(1000, [37]), on_event=False)
    try:
        called = []
        with pytest.raises(FatalEvent):
            s.amd.cg_solve_device(s.ctx, s.A, *s.vecs(), 1000, 1e-3, on_iteration=lambda i, v: called.append(i), stride=5,
                                  precond=s.dinv)
        assert called == []
    finally:
        s.close()


# -------------------------------------------------------------------- 7. refusals --

def test_refusals_leave_every_vector_and_record_untouched():
    n = 257
    mat = tri_scaled(n)
    dev = PDev(mat)
    ctx = dev.ctx
    try:
        dev.begin(start(n))
        pre = dev.snapshot()
        short = ctx.create_vector(n - 1)
        longer = ctx.create_vector(n + 1)
        both = ctx.create_vector(2 * n)
        ctx.upload(both, 1.0 + np.arange(2.0 * n))
        da, rb = ctx.view_vector(both, 0, n), ctx.view_vector(both, n - 1, n)  # one entry shared
        both0 = ctx.download(both)
        b = dev.base
        ok = (b, b + 64, b + 32)
        bad = [dict(dinv=short), dict(dinv=longer), dict(dinv="null"),
               dict(dinv=da, vecs=(dev.x, rb, dev.p, dev.w)),                  # dinv overlaps r
               dict(dinv=dev.x), dict(dinv=dev.p), dict(dinv=dev.w),
               dict(at=(b, b + 64, b)), dict(at=(b, b + 64, b + 24)),           # the records overlap
               dict(at=(b, b + 24, b + 32)), dict(at=(b, b + 48, b + 32)),      # p.w inside a record
               dict(at=(0, b + 64, b + 32)), dict(at=(b, 0, b + 32)), dict(at=(b, b + 64, 0)),
               dict(part=dev.capi.PART_INTERIOR), dict(vecs=(short, dev.r, dev.p, dev.w)),
               dict(vecs=(dev.x, dev.r, dev.p, dev.x))]
        for kw in bad:
            assert dev.until(0.0, **kw) == ERR_INVALID, kw
            with pytest.raises(dev.capi.AbftError):
                dev.capi.check(dev.until(0.0, **kw))
            same_bits([pre], [dev.snapshot()])
            assert np.array_equal(bits(pre["dinv"]), bits(ctx.download(dev.dinv)))
            assert np.array_equal(bits(ctx.download(both)), bits(both0))
        dev.capi.check(dev.until(0.0, at=ok))  # and the call itself is fine
        assert not np.array_equal(bits(dev.snapshot()["x"]), bits(pre["x"]))
    finally:
        dev.close()


def test_capture_on_a_fresh_context_is_refused_until_one_preconditioned_call_was_made():
    """the reduction's partials are allocated by the first preconditioned call, which a capturing stream cannot do:
    the entry refuses, the capture is ended and its graph destroyed unlaunched; after precond_start the same capture
    works and leaves what the eager call leaves"""
    n = 257
    mat, s = tri_scaled(n), start(n)
    ref_dev = PDev(mat)
    try:
        ref_dev.begin(s)
        ref_dev.capi.check(ref_dev.until(0.0))
        want = ref_dev.snapshot()
    finally:
        ref_dev.close()
    dev = PDev(mat)
    ctx = dev.ctx
    try:
        dev.load(dict(s, rz=0.25))
        pre = dev.snapshot()
        spare, other = ctx.create_vector(4), ctx.create_vector(4)
        ctx.graph_begin()
        ctx.copy_vector(spare, other)  # (a node of its own: the graph is not empty)
        rc = dev.until(0.0)
        msg = (dev.L.abft_hip_last_error() or b"").decode()
        g = ctx.graph_end()
        ctx.graph_destroy(g)
        assert rc == ERR_INVALID and "abft_hip_precond_start" in msg, (rc, msg)
        same_bits([pre], [dev.snapshot()])
        assert dev.begin(s)[1] > 0.0
        ctx.graph_begin()
        dev.capi.check(dev.until(0.0))
        g = ctx.graph_end()
        ctx.graph_launch(g)
        got = dev.snapshot()
        ctx.graph_destroy(g)
        same_bits([want], [got])
    finally:
        dev.close()
