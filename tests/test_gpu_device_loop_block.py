"""The device-resident block loop: abft_hip_cg_block_iteration_until_dev (the guarded block iteration, its column
mask decided on the device) and cg_solve_block_device on top of it.

The yardstick of a LIVE column is the sequence of existing calls the iteration stands for, run on a second context
-- abft_hip_spmm_dot, alpha = r.z / P.W in numpy float64, abft_hip_calc_r_block (abft_hip_calc_r_precond_block),
beta = r.z' / r.z, abft_hip_calc_px_block (abft_hip_calc_px_precond_block), all with the mask the device forms --:
the same bits in X, R, P, W, P.W and both halves of the record.  A FROZEN column is held against its definition:
its column of X, R, P keeps every bit, its record words are handed on.  cg_solve_block_device is held against itself
over every stride and graph setting (bit for bit) and against cg_solve_block(fused=True) (the same counts, histories
within the README's 1e-10)."""
import math

import numpy as np
import pytest

from _oracle import laplace5
from _precond import scaled
from test_gpu_devloop import bits, start, tri
from test_gpu_device_loop_precond import PAYLOAD, tri_scaled

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
MODES = ("none", "secded")
SCALES = np.array([1e-3, 1.0, 30.0, 5.0])


def start_block(n, k):
    """start(n) of test_gpu_devloop.py per column (p = r = b, x with every mantissa bit in use, w full of NaN)"""
    cols = [start(n, 12 + j) for j in range(k)]
    return {name: np.stack([c[name] for c in cols], axis=1) for name in ("x", "r", "p", "w")}


def quot(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


class BDev:
    """one context: a matrix, the block vectors X R P W, dinv (pre), and the scalars: record A at 0, record B at
    2k + 2, {P.W[k], events} at 2 (2k + 2)"""

    def __init__(self, mat, k, mode="none", pre=False, ones=False, fmt="csr", layout="stream", flip=None,
                 on_event=True):
        import abft_sparse_cg_amd as amd
        from abft_sparse_cg_amd import capi
        self.amd, self.capi, self.L, self.events = amd, capi, capi.load(), []
        cols, rows, vals, n = mat
        self.n, self.k, self.rec = n, k, 2 * k + 2
        self.ctx = ctx = amd.HIPContext(mode, fmt, on_event=(lambda ev, fatal: self.events.extend(ev)) if on_event else None)
        self.h = ctx.h
        self.A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout=layout)
        self.dinv = None
        if pre:
            self.dinv = ctx.jacobi(self.A)
            if ones:
                ctx.upload(self.dinv, np.ones(n))
        if flip:
            ctx.inject_at(self.A, *flip)
        self.X, self.R, self.P, self.W = (ctx.create_block(n, k) for _ in range(4))
        self.pw_at = 2 * self.rec
        self.sc = ctx.create_vector(self.pw_at + k + 1)
        self.base = self.sc.device_ptr

    def load(self, s, rr=None, rz=None):
        """the vectors of `s`; record A = {rr, rz, 0, 0}, the rest of the scalars filled with 9.0"""
        ctx, k = self.ctx, self.k
        for v, name in ((self.X, "x"), (self.R, "r"), (self.P, "p"), (self.W, "w")):
            ctx.upload(v, s[name])
        sc = np.full(self.pw_at + k + 1, 9.0)
        if rr is not None:
            sc[0:k] = rr
            sc[k:2 * k] = rr if rz is None else rz
            sc[2 * k:2 * k + 2] = 0.0
        ctx.upload(self.sc, sc)

    def begin(self, s):
        """the loop's start on the r of `s`: its sums into record A -> (rz, rr)"""
        self.load(s)
        k = self.k
        if self.dinv is None:
            rr = self.ctx.dot_block(self.R, self.R, k)
            rz = rr.copy()
        else:
            rz, rr = self.ctx.precond_start_block(self.R, self.dinv, self.P, k, (1 << k) - 1)
        self.load(dict(s, p=self.ctx.download(self.P)), rr, rz)
        return np.array(rz), np.array(rr)

    def snapshot(self):
        ctx = self.ctx
        s = {"x": ctx.download(self.X), "r": ctx.download(self.R), "p": ctx.download(self.P), "w": ctx.download(self.W),
             "sc": ctx.download(self.sc)}
        if self.dinv is not None:
            s["dinv"] = ctx.download(self.dinv)
        return s

    def until(self, thr, parity=0, at=None, vecs=None, dinv="own", k=None, A=None):
        """one guarded block iteration; at = (in, pw, out) device addresses -> the return code"""
        at = at or (self.base + 8 * self.rec * parity, self.base + 8 * self.pw_at, self.base + 8 * self.rec * (1 - parity))
        X, R, P, W = vecs or (self.X, self.R, self.P, self.W)
        d = self.dinv if dinv == "own" else dinv
        h = lambda v: v.h if v is not None else None
        return self.L.abft_hip_cg_block_iteration_until_dev(self.h, h(A or self.A), h(X), h(R), h(P), h(W), h(d),
                                                            self.k if k is None else k, at[0], at[1], at[2], thr)

    def host_calls(self, num, active):
        """the iteration as existing calls with the mask `active` -> (pw[k], rz_new[k], rr_new[k]) of every column"""
        ctx, k = self.ctx, self.k
        on = [(active >> j) & 1 for j in range(k)]
        pw = ctx.spmm_dot(self.A, self.P, self.W, k)
        alpha = [quot(num[j], pw[j]) if on[j] else 0.0 for j in range(k)]
        extra = () if self.dinv is None else (self.dinv,)
        sums = ctx.calc_r_block(self.R, self.W, k, alpha, active, *extra)
        rz_new, rr_new = (sums, sums) if self.dinv is None else sums
        beta = [quot(rz_new[j], num[j]) if on[j] else 0.0 for j in range(k)]
        ctx.calc_px_block(self.X, self.P, self.R, k, alpha, beta, active, *extra)
        return np.array(pw), np.array(rz_new), np.array(rr_new)

    def close(self):
        self.ctx.close()


VECS = ("x", "r", "p", "w")


def equal_vectors(a, b, names=VECS, cols=None):
    for name in names:
        u, v = a[name], b[name]
        if cols is not None and u.ndim == 2:
            u, v = u[:, cols], v[:, cols]
        assert np.array_equal(bits(u), bits(v)), name


def mask_of(rr, thr):
    return sum(1 << j for j in range(len(rr)) if rr[j] > thr)


def reference_run(mat, k, state, iters, thr=0.0, **kw):
    """`iters` iterations of the host-call sequence with the mask rr > thr -> [(snapshot, pw, rz, rr, active)]"""
    ref_dev = BDev(mat, k, **kw)
    ref = []
    try:
        rz, rr = ref_dev.begin(state)
        for _ in range(iters):
            active = mask_of(rr, thr)
            if not active:
                break
            pw, rz_new, rr_new = ref_dev.host_calls(rz, active)
            on = np.array([(active >> j) & 1 for j in range(k)], dtype=bool)
            rz, rr = np.where(on, rz_new, rz), np.where(on, rr_new, rr)  # (no payloads here: values move as they are)
            ref.append((ref_dev.snapshot(), pw, rz.copy(), rr.copy(), active))
        assert ref_dev.events == []
    finally:
        ref_dev.close()
    return ref


# -------------------------------------------------- 1. live == the host-call sequence --

def live_case(mat, k, iters=5, **kw):
    """`iters` guarded iterations with threshold 0.0 against the host-call sequence on a second context: equal bits
    after every iteration.  (An r.r of exactly 0.0 -- n = 1 solves its system in one step -- freezes that column where
    the host sequence would divide 0 by 0: its contract is then the frozen one.)"""
    n = mat[3]
    state = start_block(n, k)
    ref = reference_run(mat, k, state, iters, **kw)
    dev = BDev(mat, k, **kw)
    rec = dev.rec
    try:
        dev.begin(state)
        prev = dev.snapshot()
        for i in range(iters):
            cur, nxt = rec * (i & 1), rec * (1 - (i & 1))
            dev.capi.check(dev.until(0.0, parity=i & 1))
            got = dev.snapshot()
            sc = got["sc"]
            assert np.array_equal(bits(sc[cur:cur + rec]), bits(prev["sc"][cur:cur + rec]))  # what it read: left alone
            assert np.array_equal(bits(sc[nxt + 2 * k:nxt + rec]), bits([0.0, 0.0]))
            assert bits(sc[dev.pw_at + k:])[0] == bits([0.0])[0]
            if i < len(ref):
                want, pw, rz, rr, active = ref[i]
                equal_vectors(got, want)
                assert np.array_equal(bits(sc[dev.pw_at:dev.pw_at + k]), bits(pw)), (i, sc[dev.pw_at:], pw)
                assert np.array_equal(bits(sc[nxt:nxt + k]), bits(rr)), (i, sc[nxt:nxt + k], rr)
                assert np.array_equal(bits(sc[nxt + k:nxt + 2 * k]), bits(rz)), (i, sc, rz)
                if dev.dinv is None:
                    assert np.array_equal(bits(sc[nxt + k:nxt + 2 * k]), bits(sc[nxt:nxt + k]))
            else:  # every column frozen behind an r.r of exactly 0.0
                equal_vectors(got, prev, ("x", "r", "p"))
                assert np.array_equal(bits(sc[nxt:nxt + 2 * k]), bits(sc[cur:cur + 2 * k]))
            prev = got
        assert dev.events == [] and dev.L.abft_hip_pending_events(dev.h) == 0
    finally:
        dev.close()
    print("   n %d k %d: %d live iterations equal bit for bit" % (n, k, len(ref)))
    assert len(ref) >= 1
    return ref


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("n", [1, 2, 255, 257, 2049, 6145])
def test_live_columns_are_the_host_call_sequence(n, k, pre, mode):
    live_case(tri_scaled(n) if pre else tri(n), k, pre=pre, mode=mode)


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("k", [1, 2, 4, 5, 6, 7])
def test_every_k(k, pre):
    live_case(tri_scaled(257) if pre else tri(257), k, pre=pre)


# ------------------------------------------------------------------- 2. every mask --

def special_block(n, k, frozen):
    """start_block with -0.0 and NaN payloads in the frozen columns of x, r and p"""
    s = start_block(n, k)
    for name, at in (("x", 0), ("r", 1), ("p", 2)):
        a = s[name].copy()
        for j in frozen:
            a[(at + j) % n::7, j] = -0.0
            a[(at + j + 3) % n::11, j] = PAYLOAD[(at + j) % 3]
        s[name] = a
    return s


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("mask", range(8))
def test_every_mask(mask, pre, mode):
    """K = 3: the record loaded so that exactly the columns of `mask` exceed the threshold; the frozen columns' records
    hold NaN, a payload NaN and the threshold itself"""
    n, k, thr = 257, 3, 0.1 + 0.2
    mat = tri_scaled(n) if pre else tri(n)
    frozen = [j for j in range(k) if not (mask >> j) & 1]
    state = special_block(n, k, frozen)
    cold_rr = np.array([math.nan, PAYLOAD[0], thr])
    cold_rz = np.array([PAYLOAD[1], PAYLOAD[2], -0.0])

    def records(d):
        rz, rr = d.begin(state)
        live = np.array([(mask >> j) & 1 for j in range(k)], dtype=bool)
        assert all(rr[j] > thr for j in range(k) if live[j])
        rr, rz = np.where(live, rr, cold_rr), np.where(live, rz, cold_rz)  # (numpy moves the words: payloads stay)
        p = d.ctx.download(d.P)
        p[:, frozen] = state["p"][:, frozen]  # (the start rewrote P under a preconditioner)
        d.load(dict(state, p=p), rr, rz)
        return rz, rr

    want = None
    if mask:
        ref_dev = BDev(mat, k, pre=pre, mode=mode)
        try:
            rz, rr = records(ref_dev)
            pw, rz_new, rr_new = ref_dev.host_calls(rz, mask)
            want = (ref_dev.snapshot(), pw, rz_new, rr_new)
        finally:
            ref_dev.close()
    dev = BDev(mat, k, pre=pre, mode=mode)
    rec = dev.rec
    try:
        rz, rr = records(dev)
        pre_s = dev.snapshot()
        assert mask_of(pre_s["sc"][0:k], thr) == mask
        assert np.array_equal(bits(pre_s["sc"][0:2 * k]), bits(np.concatenate([rr, rz])))
        for replay in range(3 if not mask else 1):
            dev.capi.check(dev.until(thr))
            got = dev.snapshot()
            sc = got["sc"]
            assert np.array_equal(bits(sc[0:rec]), bits(pre_s["sc"][0:rec]))        # what it read: left alone
            assert np.array_equal(bits(sc[rec + 2 * k:2 * rec]), bits([0.0, 0.0]))  # no event queued; the last word
            if frozen:  # every bit of the frozen columns, and their record words
                equal_vectors(got, pre_s, ("x", "r", "p"), cols=frozen)
                f = np.array(frozen)
                assert np.array_equal(bits(sc[rec + f]), bits(pre_s["sc"][f]))
                assert np.array_equal(bits(sc[rec + k + f]), bits(pre_s["sc"][k + f]))
            if mask:
                snap, pw, rz_new, rr_new = want
                live = [j for j in range(k) if (mask >> j) & 1]
                equal_vectors(got, snap)  # the host sequence with that `active`: live and frozen columns, and W
                lv = np.array(live)
                assert np.array_equal(bits(sc[dev.pw_at + lv]), bits(pw[lv]))
                assert np.array_equal(bits(sc[rec + lv]), bits(rr_new[lv]))
                assert np.array_equal(bits(sc[rec + k + lv]), bits(rz_new[lv]))
                assert not np.array_equal(bits(got["x"][:, live]), bits(pre_s["x"][:, live]))  # it ran
        assert dev.events == [] and dev.L.abft_hip_pending_events(dev.h) == 0
    finally:
        dev.close()


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "jacobi"])
def test_infinite_rr_above_a_finite_threshold_is_live(pre):
    n, k, thr = 257, 3, 1e300
    mat, state = (tri_scaled(n) if pre else tri(n)), start_block(n, k)

    def records(d):
        rz, rr = d.begin(state)
        rr = rr.copy()
        rr[1] = math.inf
        d.load(dict(state, p=d.ctx.download(d.P)), rr, rz)
        return rz, rr

    ref_dev = BDev(mat, k, pre=pre)
    try:
        rz, rr = records(ref_dev)
        pw, rz_new, rr_new = ref_dev.host_calls(rz, 0b010)
        want = ref_dev.snapshot()
    finally:
        ref_dev.close()
    dev = BDev(mat, k, pre=pre)
    try:
        records(dev)
        pre_s = dev.snapshot()
        dev.capi.check(dev.until(thr))
        got = dev.snapshot()
    finally:
        dev.close()
    equal_vectors(got, want)
    sc, rec = got["sc"], 2 * k + 2
    assert bits(sc[rec + 1:rec + 2]) == bits(rr_new[1:2]) and bits(sc[rec + k + 1:rec + k + 2]) == bits(rz_new[1:2])
    assert np.array_equal(bits(sc[rec + np.array([0, 2])]), bits(pre_s["sc"][np.array([0, 2])]))
    assert not np.array_equal(bits(got["x"][:, 1]), bits(pre_s["x"][:, 1]))  # it ran
    equal_vectors(got, pre_s, ("x", "r", "p"), cols=[0, 2])


# --------------------------------------------------- 3. dinv == 1.0, and K = 1 --

@pytest.mark.parametrize("n", [257, 2049])
def test_identity_preconditioner_gives_the_plain_forms_bits(n):
    k, mat, state = 3, tri(n), start_block(n, 3)
    out = []
    for pre in (False, True):
        dev = BDev(mat, k, pre=pre, ones=True)
        snaps = []
        try:
            rz, rr = dev.begin(state)
            assert np.array_equal(bits(rz), bits(rr))
            for i in range(5):
                dev.capi.check(dev.until(0.0, parity=i & 1))
                snaps.append(dev.snapshot())
        finally:
            dev.close()
        out.append(snaps)
    for a, b in zip(*out):
        equal_vectors(a, b)
        assert np.array_equal(bits(a["sc"]), bits(b["sc"]))
    rec = 2 * k + 2
    last = out[1][-1]["sc"][rec:2 * rec]  # (five iterations: the last record written is B)
    assert np.array_equal(bits(last[0:k]), bits(last[k:2 * k]))


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "jacobi"])
def test_one_column_is_spmm_dot_with_k_1_and_the_block_tail(pre):
    live_case(tri_scaled(2049) if pre else tri(2049), 1, pre=pre)


# --------------------------------------------- 4. the transition inside one graph --

def block_b(n):
    return np.random.default_rng(7).random((n, 4)) * SCALES


def test_columns_stop_at_different_iterations_inside_one_graph():
    """laplace5(40, 40), four right-hand sides of very different size, threshold 1e-3 (a float64 numpy CG: 0, 60, 84
    and 71 iterations; column 0 is frozen from the start).  One batch of 16 guarded iterations captured once and
    replayed to the end; a further replay changes no bit of X, R or P."""
    import abft_sparse_cg_amd as amd
    mat = laplace5(40, 40)
    n, k, thr, stride = mat[3], 4, 1e-3, 16
    B = block_b(n)
    host = BDev(mat, k)
    try:
        vb = host.ctx.create_block(n, k)
        host.ctx.upload(vb, B)
        host.ctx.upload(host.X, np.zeros((n, k)))
        itrs_h, rr_h = amd.cg_solve_block(host.ctx, host.A, vb, host.X, host.R, host.P, host.W, 1000, thr, fused=True)
        x_h = host.ctx.download(host.X)
    finally:
        host.close()
    dev = BDev(mat, k)
    ctx, rec = dev.ctx, dev.rec
    try:
        ctx.upload(dev.X, np.zeros((n, k)))
        ctx.upload(dev.R, B)
        ctx.upload(dev.P, B)
        rr = ctx.dot_block(dev.R, dev.R, k)
        pw_at = rec * (stride + 1)
        trail = ctx.create_vector(pw_at + k + 1)
        t0 = np.zeros(pw_at + k + 1)
        t0[rec * stride:rec * stride + k] = rr
        t0[rec * stride + k:rec * stride + 2 * k] = rr
        ctx.upload(trail, t0)
        first, last = ctx.view_vector(trail, 0, rec), ctx.view_vector(trail, rec * stride, rec)
        base = trail.device_ptr
        ctx.block_loop_reserve(dev.A, k)
        ctx.graph_begin()
        ctx.copy_vector(first, last)
        for i in range(stride):
            dev.capi.check(dev.until(thr, at=(base + 8 * rec * i, base + 8 * pw_at, base + 8 * rec * (i + 1))))
        g = ctx.graph_end()
        itrs, done, launches = [0] * k, False, 0
        while not done:
            ctx.graph_launch(g)
            launches += 1
            t = ctx.download(trail)
            for i in range(stride):
                active = mask_of(t[rec * i:rec * i + k], thr)
                if not active:
                    done = True
                    break
                for j in range(k):
                    itrs[j] += (active >> j) & 1
            assert launches < 100
        print("   per-column counts", itrs, "host", list(itrs_h), "in", launches, "replays")
        assert itrs == list(itrs_h) and len(set(itrs)) >= 3 and itrs[0] == 0
        one = dev.snapshot()
        print("   x %s cg_solve_block(fused=True)'s bit for bit" % ("==" if np.array_equal(bits(one["x"]), bits(x_h)) else "!="))
        assert not one["x"][:, 0].any()  # frozen from the start
        ctx.graph_launch(g)
        two = dev.snapshot()
        equal_vectors(two, one, ("x", "r", "p"))
        ctx.graph_destroy(g)
        assert dev.events == []
    finally:
        dev.close()


# ------------------------------------------------------ 5. cg_solve_block_device --

class Solver:
    """one context, matrix and dinv (taken before anything is flipped), the five block vectors; every run starts from
    X = 0"""

    def __init__(self, mat, B, pre=False, mode="none", flip=None, on_event=True):
        self.d = d = BDev(mat, B.shape[1], mode=mode, pre=pre, flip=flip, on_event=on_event)
        self.amd, self.ctx, self.n, self.k = d.amd, d.ctx, d.n, d.k
        self.B = d.ctx.create_block(d.n, d.k)
        d.ctx.upload(self.B, B)

    @property
    def events(self):
        return self.d.events

    def vecs(self):
        return self.B, self.d.X, self.d.R, self.d.P, self.d.W

    def host(self, max_itrs, thr):
        self.ctx.upload(self.d.X, np.zeros((self.n, self.k)))
        hist = []
        itrs, rr = self.amd.cg_solve_block(self.ctx, self.d.A, *self.vecs(), max_itrs, thr,
                                           on_iteration=lambda i, v, a: hist.append((v, a)), precond=self.d.dinv,
                                           fused=True)
        return list(itrs), rr, hist, self.ctx.download(self.d.X)

    def device(self, max_itrs, thr, stride, graph, on_iteration=None):
        self.ctx.upload(self.d.X, np.zeros((self.n, self.k)))
        hist = []

        def cb(i, v, a):
            assert i == len(hist)
            hist.append((v, a))
            if on_iteration:
                on_iteration(i, v, a)
        itrs, rr = self.amd.cg_solve_block_device(self.ctx, self.d.A, *self.vecs(), max_itrs, thr, on_iteration=cb,
                                                  stride=stride, graph=graph, precond=self.d.dinv)
        return list(itrs), rr, hist, self.ctx.download(self.d.X)

    def close(self):
        self.d.close()


def rrs(hist):
    return np.array([v for v, _ in hist]).reshape(len(hist), -1)


@pytest.mark.parametrize("thr", [1e-3, 1e-10])
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "jacobi"])
def test_cg_solve_block_device_agrees_with_itself_and_the_fused_block_loop(pre, thr):
    from abft_sparse_cg_amd.context import threshold_ambiguous
    mat = scaled(*laplace5(40, 40)) if pre else laplace5(37, 29)
    s = Solver(mat, block_b(mat[3]), pre=pre)
    try:
        for max_itrs in (1000, 23):
            itrs_h, rr_h, hist_h, x_h = s.host(max_itrs, thr)
            assert not any(threshold_ambiguous(v[j], thr) for v, a in hist_h for j in range(s.k) if (a >> j) & 1)
            runs = [s.device(max_itrs, thr, stride, graph) for stride in (1, 5, 16) for graph in (True, False)]
            for itrs, rr, hist, x in runs:
                assert itrs == itrs_h and len(hist) == len(hist_h) == max(itrs_h), (itrs, itrs_h)
                assert [a for _, a in hist] == [a for _, a in hist_h]
                assert np.array_equal(bits(rrs(hist)), bits(rrs(runs[0][2]))) and np.array_equal(bits(x), bits(runs[0][3]))
                assert np.array_equal(bits(rr), bits(runs[0][1]))
                err = float(np.max(np.abs(rrs(hist) - rrs(hist_h)) / np.abs(rrs(hist_h)))) if hist else 0.0
                assert err <= 1e-10, err
            same = np.array_equal(bits(rrs(runs[0][2])), bits(rrs(hist_h))) and np.array_equal(bits(runs[0][3]), bits(x_h))
            print("   thr %g max_itrs %d: counts %s; device loop %s cg_solve_block(fused=True) bit for bit" %
                  (thr, max_itrs, itrs_h, "==" if same else "!="))
        assert s.events == []
    finally:
        s.close()


# ------------------------------------------------------------------- 6. events --

def test_one_repaired_bit_is_reported_once_as_in_the_host_block_loop():
    mat = laplace5(40, 40)
    B = block_b(mat[3])
    clean = Solver(mat, B, mode="secded")
    try:
        ref = clean.device(1000, 1e-3, 5, True)
        assert clean.events == []
    finally:
        clean.close()
    s = Solver(mat, B, mode="secded", flip=(1000, [37]))
    try:
        s.host(1000, 1e-3)
        host_events = list(s.events)
        assert len(host_events) == 1
    finally:
        s.close()
    s = Solver(mat, B, mode="secded", flip=(1000, [37]))
    try:
        seen = []
        itrs, rr, hist, x = s.device(1000, 1e-3, 5, True, on_iteration=lambda i, v, a: seen.append(len(s.events)))
        assert s.events == host_events, (s.events, host_events)
        assert seen and all(c == 1 for c in seen)  # drained before the first callback
        assert itrs == ref[0] and np.array_equal(bits(rrs(hist)), bits(rrs(ref[2]))) and np.array_equal(bits(x), bits(ref[3]))
    finally:
        s.close()


def test_a_fatal_event_is_raised_before_any_callback():
    from abft_sparse_cg_amd import FatalEvent
    mat = laplace5(40, 40)
    s = Solver(mat, block_b(mat[3]), mode="sed", flip=(1000, [37]), on_event=False)
    try:
        called = []
        with pytest.raises(FatalEvent):
            s.amd.cg_solve_block_device(s.ctx, s.d.A, *s.vecs(), 1000, 1e-3, on_iteration=lambda i, v, a: called.append(i),
                                        stride=5)
        assert called == []
    finally:
        s.close()


# -------------------------------------------------------------------- 7. refusals --

def test_refusals_leave_every_vector_and_record_untouched(monkeypatch):
    from abft_sparse_cg_amd import generators
    n, k = 257, 3
    dev = BDev(tri_scaled(n), k, pre=True)
    ctx, rec = dev.ctx, dev.rec
    coo = BDev(tri(n), k, fmt="coo", layout=None)
    monkeypatch.setenv("ABFT_HIP_LAYOUT", "panels")
    monkeypatch.setenv("ABFT_HIP_PANEL_WIDTH", "256")
    rnd = generators.generate("random:1024,8,1")
    pan = BDev(rnd, k, mode="secded", layout=None)
    try:
        dev.begin(start_block(n, k))
        pre = dev.snapshot()
        short, longer = ctx.create_vector(n * k - 1), ctx.create_vector(n * k + k)
        four = ctx.create_block(n, 4)
        dshort = ctx.create_vector(n - 1)
        both = ctx.create_vector(2 * n * k)
        ctx.upload(both, 1.0 + np.arange(2.0 * n * k))
        xa, rb = ctx.view_vector(both, 0, n * k), ctx.view_vector(both, n * k - 1, n * k)  # one entry shared
        both0 = ctx.download(both)
        dx = ctx.view_vector(dev.X, 0, n)  # a dinv inside X
        b = dev.base
        pw = b + 8 * dev.pw_at
        ok = (b, pw, b + 8 * rec)
        X, R, P, W = dev.X, dev.R, dev.P, dev.W
        bad = [dict(vecs=(short, R, P, W)), dict(vecs=(X, longer, P, W)), dict(vecs=(X, R, P, four)),  # lengths
               dict(dinv=dshort),
               dict(k=0), dict(k=9), dict(k=-1), dict(k=2), dict(k=4),
               dict(at=(b, pw, b)), dict(at=(b, pw, b + 8 * (rec - 1))),            # the records overlap
               dict(at=(b, b + 8 * (rec - 1), b + 8 * rec)), dict(at=(b, b + 8 * (rec + 1), b + 8 * rec)),  # P.W inside one
               dict(at=(b, pw - 8 * k, b + 8 * rec)),
               dict(at=(0, pw, b + 8 * rec)), dict(at=(b, 0, b + 8 * rec)), dict(at=(b, pw, 0)),            # null pointers
               dict(vecs=(None, R, P, W)), dict(vecs=(X, R, P, None)), dict(A="null"),
               dict(vecs=(X, R, P, X)), dict(vecs=(X, R, W, W)), dict(vecs=(xa, rb, P, W)),                 # overlaps
               dict(dinv=dx)]                                                                              # dinv in X
        for kw in bad:
            if kw.get("A") == "null":
                rc = dev.L.abft_hip_cg_block_iteration_until_dev(dev.h, None, X.h, R.h, P.h, W.h, dev.dinv.h, k, *ok, 0.0)
            else:
                rc = dev.until(0.0, **kw)
            assert rc == ERR_INVALID, kw
            with pytest.raises(dev.capi.AbftError):
                dev.capi.check(rc)
            post = dev.snapshot()
            equal_vectors(post, pre, ("x", "r", "p", "w", "dinv"))
            assert np.array_equal(bits(post["sc"]), bits(pre["sc"])), kw
            assert np.array_equal(bits(ctx.download(both)), bits(both0))
        # a COO matrix, and a CSR matrix that is not in the streaming layout
        for other in (coo, pan):
            if other is pan:
                assert other.ctx.matrix_info(other.A)[0] == "panels"
            other.load(start_block(other.n, k), np.ones(k))
            before = other.snapshot()
            assert other.until(0.0) == ERR_INVALID
            after = other.snapshot()
            equal_vectors(after, before)
            assert np.array_equal(bits(after["sc"]), bits(before["sc"]))
            assert other.L.abft_hip_block_loop_reserve(other.h, other.A.h, k) == ERR_INVALID
        for kk in (0, 9):
            assert dev.L.abft_hip_block_loop_reserve(dev.h, dev.A.h, kk) == ERR_INVALID
        dev.capi.check(dev.until(0.0, at=ok))  # and the call itself is fine
        assert not np.array_equal(bits(dev.snapshot()["x"]), bits(pre["x"]))
    finally:
        for d in (pan, coo, dev):
            d.close()


# ------------------------------------------------------ 8. capture on a fresh context --

@pytest.mark.parametrize("pre", [False, True], ids=["plain", "jacobi"])
def test_capture_on_a_fresh_context_is_refused_until_the_loop_is_reserved(pre):
    """the partials and the alpha scratch are allocated on first use, which a capturing stream cannot do: the entry
    refuses, the capture is ended and its graph destroyed unlaunched; after block_loop_reserve the same capture works
    and leaves what the eager call leaves"""
    n, k = 257, 3
    mat, s = (tri_scaled(n) if pre else tri(n)), start_block(n, k)
    rr = np.array([float(s["r"][:, j] @ s["r"][:, j]) for j in range(k)])
    ref_dev = BDev(mat, k, pre=pre)
    try:
        ref_dev.load(s, rr, 0.5 * rr)
        ref_dev.capi.check(ref_dev.until(0.0))
        want = ref_dev.snapshot()
    finally:
        ref_dev.close()
    dev = BDev(mat, k, pre=pre)
    ctx = dev.ctx
    try:
        dev.load(s, rr, 0.5 * rr)
        before = dev.snapshot()
        spare, other = ctx.create_vector(4), ctx.create_vector(4)
        ctx.graph_begin()
        ctx.copy_vector(spare, other)  # (a node of its own: the graph is not empty)
        rc = dev.until(0.0)
        msg = (dev.L.abft_hip_last_error() or b"").decode()
        rc2 = dev.L.abft_hip_block_loop_reserve(dev.h, dev.A.h, k)  # eager only
        g = ctx.graph_end()
        ctx.graph_destroy(g)
        assert rc == ERR_INVALID and "abft_hip_block_loop_reserve" in msg, (rc, msg)
        assert rc2 == ERR_INVALID
        after = dev.snapshot()
        equal_vectors(after, before)
        assert np.array_equal(bits(after["sc"]), bits(before["sc"]))
        ctx.block_loop_reserve(dev.A, k)
        ctx.graph_begin()
        dev.capi.check(dev.until(0.0))
        g = ctx.graph_end()
        ctx.graph_launch(g)
        got = dev.snapshot()
        ctx.graph_destroy(g)
        equal_vectors(got, want)
        assert np.array_equal(bits(got["sc"]), bits(want["sc"]))
        assert not np.array_equal(bits(got["x"]), bits(before["x"]))
    finally:
        dev.close()
