"""The fused block iteration on the GPU: abft_hip_spmm_dot against abft_hip_spmm,
abft_hip_calc_r_block / abft_hip_calc_px_block (and their Jacobi forms) against the calls they stand in
for, the refusals, cg_solve_block(fused=True) against fused=False, and the CLI's --block-fused.

    spmm_dot       W bit-identical to spmm's; every sum within 1e-13 of the sum of the terms' magnitudes
                   of the serial sum (the bar of test_gpu_vector_ecc.close for a tree sum against a
                   serial one); two calls give the same bits; power-of-two columns scale exactly
    events         one spmm_dot queues what one spmm queues; a repaired element changes no bit
    vector calls   R, X, P and the sums bit for bit those of calc_xr_block + calc_p_block
    refusals       every vector's words unchanged
    solves         per column the iteration count of the unfused loop, true residual within 10 x
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _oracle import MODES, laplace5, ora_dot, rhs
from _precond import matvec, scaled
from test_gpu_packed_csr import long_row, three_values_wide_span, wide_row
from test_gpu_vector_ecc import ragged

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = np.uint64
KS = (1, 2, 3, 4, 5, 8)


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(U), np.asarray(b, dtype=np.float64).view(U))


class Box:
    """a context that collects its events; the matrix in the streaming layout"""

    def __init__(self, amd, mode, mat=None, fmt="csr"):
        self.events, self.fatal = [], False
        self.ctx = amd.HIPContext(mode, fmt, on_event=self._on)
        if mat is not None:
            cols, rows, vals, n = mat
            self.n = n
            self.A = self.ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")

    def _on(self, ev, fatal):
        self.events += ev
        self.fatal |= fatal

    def take(self):
        self.ctx._drain()
        ev, f = self.events, self.fatal
        self.events, self.fatal = [], False
        return ev, f

    def block(self, array, offset=0):
        """a block vector holding `array` (n, k); offset > 0: a view at that offset of a longer vector"""
        n, k = array.shape
        if offset:
            v = self.ctx.view_vector(self.ctx.create_vector(n * k + offset + 2), offset, n * k)
            v.K = k
        else:
            v = self.ctx.create_block(n, k)
        self.ctx.upload(v, array)
        return v

    def vec(self, array, offset=0):
        v = self.ctx.create_vector(len(array) + offset)
        if offset:
            v = self.ctx.view_vector(v, offset, len(array))
        self.ctx.upload(v, array)
        return v

    def words(self, v):
        return self.ctx.download(v).reshape(-1).view(U).copy()


def block_x(n, k, seed=10):
    return np.stack([rhs(n, seed + j) - 0.5 for j in range(k)], axis=1)


MATS = {
    "lap": lambda: laplace5(40, 40),
    "ragged": ragged,
    "three": three_values_wide_span,
    "wide": wide_row,
    "long": long_row,
}
SPMM_CASES = [("lap", m) for m in MODES] + [(mat, m) for mat in ("ragged", "three", "wide", "long")
                                            for m in ("none", "secded")]


@pytest.fixture(scope="module")
def mats():
    return {name: make() for name, make in MATS.items()}


# ---- 1. spmm_dot against spmm ----

@pytest.mark.parametrize("mat,mode", SPMM_CASES)
def test_spmm_dot_against_spmm(amd, mats, mat, mode):
    box = Box(amd, mode, mats[mat])
    n = box.n
    try:
        for k in KS:
            X = block_x(n, k)
            bx = box.block(X)
            w0, w1 = box.block(np.full((n, k), np.nan)), box.block(np.full((n, k), np.nan))
            box.ctx.spmm(box.A, bx, w0, k)
            W = box.ctx.download(w0)
            d = box.ctx.spmm_dot(box.A, bx, w1, k)
            assert bits_equal(box.ctx.download(w1), W), (mat, mode, k)
            assert d.shape == (k,)
            for j in range(k):
                terms = float(np.abs(X[:, j] * W[:, j]).sum())
                err = abs(d[j] - ora_dot(X[:, j], W[:, j]))
                print("%s %s k=%d j=%d: |sum - serial| = %.3e, bar %.3e" % (mat, mode, k, j, err, 1e-13 * terms))
                assert err <= 1e-13 * terms, (mat, mode, k, j)
            # the fold order is fixed: the same bits again
            d2 = box.ctx.spmm_dot(box.A, bx, w1, k)
            assert bits_equal(d, d2), (mat, mode, k)
            # column j = 2^j column 0: W scales exactly, and so does every sum
            two = np.stack([X[:, 0] * 2.0 ** j for j in range(k)], axis=1)
            box.ctx.upload(bx, two)
            d3 = box.ctx.spmm_dot(box.A, bx, w1, k)
            assert d3[0] == d[0]
            assert all(d3[j] == d3[0] * 4.0 ** j for j in range(k)), (mat, mode, k, d3)
            for v in (bx, w0, w1):
                box.ctx.destroy_vector(v)
        assert box.take() == ([], False)
    finally:
        box.ctx.close()


# ---- 2. events ----

def flipped_run(amd, mat, flips, k, fused):
    box = Box(amd, "secded", mat)
    try:
        for i, bits in flips:
            box.ctx.inject_at(box.A, i, bits)
        X = block_x(box.n, k, seed=50)
        bx, bw = box.block(X), box.block(np.full((box.n, k), np.nan))
        if fused:
            d = box.ctx.spmm_dot(box.A, bx, bw, k)
        else:
            box.ctx.spmm(box.A, bx, bw, k)
            d = None
        ev = box.take()
        return ev, box.words(bw), d, box.ctx.stored_words(box.A)
    finally:
        box.ctx.close()


@pytest.mark.parametrize("mat", ["lap", "long"])
@pytest.mark.parametrize("k", [1, 4])
def test_spmm_dot_repairs_with_spmms_events(amd, mats, mat, k):
    nnz = len(mats[mat][2])
    clean = flipped_run(amd, mats[mat], [], k, True)
    assert clean[0] == ([], False)
    for flip in ([(nnz // 2, [40])], [(7, [70])], [(nnz - 1, [5]), (nnz // 3, [90])]):
        ref = flipped_run(amd, mats[mat], flip, k, False)
        got = flipped_run(amd, mats[mat], flip, k, True)
        assert got[0] == ref[0] and not got[0][1] and len(got[0][0]) == len(flip), (flip, got[0], ref[0])
        assert np.array_equal(got[3], ref[3]) and np.array_equal(got[3], clean[3])  # repaired in memory
        assert np.array_equal(got[1], clean[1]) and np.array_equal(got[1], ref[1])
        assert bits_equal(got[2], clean[2]), (flip, got[2], clean[2])


def test_spmm_dot_double_flip_is_fatal(amd, mats):
    nnz = len(mats["lap"][2])
    flip = [(nnz // 2, [3, 40])]
    ref = flipped_run(amd, mats["lap"], flip, 3, False)
    got = flipped_run(amd, mats["lap"], flip, 3, True)
    assert got[0] == ref[0] and got[0][1] and got[0][0][0][0] == 4, (got[0], ref[0])
    assert np.array_equal(got[1], ref[1])
    # without an event handler the fatal line ends the call, as for spmm
    cols, rows, vals, n = mats["lap"]
    ctx = amd.HIPContext("secded", "csr")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        X, W = ctx.create_block(n, 3), ctx.create_block(n, 3)
        ctx.upload(X, block_x(n, 3))
        ctx.inject_at(A, nnz // 2, [3, 40])
        with pytest.raises(amd.FatalEvent):
            ctx.spmm_dot(A, X, W, 3)
    finally:
        ctx.close()


# ---- 3. calc_r_block and calc_px_block against the existing calls, bit for bit ----

def masks(k):
    return sorted({(1 << k) - 1, 0, 1 << (k // 2), sum(1 << j for j in range(0, k, 2))})


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025, 4099])
def test_fused_vector_calls_bit_for_bit(amd, n, offset):
    box = Box(amd, "none")
    ctx = box.ctx
    try:
        for k in (1, 3, 4, 8):
            rng = np.random.default_rng(1000 * n + 10 * k + offset)
            if offset and k % 2 == 0:
                # an even k moves pairs: a view at an odd offset is refused, by the new calls as by the old
                v = [box.block(rng.standard_normal((n, k)), offset if i == 0 else 0) for i in range(3)]
                before = [box.words(a) for a in v]
                with pytest.raises(amd.AbftError) as e:
                    ctx.calc_r_block(v[0], v[1], k, np.ones(k), 1)
                assert "16-byte aligned" in str(e.value)
                with pytest.raises(amd.AbftError) as e:
                    ctx.calc_px_block(v[0], v[1], v[2], k, np.ones(k), np.ones(k), 1)
                assert "16-byte aligned" in str(e.value)
                assert all(np.array_equal(box.words(a), b) for a, b in zip(v, before))
                continue
            for active in masks(k):
                for pre in (False, True):
                    x, r, p, w = (rng.standard_normal((n, k)) for _ in range(4))
                    alpha, beta = rng.standard_normal(k), rng.standard_normal(k)
                    dinv = rng.random(n) + 0.25
                    for j in range(k):
                        if not (active >> j) & 1:  # an inactive column keeps whatever it holds
                            for a in (x, r, p):
                                a[::3, j] = np.nan
                                a[1::3, j] = -0.0
                    old = [box.block(a, offset) for a in (x, r, p, w)]
                    new = [box.block(a, offset) for a in (x, r, p, w)]
                    if pre:
                        dv = box.vec(dinv, (k + offset) % 2)
                        rz0, rr0 = ctx.calc_xr_precond_block(old[0], old[1], old[2], old[3], dv, k, alpha, active)
                        ctx.calc_p_precond_block(old[2], old[1], dv, k, beta, active)
                        rz1, rr1 = ctx.calc_r_block(new[1], new[3], k, alpha, active, dv)
                        assert bits_equal(rz1, rz0), (n, k, active)
                    else:
                        dv = None
                        rr0 = ctx.calc_xr_block(old[0], old[1], old[2], old[3], k, alpha, active)
                        ctx.calc_p_block(old[2], old[1], k, beta, active)
                        rr1 = ctx.calc_r_block(new[1], new[3], k, alpha, active)
                    assert bits_equal(rr1, rr0), (n, k, active, pre)
                    assert np.array_equal(box.words(new[1]), box.words(old[1])), (n, k, active, pre)
                    # x and p untouched so far; then both in one pass
                    assert np.array_equal(box.words(new[0]), x.view(U).reshape(-1))
                    assert np.array_equal(box.words(new[2]), p.view(U).reshape(-1))
                    ctx.calc_px_block(new[0], new[2], new[1], k, alpha, beta, active, dv)
                    for i in (0, 1, 2, 3):
                        assert np.array_equal(box.words(new[i]), box.words(old[i])), (n, k, active, pre, i)
                    got = [ctx.download(a).reshape(n, k) for a in new[:3]]
                    for j in range(k):
                        if not (active >> j) & 1:
                            for g, a in zip(got, (x, r, p)):
                                assert bits_equal(g[:, j], a[:, j]), (n, k, active, pre, j)
                    for a in old + new + ([dv] if pre else []):
                        if a.h and not offset:
                            ctx.destroy_vector(a)
        assert box.take() == ([], False)
    finally:
        ctx.close()


# ---- 4. refusals ----

def refused(box, vectors, call, *needles):
    before = [box.words(v) for v in vectors]
    with pytest.raises(Exception) as e:
        call()
    assert type(e.value).__name__ == "AbftError", repr(e.value)
    for s in needles:
        assert s in str(e.value), (s, str(e.value))
    for v, b in zip(vectors, before):
        assert np.array_equal(box.words(v), b)


def test_refusals(amd, mats):
    cols, rows, vals, n = laplace5(20, 20)
    rng = np.random.default_rng(5)
    ones = np.ones(3)
    # a COO context
    box = Box(amd, "sec7", fmt="coo")
    try:
        A = box.ctx.create_matrix(cols, rows, vals, n, len(vals))
        X, W = box.block(rng.standard_normal((n, 2))), box.block(rng.standard_normal((n, 2)))
        refused(box, [X, W], lambda: box.ctx.spmm_dot(A, X, W, 2), "spmm_dot", "COO")
    finally:
        box.ctx.close()
    box = Box(amd, "sec7", (cols, rows, vals, n))
    ctx = box.ctx
    try:
        # a matrix that is not square (two more columns than rows)
        wide = ctx.create_matrix(cols, rows, vals, n, len(vals), n_in=n + 2)
        X, W = box.block(rng.standard_normal((n, 2))), box.block(rng.standard_normal((n, 2)))
        if ctx.matrix_info(wide)[0] == "stream":
            refused(box, [X, W], lambda: ctx.spmm_dot(wide, X, W, 2), "spmm_dot", "not square")
        else:
            refused(box, [X, W], lambda: ctx.spmm_dot(wide, X, W, 2), "spmm_dot", "layout")
        # k = 9
        for k in (9,):
            m = k
            V = [box.vec(rng.standard_normal(n * m)) for _ in range(3)]
            dv = box.vec(rng.random(n) + 1.0)
            msg = "k = %d outside [1, 8]" % k
            a = np.ones(m)
            refused(box, V, lambda: ctx.spmm_dot(box.A, V[0], V[1], k), msg)
            refused(box, V, lambda: ctx.calc_r_block(V[0], V[1], k, a[:8], 1), msg)
            refused(box, V, lambda: ctx.calc_px_block(V[0], V[1], V[2], k, a[:8], a[:8], 1), msg)
            refused(box, V, lambda: ctx.calc_r_block(V[0], V[1], k, a[:8], 1, dv), msg)
            refused(box, V, lambda: ctx.calc_px_block(V[0], V[1], V[2], k, a[:8], a[:8], 1, dv), msg)
        # short operands
        k = 3
        full = [box.block(rng.standard_normal((n, k))) for _ in range(3)]
        short = box.block(rng.standard_normal((n - 1, k)))
        dv, dshort = box.vec(rng.random(n) + 1.0), box.vec(rng.random(n - 1) + 1.0)
        allv = full + [short, dv, dshort]
        nb = "not a block of"
        refused(box, allv, lambda: ctx.spmm_dot(box.A, full[0], short, k), nb)
        refused(box, allv, lambda: ctx.spmm_dot(box.A, short, full[0], k), nb)
        refused(box, allv, lambda: ctx.calc_r_block(full[0], short, k, ones, 7), nb)
        refused(box, allv, lambda: ctx.calc_r_block(short, full[0], k, ones, 7), nb)
        refused(box, allv, lambda: ctx.calc_px_block(full[0], full[1], short, k, ones, ones, 7), nb)
        refused(box, allv, lambda: ctx.calc_px_block(full[0], short, full[2], k, ones, ones, 7), nb)
        refused(box, allv, lambda: ctx.calc_px_block(short, full[1], full[2], k, ones, ones, 7), nb)
        refused(box, allv, lambda: ctx.calc_r_block(full[0], full[1], k, ones, 7, dshort), nb)
        refused(box, allv, lambda: ctx.calc_px_block(full[0], full[1], full[2], k, ones, ones, 7, dshort), nb)
        # overlapping views
        big = box.vec(rng.standard_normal(2 * n * k + n))
        a0 = ctx.view_vector(big, 0, n * k)
        a1 = ctx.view_vector(big, n * k - 3, n * k)   # overlaps a0's tail
        a2 = ctx.view_vector(big, 2 * n * k - 8, n)   # an n-entry dinv over a1's tail
        for v in (a0, a1):
            v.K = k
        allv = full + [big, dv]
        ov = "overlap"
        refused(box, allv, lambda: ctx.spmm_dot(box.A, a0, a1, k), ov)
        refused(box, allv, lambda: ctx.spmm_dot(box.A, a0, a0, k), ov)
        refused(box, allv, lambda: ctx.calc_r_block(a0, a1, k, ones, 7), ov)
        refused(box, allv, lambda: ctx.calc_r_block(a1, a0, k, ones, 7, dv), ov)
        refused(box, allv, lambda: ctx.calc_px_block(a0, a1, full[0], k, ones, ones, 7), ov)
        refused(box, allv, lambda: ctx.calc_px_block(a0, full[0], a1, k, ones, ones, 7), ov)
        refused(box, allv, lambda: ctx.calc_px_block(full[0], a0, a1, k, ones, ones, 7, dv), ov)
        refused(box, allv, lambda: ctx.calc_r_block(a1, full[0], k, ones, 7, a2), "dinv overlaps")
        refused(box, allv, lambda: ctx.calc_px_block(full[0], a1, full[1], k, ones, ones, 7, a2), "dinv overlaps")
        refused(box, allv, lambda: ctx.calc_px_block(a1, full[0], full[1], k, ones, ones, 7, a2), "dinv overlaps")
        assert box.take() == ([], False)
    finally:
        ctx.close()


LAYOUT_PROBE = r'''
import sys
sys.path.insert(0, "tests")
import numpy as np
import abft_sparse_cg_amd as amd
from _oracle import laplace5
want = sys.argv[1]
cols, rows, vals, n = laplace5(40, 33)
ctx = amd.HIPContext("sec8", "csr")
A = ctx.create_matrix(cols, rows, vals, n, len(vals))
assert ctx.matrix_info(A)[0] == want, ctx.matrix_info(A)
X, W = ctx.create_block(n, 2), ctx.create_block(n, 2)
x, w = np.random.default_rng(1).standard_normal((2, n, 2))
ctx.upload(X, x)
ctx.upload(W, w)
try:
    ctx.spmm_dot(A, X, W, 2)
except amd.AbftError as e:
    assert "spmm_dot" in str(e) and want[:5] in str(e) and "abft_hip_matrix_create_csr_stream" in str(e), str(e)
else:
    raise AssertionError("spmm_dot ran on the %s layout" % want)
assert np.array_equal(ctx.download(X).view(np.uint64), x.view(np.uint64))
assert np.array_equal(ctx.download(W).view(np.uint64), w.view(np.uint64))
S = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
d = ctx.spmm_dot(S, X, W, 2)
assert np.all(d > 0)
ctx.close()
print("ok")
'''


@pytest.mark.parametrize("layout,want", [("sweep", "sweep"), ("panels", "panels")])
def test_spmm_dot_refuses_the_other_layouts(layout, want):
    env = dict(os.environ, ABFT_HIP_LAYOUT=layout, ABFT_HIP_PANEL_WIDTH="16")
    p = subprocess.run([sys.executable, "-c", LAYOUT_PROBE, want], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


# ---- 5. solves ----

class Run:
    pass


def solve(amd, mat, jacobi, conv, fused, k=3, **kw):
    cols, rows, vals, n = mat
    box = Box(amd, "secded", mat)
    ctx = box.ctx
    try:
        B = np.stack([rhs(n, 1 + j) for j in range(k)], axis=1)
        V = [ctx.create_block(n, k) for _ in range(5)]
        ctx.upload(V[0], B)
        ctx.upload(V[1], np.zeros((n, k)))
        r = Run()
        r.hist, r.records = [], []
        flip = kw.pop("flip", None)

        def on_iteration(i, rr, active):
            r.hist.append((rr, active))
            if flip is not None and i == flip[0]:
                ctx.flip_vector(V[1], flip[1], flip[2])

        if jacobi:
            kw["precond"] = ctx.jacobi(box.A)
        r.itrs, r.rr = amd.cg_solve_block(ctx, box.A, *V, max_itrs=2000, conv_threshold=conv, on_iteration=on_iteration,
                                          on_check=lambda *e: r.records.append(e), **dict(kw, **({"fused": True} if fused else {})))
        r.x = ctx.download(V[1])
        r.res = [float(np.linalg.norm(B[:, j] - matvec(cols, rows, vals, n, np.ascontiguousarray(r.x[:, j]))))
                 for j in range(k)]
        assert box.take() == ([], False)
        return r
    finally:
        ctx.close()


def stop_rr(run, j):
    """column j's rr at its stopping step"""
    return [rr[j] for rr, active in run.hist if (active >> j) & 1][-1]


@pytest.mark.parametrize("conv", [1e-3, 1e-10])
@pytest.mark.parametrize("system", ["laplace", "scaled-jacobi"])
def test_fused_solve_follows_the_unfused_one(amd, mats, system, conv):
    from abft_sparse_cg_amd.context import threshold_ambiguous
    mat = mats["lap"] if system == "laplace" else scaled(*mats["lap"])
    jacobi = system != "laplace"
    off, on = solve(amd, mat, jacobi, conv, False), solve(amd, mat, jacobi, conv, True)
    print("iterations: unfused %s, fused %s" % (off.itrs, on.itrs))
    print("residuals: unfused %s, fused %s" % (off.res, on.res))
    skipped = 0
    for j in range(3):
        assert 0 < off.itrs[j] < 2000
        if threshold_ambiguous(stop_rr(off, j), conv):
            skipped += 1
            continue
        assert on.itrs[j] == off.itrs[j], (j, on.itrs, off.itrs)
    assert skipped <= 1
    for j in range(3):
        assert on.res[j] <= 10 * off.res[j], (j, on.res, off.res)


def test_fused_solve_rolls_back_one_column(amd, mats):
    mat = mats["lap"]
    n = mat[3]
    flip = (7, (n // 2) * 3 + 1, [58])  # after iteration 7: X[n // 2, 1]
    off = solve(amd, mat, False, 1e-10, False, check_every=5, flip=flip)
    on = solve(amd, mat, False, 1e-10, True, check_every=5, flip=flip)
    shape = lambda run: [(i, ok, back, j) for i, gap, ok, back, j in run.records]
    failed = [e for e in on.records if not e[2]]
    print("fused: iterations %s, failed checks %s" % (on.itrs, failed))
    assert failed and all(e[4] == 1 for e in failed)
    assert shape(on) == shape(off)
    assert on.itrs == off.itrs and all(0 < i < 2000 for i in on.itrs)
    for j in range(3):
        assert on.rr[j] <= 1e-10
        assert on.res[j] <= 10 * off.res[j], (j, on.res, off.res)


# ---- 6. CLI ----

def cli(args):
    p = subprocess.run([sys.executable, "-m", "abft_sparse_cg_amd.cg", "-t", "hip", "-s", "laplace5:40,40", "-m",
                        "secded", "-i", "300", "-c", "1e-8"] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_cli_block_fused():
    base = cli(["--rhs", "3"])
    out = cli(["--rhs", "3", "--block-fused"])
    assert "block iteration: fused" not in base
    assert out.count("block iteration: fused\n") == 1
    assert out.index("block iteration: fused") < out.index("iteration     0 :")
    ran = re.findall(r"rhs \d: ran for \d+ iterations", out)
    assert len(ran) == 3 and ran == re.findall(r"rhs \d: ran for \d+ iterations", base)
    # everything but the flag's line, the residuals' last digits and the time is the same text
    strip = lambda s: [l for l in s.splitlines() if not re.match(r"iteration +\d+ :|block iteration|time taken|rhs \d: (total|max) error", l)]
    assert strip(out) == strip(base)
