"""CPU-side checks of the residual checks with rollback (abft_hip_vector_flip, abft_hip_residual_*,
abft_hip_copy_block): the header declares the entries and the built library exports them, the CLI
parses the new flags like the other flags, and the control flow of cg_solve / cg_solve_block with
check_every > 0 -- when a check runs, what a failure restores, what the iteration count counts --
checked against numpy stand-ins for the context's operations.

As in test_block_host.py, whatever loads the package runs in a child interpreter."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["abft_hip_vector_flip", "abft_hip_residual_gap", "abft_hip_residual_restart", "abft_hip_residual_gap_block",
       "abft_hip_residual_restart_block", "abft_hip_copy_block"]


def child(code):
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_header_declares_the_residual_check_entries():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_capi_symbols import declared_symbols
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s


def test_library_exports_the_residual_check_entries():
    out = child("""
import ctypes
from abft_sparse_cg_amd import capi
lib = ctypes.CDLL(capi.LIB_PATH)
missing = [s for s in %r if not hasattr(lib, s) or s not in capi.SIGNATURES]
assert not missing, missing
print("ok")
""" % (NEW,))
    assert out.strip() == "ok"


def test_check_flags_are_parsed_like_the_other_flags():
    out = child("""
from abft_sparse_cg_amd import cg
o = cg.parse(["cg"])
assert (o["check_every"], o["check_tol"], o["max_rollbacks"], o["flip_vector"]) == (0, 1e-7, 3, [])
o = cg.parse(["cg", "--check-every", "5", "--check-tol", "1e-6", "--max-rollbacks", "0",
              "--flip-vector", "10:x:123:55", "--flip-vector", "3:p:0:1,62"])
assert (o["check_every"], o["check_tol"], o["max_rollbacks"]) == (5, 1e-6, 0), o
assert o["flip_vector"] == [(10, "x", 123, [55]), (3, "p", 0, [1, 62])], o["flip_vector"]
bad = [["--check-every", "-1"], ["--check-every", "x"], ["--check-every"], ["--check-tol", "0"],
       ["--check-tol", "-1e-3"], ["--check-tol", "inf"], ["--check-tol", "nan"], ["--check-tol", "t"],
       ["--max-rollbacks", "-1"], ["--max-rollbacks", "y"], ["--flip-vector", "10:w:1:3"],
       ["--flip-vector", "10:x:1"], ["--flip-vector", "10:x:1:64"], ["--flip-vector", "-1:x:1:3"],
       ["--flip-vector", "10:x:-1:3"], ["--flip-vector", "a:x:1:3"], ["--flip-vector", "10:x:1:3,"],
       ["--flip-vector"]]
for b in bad:
    try:
        cg.parse(["cg"] + b)
    except SystemExit as e:
        assert e.code == 1, b
    else:
        raise AssertionError(b)
print("ok")
""")
    assert out.strip().endswith("ok")
    for msg in ("Invalid residual check interval", "Invalid residual check tolerance", "Invalid number of rollbacks",
                "Invalid --flip-vector"):
        assert msg in out, msg


# numpy stand-ins for the single context and the block one, with the new calls; every reduction is
# np.sum over a contiguous column, so residual_restart's r.r is the bits dot(r, r) gives
STANDIN = r'''
import math
import numpy as np
from abft_sparse_cg_amd.context import cg_solve, cg_solve_block, fdiv, ResidualCheckFailed

class V:
    def __init__(self, a, K=None):
        self.a, self.K, self.N = a, K, a.size  # as Vector.N: N * K entries for a block

def col(v, j):
    return np.ascontiguousarray(v.a[:, j])

def flip(a, i, bits):
    u = a.reshape(-1).view(np.uint64)
    for bit in bits:
        u[i] ^= np.uint64(1) << np.uint64(bit)

class Single:
    def __init__(self, A):
        self.A, self.calls = A, []
    def create_vector(self, n):
        self.calls.append(("create",)); return V(np.zeros(n))
    def destroy_vector(self, v):
        self.calls.append(("destroy",))
    def copy_vector(self, d, s):
        self.calls.append(("copy",)); d.a[:] = s.a
    def dot(self, a, b):
        self.calls.append(("dot",)); return float(np.sum(a.a * b.a))
    def spmv(self, A, x, y):
        self.calls.append(("spmv",)); y.a[:] = self.A @ x.a
    def calc_xr(self, x, r, p, w, alpha):
        self.calls.append(("calc_xr", alpha))
        x.a[:] = x.a + alpha * p.a; r.a[:] = r.a - alpha * w.a
        return float(np.sum(r.a * r.a))
    def calc_p(self, p, r, beta):
        self.calls.append(("calc_p", beta)); p.a[:] = r.a + beta * p.a
    def residual_gap(self, A, b, x, r, w):
        self.calls.append(("gap",))
        w.a[:] = self.A @ x.a
        t = b.a - w.a
        g = t - r.a
        return float(np.sum(g * g)), float(np.sum(t * t))
    def residual_restart(self, A, b, x, r, p, w):
        self.calls.append(("restart",))
        w.a[:] = self.A @ x.a
        r.a[:] = b.a - w.a
        p.a[:] = r.a
        return float(np.sum(r.a * r.a))
    def flip_vector(self, v, i, bits):
        flip(v.a, i, bits)

class Block:
    def __init__(self, A):
        self.A, self.calls = A, []
    def create_block(self, n, k):
        self.calls.append(("create",)); return V(np.zeros((n, k)), k)
    def destroy_vector(self, v):
        self.calls.append(("destroy",))
    def copy_vector(self, d, s):
        self.calls.append(("copy",)); d.a[:] = s.a
    def dot_block(self, a, b, k):
        self.calls.append(("dot",))
        return np.array([float(np.sum(col(a, j) * col(b, j))) for j in range(k)])
    def spmm(self, A, x, y, k, drain=True):
        self.calls.append(("spmv",))
        for j in range(k):
            y.a[:, j] = self.A @ col(x, j)
    def calc_xr_block(self, x, r, p, w, k, alpha, active):
        self.calls.append(("calc_xr", active))
        for j in range(k):
            if (active >> j) & 1:
                x.a[:, j] = x.a[:, j] + alpha[j] * p.a[:, j]; r.a[:, j] = r.a[:, j] - alpha[j] * w.a[:, j]
        return np.array([float(np.sum(col(r, j) * col(r, j))) for j in range(k)])
    def calc_p_block(self, p, r, k, beta, active):
        self.calls.append(("calc_p", active))
        for j in range(k):
            if (active >> j) & 1:
                p.a[:, j] = r.a[:, j] + beta[j] * p.a[:, j]
    def residual_gap_block(self, A, B, X, R, W, k, active):
        self.calls.append(("gap", active))
        self.spmm(A, X, W, k)
        self.calls.pop()
        g2, t2 = np.zeros(k), np.zeros(k)
        for j in range(k):
            if (active >> j) & 1:
                t = col(B, j) - col(W, j)
                g = t - col(R, j)
                g2[j], t2[j] = np.sum(g * g), np.sum(t * t)
        return g2, t2
    def residual_restart_block(self, A, B, X, R, P, W, k, mask):
        self.calls.append(("restart", mask))
        self.spmm(A, X, W, k)
        self.calls.pop()
        for j in range(k):
            if (mask >> j) & 1:
                R.a[:, j] = B.a[:, j] - W.a[:, j]
                P.a[:, j] = R.a[:, j]
        return np.array([float(np.sum(col(R, j) * col(R, j))) for j in range(k)])
    def copy_block(self, dst, src, k, mask):
        self.calls.append(("copy_block", mask))
        for j in range(k):
            if (mask >> j) & 1:
                dst.a[:, j] = src.a[:, j]
    def flip_vector(self, v, i, bits):
        flip(v.a, i, bits)

def laplace(nx):
    n = nx * nx
    A = np.zeros((n, n))
    for i in range(nx):
        for j in range(nx):
            k = i * nx + j
            A[k, k] = 4.0
            for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                if 0 <= i + di < nx and 0 <= j + dj < nx:
                    A[k, (i + di) * nx + j + dj] = -1.0
    return A

def single(A, b, max_itrs, conv, flips=(), cls=Single, **kw):
    """-> (itr, rr, x, history, checks, ctx); flips: (iteration, 'x' | 'r' | 'p', index, bits)"""
    s = cls(A)
    n = len(b)
    vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
    vecs = {"x": vx, "r": vr, "p": vp}
    hist, checks = [], []
    def on_it(i, r):
        hist.append(r)
        for fi, name, idx, bits in flips:
            if fi == i:
                s.flip_vector(vecs[name], idx, bits)
    it, rr = cg_solve(s, None, vb, vx, vr, vp, vw, max_itrs, conv, on_iteration=on_it,
                      on_check=lambda *c: checks.append(c), **kw)
    return it, rr, vx.a, hist, checks, s

def block(A, B, max_itrs, conv, flips=(), **kw):
    s = Block(A)
    n, k = B.shape
    mk = lambda a: V(a, k)
    vb, vx, vr, vp, vw = mk(B.copy()), mk(np.zeros((n, k))), mk(np.zeros((n, k))), mk(np.zeros((n, k))), mk(np.zeros((n, k)))
    vecs = {"x": vx, "r": vr, "p": vp}
    hist, checks = [], []
    def on_it(i, r, act):
        hist.append((r, act))
        for fi, name, idx, bits in flips:
            if fi == i:
                s.flip_vector(vecs[name], idx, bits)
    itrs, rr = cg_solve_block(s, None, vb, vx, vr, vp, vw, max_itrs, conv, on_iteration=on_it,
                              on_check=lambda *c: checks.append(c), **kw)
    return itrs, rr, vx.a, hist, checks, s

def true_res(A, b, x):
    return float(np.linalg.norm(b - A @ x))

A = laplace(12)
n = A.shape[0]
b = np.random.default_rng(4).random(n) + 0.5
'''


def test_check_every_0_makes_todays_calls():
    out = child(STANDIN + r'''
def todays(A, b, max_itrs, conv):
    # the loop as it stood before residual checks (context.cg_solve, cg.cpp:87-118)
    s = Single(A)
    vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
    s.copy_vector(vr, vb); s.copy_vector(vp, vr)
    rr = s.dot(vr, vr)
    itr = 0
    while itr < max_itrs and rr > conv:
        s.spmv(None, vp, vw)
        alpha = fdiv(rr, s.dot(vp, vw))
        rr_new = s.calc_xr(vx, vr, vp, vw, alpha)
        s.calc_p(vp, vr, fdiv(rr_new, rr))
        rr = rr_new
        itr += 1
    return s.calls, itr, rr, vx.a

for max_itrs, conv in ((1000, 1e-20), (7, 1e-20), (0, 1e-3), (1000, 1e9)):
    calls, it0, rr0, x0 = todays(A, b, max_itrs, conv)
    for kw in ({}, {"check_every": 0}):
        it, rr, x, h, checks, s = single(A, b, max_itrs, conv, **kw)
        assert s.calls == calls and it == it0 and rr == rr0 and np.array_equal(x, x0) and checks == []
    B = np.stack([b, 2 * b[::-1], b * b], axis=1)
    itrs, rrb, X, hist, checks, s = block(A, B, max_itrs, conv, check_every=0)
    assert checks == [] and not any(c[0] in ("gap", "restart", "copy_block", "create") for c in s.calls)
print("ok")
''')
    assert out.strip() == "ok"


def test_clean_run_with_checks_keeps_the_rr_history_bit_for_bit():
    out = child(STANDIN + r'''
it0, rr0, x0, h0, _, _ = single(A, b, 1000, 1e-20)
for ce in (1, 3, 7, 50, 1000):
    it, rr, x, h, checks, s = single(A, b, 1000, 1e-20, check_every=ce)
    assert (it, rr) == (it0, rr0) and h == h0 and np.array_equal(x, x0), ce
    assert checks and all(c[2] for c in checks), ce
    # periodic checks after iterations ce-1, 2ce-1, ...; and one on the final state unless it was just checked
    want = [i for i in range(ce - 1, it0, ce)]
    if not want or want[-1] != it0 - 1:
        want.append(it0 - 1)
    assert [c[0] for c in checks] == want, (ce, [c[0] for c in checks], want)
    assert s.calls.count(("create",)) == s.calls.count(("destroy",)) == 1
print("ok")
''')
    assert out.strip() == "ok"


def test_flip_in_x_is_caught_rolled_back_and_recovered():
    out = child(STANDIN + r'''
it0, rr0, x0, h0, _, _ = single(A, b, 1000, 1e-20)
clean = true_res(A, b, x0)
i = int(np.argmax(np.abs(x0)))
for bit in (62, 55, 52, 51, 45):
    # without checks: rr still "converges", x is wrong
    it, rr, x, h, checks, _ = single(A, b, 1000, 1e-20, flips=[(7, "x", i, [bit])])
    assert not np.isfinite(true_res(A, b, x)) or true_res(A, b, x) > 1e3 * clean, bit
    assert rr <= 1e-20 and checks == []
    # with checks every 5: caught after iteration 9, rolled back to the checkpoint of iteration 4
    it, rr, x, h, checks, s = single(A, b, 1000, 1e-20, flips=[(7, "x", i, [bit])], check_every=5)
    fails = [c for c in checks if not c[2]]
    assert [(c[0], c[3]) for c in fails] == [(9, 4)], (bit, checks)
    assert h[:10] == h0[:10] and it > it0
    assert true_res(A, b, x) <= 10 * clean, (bit, true_res(A, b, x), clean)
    assert s.calls.count(("restart",)) == 1
print("ok")
''')
    assert out.strip() == "ok"


def test_flip_to_inf_or_nan_is_caught():
    out = child(STANDIN + r'''
it0, rr0, x0, h0, _, _ = single(A, b, 1000, 1e-20)
clean = true_res(A, b, x0)
s8 = Single(A)
vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
cg_solve(s8, None, vb, vx, vr, vp, vw, 8, 0.0)   # the state after iteration 7
for name, v in (("x", vx.a), ("r", vr.a)):
    i = int(np.argmax(np.abs(v)))
    e = int(v[i:i + 1].view(np.uint64)[0] >> np.uint64(52)) & 0x7FF
    bits = [52 + t for t in range(11) if not (e >> t) & 1]   # exponent all ones: inf or NaN
    it, rr, x, h, checks, s = single(A, b, 1000, 1e-20, check_every=5, flips=[(7, name, i, bits)])
    fails = [c for c in checks if not c[2]]
    # x: the periodic check after iteration 9; r: rr is NaN after iteration 8, the loop is about to
    # stop, and the check on that final state fails
    assert [(c[0], c[3]) for c in fails] == [(9 if name == "x" else 8, 4)], (name, checks)
    assert not np.isfinite(fails[0][1]) or fails[0][1] > 1e3, fails
    assert true_res(A, b, x) <= 10 * clean and np.all(np.isfinite(x))
print("ok")
''')
    assert out.strip() == "ok"


def test_flip_after_the_last_periodic_check_is_caught_by_the_final_check():
    out = child(STANDIN + r'''
it0, rr0, x0, h0, _, _ = single(A, b, 1000, 1e-20)
clean = true_res(A, b, x0)
ce = next(c for c in range(5, 12) if it0 % c >= 4)
last = (it0 // ce) * ce - 1           # the last periodic check, at least 4 iterations before the end
it, rr, x, h, checks, s = single(A, b, 1000, 1e-20, check_every=ce, flips=[(last + 2, "x", 3, [55])])
fails = [c for c in checks if not c[2]]
assert [(c[0], c[3]) for c in fails] == [(it0 - 1, last)], (checks, it0, last)
assert checks[-1][2] and true_res(A, b, x) <= 10 * clean and it > it0
# the same flip at max_itrs: rolled back and raised, x the last good checkpoint
try:
    single(A, b, it0, 1e-20, check_every=ce, flips=[(last + 2, "x", 3, [55])])
except ResidualCheckFailed as e:
    assert [(c[0], c[2], c[3]) for c in e.checks][-1] == (it0 - 1, False, last), e.checks
    assert "max_itrs" in str(e)
else:
    raise AssertionError("no ResidualCheckFailed at max_itrs")
print("ok")
''')
    assert out.strip() == "ok"


def test_a_check_that_keeps_failing_raises_after_max_rollbacks():
    out = child(STANDIN + r'''
class Broken(Single):
    def residual_gap(self, *a):
        g2, t2 = Single.residual_gap(self, *a)
        return float("nan"), t2          # NaN must fail the pass rule
for m in (0, 1, 3):
    try:
        single(A, b, 1000, 1e-20, cls=Broken, check_every=4, max_rollbacks=m)
    except ResidualCheckFailed as e:
        assert len(e.checks) == m + 1 and not any(c[2] for c in e.checks), e.checks
        # iterations count on through the rollbacks: a check every 4 of them
        assert [c[0] for c in e.checks] == [4 * t + 3 for t in range(m + 1)], e.checks
        assert [c[3] for c in e.checks] == [-1] * (m + 1)  # the checkpoint of the start
    else:
        raise AssertionError(m)
# a rollback counts towards max_itrs: iterations run, repeated ones included
class FailOnce(Single):
    n_gap = 0
    def residual_gap(self, *a):
        FailOnce.n_gap += 1
        g2, t2 = Single.residual_gap(self, *a)
        return (1.0 if FailOnce.n_gap == 2 else g2), t2
it0, _, _, h0, _, _ = single(A, b, 1000, 1e-20)
it, rr, x, h, checks, _ = single(A, b, 1000, 1e-20, cls=FailOnce, check_every=4)
assert [(c[0], c[2], c[3]) for c in checks[:3]] == [(3, True, None), (7, False, 3), (11, True, None)], checks[:3]
# iterations 4-7 ran twice (a restart from the checkpoint of iteration 3 is a fresh CG start)
assert h[:8] == h0[:8] and len(h) == it and it >= it0 + 4, (it, it0)
print("ok")
''')
    assert out.strip() == "ok"


def test_block_rollback_touches_only_its_column():
    out = child(STANDIN + r'''
k = 3
B = np.stack([b, 2 * b[::-1], np.sin(np.arange(n)) + 2.0], axis=1)
itrs0, rr0, X0, hist0, _, _ = block(A, B, 1000, 1e-20)
itrs1, rr1, X1, hist1, checks1, s1 = block(A, B, 1000, 1e-20, check_every=5)
# clean: every column's history and x bit for bit those of the run without checks
assert itrs1 == itrs0 and np.array_equal(rr1, rr0) and np.array_equal(X1, X0)
assert all(np.array_equal(a[0], c[0]) and a[1] == c[1] for a, c in zip(hist0, hist1))
assert checks1 and all(c[2] for c in checks1)
# a flip of x[row 17, column 1] after iteration 7
itrs, rr, X, hist, checks, s = block(A, B, 1000, 1e-20, check_every=5, flips=[(7, "x", 17 * k + 1, [55])])
fails = [c for c in checks if not c[2]]
assert [(c[0], c[3], c[4]) for c in fails] == [(9, 4, 1)], fails
assert ("restart", 2) in s.calls and ("copy_block", 2) in s.calls
for j in (0, 2):
    assert itrs[j] == itrs0[j] and rr[j] == rr0[j] and np.array_equal(X[:, j], X0[:, j]), j
    assert [h[0][j] for h in hist if (h[1] >> j) & 1] == [h[0][j] for h in hist0 if (h[1] >> j) & 1], j
assert itrs[1] > itrs0[1]
assert true_res(A, B[:, 1], X[:, 1]) <= 10 * true_res(A, B[:, 1], X0[:, 1])
# the single solve on column 1 with the same flip: the same iterations and checks
it, rrs, x, h, cs, _ = single(A, B[:, 1], 1000, 1e-20, check_every=5, flips=[(7, "x", 17, [55])])
assert it == itrs[1] and [c[:4] for c in checks if c[4] == 1] == cs
print("ok")
''')
    assert out.strip() == "ok"
