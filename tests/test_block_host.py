"""CPU-side checks of the block right-hand-side extension (abft_hip_spmm and the *_block calls):
the header declares the five entries and the built library exports them, the CLI's --rhs flag is
parsed like the other flags, and cg_solve_block's control flow -- per column exactly cg_solve's --
checked against numpy stand-ins for the context's operations.

As in test_capi_symbols.py, whatever loads the package runs in a child interpreter."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "abft_hip.h")
NEW = ["abft_hip_matrix_create_csr_stream", "abft_hip_spmm", "abft_hip_dot_block", "abft_hip_calc_xr_block",
       "abft_hip_calc_p_block"]


def child(code):
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_header_declares_the_block_entries():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_capi_symbols import declared_symbols
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s


def test_library_exports_the_block_entries():
    out = child("""
import ctypes
from abft_sparse_cg_amd import capi
lib = ctypes.CDLL(capi.LIB_PATH)
missing = [s for s in %r if not hasattr(lib, s) or s not in capi.SIGNATURES]
assert not missing, missing
print("ok")
""" % (NEW,))
    assert out.strip() == "ok"


def test_rhs_flag_is_parsed_like_the_other_flags():
    out = child("""
from abft_sparse_cg_amd import cg
assert cg.parse(["cg"])["rhs"] == 1
for k in range(1, 9):
    assert cg.parse(["cg", "--rhs", str(k)])["rhs"] == k
for bad in (["--rhs", "0"], ["--rhs", "9"], ["--rhs", "x"], ["--rhs", "-1"], ["--rhs"]):
    try:
        cg.parse(["cg"] + bad)
    except SystemExit as e:
        assert e.code == 1, bad
    else:
        raise AssertionError(bad)
print("ok")
""")
    assert out.strip().endswith("ok")
    assert "Invalid number of right-hand sides" in out


# numpy stand-ins: the single context (cg_solve) and the block one (cg_solve_block); every
# reduction is np.sum over a contiguous column, so column j of the block run and the single run
# on that column see the same bits
STANDIN = r'''
import numpy as np
from abft_sparse_cg_amd.context import cg_solve, cg_solve_block

class V:
    def __init__(self, a, K=None):
        self.a, self.K = a, K

def col(v, j):
    return np.ascontiguousarray(v.a[:, j])

class Single:
    def __init__(self, A):
        self.A, self.calls = A, []
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

class Block:
    def __init__(self, A):
        self.A, self.calls, self.masks = A, [], []
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
        self.masks.append(active)
        self.calls.append(("calc_xr",) + tuple(alpha))
        for j in range(k):
            if (active >> j) & 1:
                x.a[:, j] = x.a[:, j] + alpha[j] * p.a[:, j]; r.a[:, j] = r.a[:, j] - alpha[j] * w.a[:, j]
        return np.array([float(np.sum(col(r, j) * col(r, j))) for j in range(k)])
    def calc_p_block(self, p, r, k, beta, active):
        self.calls.append(("calc_p",) + tuple(beta))
        for j in range(k):
            if (active >> j) & 1:
                p.a[:, j] = r.a[:, j] + beta[j] * p.a[:, j]

def spd(n, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    return M @ M.T / n + np.diag(np.linspace(0.05, 3.0, n))

def single(A, b, max_itrs, conv):
    s = Single(A)
    n = len(b)
    vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
    hist = []
    it, rr = cg_solve(s, None, vb, vx, vr, vp, vw, max_itrs, conv, on_iteration=lambda i, r: hist.append(r))
    return it, rr, vx.a, hist, s.calls

def block(A, B, max_itrs, conv):
    s = Block(A)
    n, k = B.shape
    mk = lambda a: V(a, k)
    vb, vx, vr, vp, vw = mk(B.copy()), mk(np.zeros((n, k))), mk(np.zeros((n, k))), mk(np.zeros((n, k))), mk(np.zeros((n, k)))
    hist = []
    itrs, rr = cg_solve_block(s, None, vb, vx, vr, vp, vw, max_itrs, conv,
                              on_iteration=lambda i, r, act: hist.append((r, act)))
    return itrs, rr, vx.a, hist, s
'''


def test_cg_solve_block_stops_each_column_where_cg_solve_does():
    out = child(STANDIN + r'''
n = 40
A = spd(n, 3)
rng = np.random.default_rng(7)
# right-hand sides of very different sizes: the columns cross the threshold at different iterations
B = rng.random((n, 5)) * np.array([1e-3, 1.0, 30.0, 1e-6, 5.0])
for max_itrs, conv in ((1000, 1e-10), (1000, 1e-4), (7, 1e-10), (0, 1e-3), (1000, 1e9)):
    itrs, rr, X, hist, s = block(A, B, max_itrs, conv)
    seen = []
    for j in range(B.shape[1]):
        it, r1, x1, h1, _ = single(A, B[:, j], max_itrs, conv)
        assert itrs[j] == it, (max_itrs, conv, j, itrs[j], it)
        assert rr[j] == r1 and np.array_equal(X[:, j], x1), (j,)
        # column j's residuals over the iterations it was active: cg_solve's history
        hj = [r[j] for r, act in hist if (act >> j) & 1]
        assert hj == h1, j
        seen.append(it)
    # an iteration runs while any column is active; a frozen column never comes back
    assert len(s.masks) == max(seen)
    for j in range(B.shape[1]):
        bits = [(m >> j) & 1 for m in s.masks]
        assert bits == [1] * itrs[j] + [0] * (len(bits) - itrs[j]), (j, bits)
    assert len(set(seen)) > 1 or max_itrs in (0, 7) or conv > 1
print("ok")
''')
    assert out.strip() == "ok"


def test_cg_solve_block_k1_makes_cg_solves_calls():
    out = child(STANDIN + r'''
n = 30
A = spd(n, 5)
b = np.random.default_rng(2).random(n)
for max_itrs, conv in ((1000, 1e-9), (4, 1e-9), (0, 1e-3)):
    it, rr, x, h, calls = single(A, b, max_itrs, conv)
    itrs, rrb, X, hist, s = block(A, b.reshape(n, 1), max_itrs, conv)
    assert s.calls == calls, (s.calls[:8], calls[:8])
    assert itrs == [it] and rrb[0] == rr and np.array_equal(X[:, 0], x)
print("ok")
''')
    assert out.strip() == "ok"
