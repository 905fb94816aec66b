"""CPU-side checks of the fused block iteration (abft_hip_spmm_dot, abft_hip_calc_r_block,
abft_hip_calc_px_block and their Jacobi forms; cg_solve_block(..., fused=True); the CLI's --block-fused):
the header declares the five entries and the built library exports them, the solver's call sequence with
and without the option against a recording stand-in for the context, and the flag's parsing.

As in test_block_host.py, whatever loads the package runs in a child interpreter."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["abft_hip_spmm_dot", "abft_hip_calc_r_block", "abft_hip_calc_px_block", "abft_hip_calc_r_precond_block",
       "abft_hip_calc_px_precond_block"]


def child(code):
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_header_declares_the_fused_entries():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_capi_symbols import declared_symbols
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s


def test_library_exports_the_fused_entries():
    out = child("""
import ctypes
from abft_sparse_cg_amd import capi
lib = ctypes.CDLL(capi.LIB_PATH)
missing = [s for s in %r if not hasattr(lib, s) or s not in capi.SIGNATURES]
assert not missing, missing
print("ok")
""" % (NEW,))
    assert out.strip() == "ok"


# A recording stand-in for HIPContext: every operation of cg_solve_block in numpy (each reduction np.sum
# over a contiguous column, so the fused and the unfused calls see the same bits and the two loops take
# the same decisions), every call appended to .calls by name -- the vector calls with whether they got
# a dinv, spmm / spmm_dot with their drain argument.
STANDIN = r'''
import numpy as np
from abft_sparse_cg_amd.context import cg_solve_block

class V:
    def __init__(self, a, K=None):
        self.a, self.K, self.N = a, K, a.size

def col(v, j):
    return np.ascontiguousarray(v.a[:, j])

def sums(a, b, k):
    return np.array([float(np.sum(col(a, j) * col(b, j))) for j in range(k)])

class Rec:
    def __init__(self, A, flip=None):
        self.A, self.calls, self.flip, self.iters = A, [], flip, 0
    def create_block(self, n, k):
        return V(np.zeros((n, k)), k)
    def destroy_vector(self, v):
        pass
    def copy_vector(self, d, s):
        self.calls.append(("copy",)); d.a[:] = s.a
    def copy_block(self, d, s, k, mask):
        self.calls.append(("copy_block", mask))
        for j in range(k):
            if (mask >> j) & 1:
                d.a[:, j] = s.a[:, j]
    def dot_block(self, a, b, k):
        self.calls.append(("dot_block",)); return sums(a, b, k)
    def _mm(self, x, y, k):
        for j in range(k):
            y.a[:, j] = self.A @ col(x, j)
    def spmm(self, A, x, y, k, drain=True):
        self.calls.append(("spmm", drain)); self._mm(x, y, k)
    def spmm_dot(self, A, x, y, k, drain=True):
        self.calls.append(("spmm_dot", drain)); self._mm(x, y, k); return sums(x, y, k)
    def _r(self, r, w, k, alpha, active, dinv):
        for j in range(k):
            if (active >> j) & 1:
                r.a[:, j] = r.a[:, j] - alpha[j] * w.a[:, j]
        rr = sums(r, r, k)
        if dinv is None:
            return rr
        z = V(dinv.a[:, None] * r.a)
        return sums(r, z, k), rr
    def _x(self, x, p, k, alpha, active):
        for j in range(k):
            if (active >> j) & 1:
                x.a[:, j] = x.a[:, j] + alpha[j] * p.a[:, j]
    def _p(self, p, r, k, beta, active, dinv):
        for j in range(k):
            if (active >> j) & 1:
                z = r.a[:, j] if dinv is None else dinv.a * r.a[:, j]
                p.a[:, j] = z + beta[j] * p.a[:, j]
    def _after(self, x):
        self.iters += 1
        if self.flip and self.flip[0] == self.iters:
            x.a[self.flip[1], self.flip[2]] += 1e3
    def calc_xr_block(self, x, r, p, w, k, alpha, active):
        self.calls.append(("calc_xr", False)); self._x(x, p, k, alpha, active)
        return self._r(r, w, k, alpha, active, None)
    def calc_p_block(self, p, r, k, beta, active):
        self.calls.append(("calc_p", False)); self._p(p, r, k, beta, active, None); self._after(self.x)
    def calc_xr_precond_block(self, x, r, p, w, dinv, k, alpha, active):
        self.calls.append(("calc_xr", True)); self._x(x, p, k, alpha, active)
        return self._r(r, w, k, alpha, active, dinv)
    def calc_p_precond_block(self, p, r, dinv, k, beta, active):
        self.calls.append(("calc_p", True)); self._p(p, r, k, beta, active, dinv); self._after(self.x)
    def calc_r_block(self, r, w, k, alpha, active, dinv=None):
        self.calls.append(("calc_r", dinv is not None))
        return self._r(r, w, k, alpha, active, dinv)
    def calc_px_block(self, x, p, r, k, alpha, beta, active, dinv=None):
        self.calls.append(("calc_px", dinv is not None))
        self._x(x, p, k, alpha, active); self._p(p, r, k, beta, active, dinv); self._after(x)
    def precond_start_block(self, r, dinv, p, k, mask):
        self.calls.append(("precond_start", mask))
        z = V(dinv.a[:, None] * r.a)
        for j in range(k):
            if (mask >> j) & 1:
                p.a[:, j] = z.a[:, j]
        return sums(r, z, k), sums(r, r, k)
    def residual_gap_block(self, A, b, x, r, scratch, k, active):
        self.calls.append(("gap", active)); self._mm(x, scratch, k)
        t = V(b.a - scratch.a); g = V(t.a - r.a)
        on = np.array([(active >> j) & 1 for j in range(k)], dtype=float)
        return sums(g, g, k) * on, sums(t, t, k) * on
    def residual_restart_block(self, A, b, x, r, p, scratch, k, mask):
        self.calls.append(("restart", mask)); self._mm(x, scratch, k)
        for j in range(k):
            if (mask >> j) & 1:
                r.a[:, j] = b.a[:, j] - scratch.a[:, j]; p.a[:, j] = r.a[:, j]
        return sums(r, r, k)

def spd(n, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    return M @ M.T / n + np.diag(np.linspace(0.05, 3.0, n))

def run(A, B, precond=False, flip=None, **kw):
    s = Rec(A, flip)
    n, k = B.shape
    mk = lambda a: V(a, k)
    vb, vx, vr, vp, vw = mk(B.copy()), mk(np.zeros((n, k))), mk(np.zeros((n, k))), mk(np.zeros((n, k))), mk(np.zeros((n, k)))
    s.x = vx
    if precond:
        kw["precond"] = V(1.0 / np.diag(A).copy())
    hist = []
    itrs, rr = cg_solve_block(s, None, vb, vx, vr, vp, vw, 1000, 1e-10, on_iteration=lambda i, r, a: hist.append(a), **kw)
    return s.calls, list(itrs), rr, vx.a, hist

def fuse(calls):
    """today's call list with every spmm / dot_block / calc_xr / calc_p run replaced by the fused triple"""
    out, i = [], 0
    while i < len(calls):
        if calls[i][0] == "spmm":
            names = [c[0] for c in calls[i:i + 4]]
            assert names == ["spmm", "dot_block", "calc_xr", "calc_p"], names
            assert calls[i] == ("spmm", False)
            pre = calls[i + 2][1]
            assert calls[i + 3][1] == pre
            out += [("spmm_dot", False), ("calc_r", pre), ("calc_px", pre)]
            i += 4
        else:
            out.append(calls[i]); i += 1
    return out

n = 40
A = spd(n, 3)
B = np.random.default_rng(7).random((n, 4)) * np.array([1e-3, 1.0, 30.0, 5.0])
'''


def test_fused_false_makes_todays_calls():
    out = child(STANDIN + r'''
for pre in (False, True):
    for kw in ({}, {"check_every": 5}):
        base = run(A, B, pre, **kw)
        off = run(A, B, pre, fused=False, **kw)
        assert off[0] == base[0] and off[1] == base[1] and np.array_equal(off[3], base[3])
        names = {c[0] for c in base[0]}
        assert not names & {"spmm_dot", "calc_r", "calc_px"}, names
        assert {"spmm", "dot_block", "calc_xr", "calc_p"} <= names
print("ok")
''')
    assert out.strip() == "ok"


def test_fused_true_makes_the_three_call_iteration():
    out = child(STANDIN + r'''
cases = 0
for Bk in (B, B[:, 1:2].copy()):  # K = 4 and K = 1
    for pre in (False, True):
        for kw in ({}, {"check_every": 5}, {"check_every": 3, "flip": (7, 11, Bk.shape[1] - 1)}):
            kw = dict(kw)
            flip = kw.pop("flip", None)
            base = run(A, Bk, pre, flip=flip, **kw)
            on = run(A, Bk, pre, flip=flip, fused=True, **kw)
            # the same decisions (the stand-in's sums are the same bits either way) ...
            assert on[1] == base[1] and on[4] == base[4] and np.array_equal(on[3], base[3])
            # ... through exactly spmm_dot, calc_r_block, calc_px_block per iteration, the checks, copies,
            # restarts and the start-up calls where they were
            assert on[0] == fuse(base[0]), (on[0][:12], fuse(base[0])[:12])
            names = [c[0] for c in on[0]]
            assert not set(names) & {"spmm", "calc_xr", "calc_p"}
            assert names.count("dot_block") == (0 if pre else 1)  # the start's R . R alone
            it = [c for c in on[0] if c[0] in ("spmm_dot", "calc_r", "calc_px")]
            assert len(it) == 3 * len(on[4])
            for i in range(0, len(it), 3):
                assert it[i:i + 3] == [("spmm_dot", False), ("calc_r", pre), ("calc_px", pre)]
            if flip:
                assert any(c[0] == "restart" for c in on[0])
            cases += 1
assert cases == 12
print("ok")
''')
    assert out.strip() == "ok"


def test_block_fused_flag():
    out = child("""
from abft_sparse_cg_amd import cg
assert cg.parse(["cg"])["block_fused"] is False
assert cg.parse(["cg", "--rhs", "3"])["block_fused"] is False
assert cg.parse(["cg", "--rhs", "3", "--block-fused"])["block_fused"] is True
assert cg.parse(["cg", "--block-fused", "--rhs", "8"])["block_fused"] is True
for bad in (["--block-fused"], ["--block-fused", "--rhs", "1"]):
    try:
        cg.parse(["cg"] + bad)
    except SystemExit as e:
        assert e.code == 1, bad
    else:
        raise AssertionError(bad)
print("ok")
""")
    assert out.strip().endswith("ok")
    assert "--block-fused" in out
    p = subprocess.run([sys.executable, "-m", "abft_sparse_cg_amd.cg", "-t", "hip", "-s", "laplace5:10,10",
                        "--block-fused"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 1 and "--block-fused" in p.stdout, p.stdout + p.stderr
