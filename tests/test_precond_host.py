"""CPU-side checks of Jacobi preconditioning (abft_hip_matrix_diag_inverse, abft_hip_precond_start,
abft_hip_calc_xr_precond, abft_hip_calc_p_precond and their block forms): the header declares the entries and
the built library exports them, the CLI parses --precond like the other flags, and the control flow of
cg_solve / cg_solve_block with precond= -- which calls replace which, what follows a rollback -- checked
against numpy stand-ins for the context's operations (those of test_residual_check_host.py, extended).

As there, whatever loads the package runs in a child interpreter."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_residual_check_host import STANDIN as BASE, child  # noqa: E402

NEW = ["abft_hip_matrix_diag_inverse", "abft_hip_precond_start", "abft_hip_calc_xr_precond",
       "abft_hip_calc_p_precond", "abft_hip_precond_start_block", "abft_hip_calc_xr_precond_block",
       "abft_hip_calc_p_precond_block"]


def test_header_declares_the_precond_entries():
    from test_capi_symbols import declared_symbols
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s


def test_library_exports_the_precond_entries():
    out = child("""
import ctypes
from abft_sparse_cg_amd import capi
lib = ctypes.CDLL(capi.LIB_PATH)
missing = [s for s in %r if not hasattr(lib, s) or s not in capi.SIGNATURES]
assert not missing, missing
print("ok")
""" % (NEW,))
    assert out.strip() == "ok"


def test_precond_flag_is_parsed_like_the_other_flags():
    out = child("""
from abft_sparse_cg_amd import cg
assert cg.parse(["cg"])["precond"] == "none"
assert cg.parse(["cg", "--precond", "jacobi"])["precond"] == "jacobi"
assert cg.parse(["cg", "--precond", "none", "--rhs", "3"])["precond"] == "none"
for b in (["--precond", "ilu"], ["--precond", "Jacobi"], ["--precond", ""], ["--precond"]):
    try:
        cg.parse(["cg"] + b)
    except SystemExit as e:
        assert e.code == 1, b
    else:
        raise AssertionError(b)
print("ok")
""")
    assert out.strip().endswith("ok")
    assert out.count("Invalid preconditioner") == 4, out


# the stand-ins with the preconditioned calls; z = dinv * r is formed where the kernels form it
STANDIN = BASE + r'''
class PSingle(Single):
    def precond_start(self, r, d, p):
        self.calls.append(("precond_start",))
        z = d.a * r.a
        p.a[:] = z
        return float(np.sum(r.a * z)), float(np.sum(r.a * r.a))
    def calc_xr_precond(self, x, r, p, w, d, alpha):
        self.calls.append(("calc_xr_precond", alpha))
        x.a[:] = x.a + alpha * p.a; r.a[:] = r.a - alpha * w.a
        z = d.a * r.a
        return float(np.sum(r.a * z)), float(np.sum(r.a * r.a))
    def calc_p_precond(self, p, r, d, beta):
        self.calls.append(("calc_p_precond", beta)); p.a[:] = d.a * r.a + beta * p.a

class PBlock(Block):
    def sums(self, r, d, k):
        return (np.array([float(np.sum(col(r, j) * (d.a * col(r, j)))) for j in range(k)]),
                np.array([float(np.sum(col(r, j) * col(r, j))) for j in range(k)]))
    def precond_start_block(self, r, d, p, k, mask):
        self.calls.append(("precond_start", mask))
        for j in range(k):
            if (mask >> j) & 1:
                p.a[:, j] = d.a * r.a[:, j]
        return self.sums(r, d, k)
    def calc_xr_precond_block(self, x, r, p, w, d, k, alpha, active):
        self.calls.append(("calc_xr_precond", active))
        for j in range(k):
            if (active >> j) & 1:
                x.a[:, j] = x.a[:, j] + alpha[j] * p.a[:, j]; r.a[:, j] = r.a[:, j] - alpha[j] * w.a[:, j]
        return self.sums(r, d, k)
    def calc_p_precond_block(self, p, r, d, k, beta, active):
        self.calls.append(("calc_p_precond", active))
        for j in range(k):
            if (active >> j) & 1:
                p.a[:, j] = d.a * r.a[:, j] + beta[j] * p.a[:, j]

def psingle(A, b, max_itrs, conv, dinv, flips=(), **kw):
    return single(A, b, max_itrs, conv, flips=flips, cls=PSingle, precond=None if dinv is None else V(dinv), **kw)

def pblock(A, B, max_itrs, conv, dinv, flips=(), **kw):
    s = PBlock(A)
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
                              on_check=lambda *c: checks.append(c), precond=None if dinv is None else V(dinv), **kw)
    return itrs, rr, vx.a, hist, checks, s

names = lambda calls: [c[0] for c in calls]
dinv = 1.0 / np.diag(A) * (1.0 + 0.5 * np.sin(np.arange(n)))   # some positive diagonal M^-1
'''


def test_precond_none_makes_todays_calls():
    out = child(STANDIN + r'''
for max_itrs, conv in ((1000, 1e-20), (7, 1e-20), (0, 1e-3), (1000, 1e9)):
    for kw in ({}, {"check_every": 4}):
        it0, rr0, x0, h0, c0, s0 = single(A, b, max_itrs, conv, **kw)           # no precond argument at all
        it, rr, x, h, c, s = psingle(A, b, max_itrs, conv, None, **kw)          # precond=None
        assert s.calls == s0.calls and (it, rr) == (it0, rr0) and h == h0 and np.array_equal(x, x0) and c == c0
        assert not any("precond" in nm for nm in names(s.calls))
        B = np.stack([b, 2 * b[::-1], b * b], axis=1)
        r0 = block(A, B, max_itrs, conv, **kw)
        r1 = pblock(A, B, max_itrs, conv, None, **kw)
        assert r1[5].calls == r0[5].calls and r1[0] == r0[0] and np.array_equal(r1[2], r0[2])
        assert not any("precond" in nm for nm in names(r1[5].calls))
print("ok")
''')
    assert out.strip() == "ok"


def test_precond_loop_is_the_specified_call_sequence():
    out = child(STANDIN + r'''
it, rr, x, h, checks, s = psingle(A, b, 1000, 1e-20, dinv)
assert it > 3 and rr <= 1e-20 and true_res(A, b, x) < 1e-8
assert names(s.calls) == ["copy", "precond_start"] + ["spmv", "dot", "calc_xr_precond", "calc_p_precond"] * it
# the scalars: alpha = rz / pw and beta = rz_new / rz, replayed from the operations themselves
t = PSingle(A)
vb, vx, vr, vp, vw, vd = V(b.copy()), V(np.zeros(n)), V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(dinv)
rz, rr1 = t.precond_start(vr, vd, vp)
for i in range(it):
    t.spmv(None, vp, vw)
    alpha = fdiv(rz, t.dot(vp, vw))
    assert s.calls[2 + 4 * i + 2] == ("calc_xr_precond", alpha), i
    rz_new, rr1 = t.calc_xr_precond(vx, vr, vp, vw, vd, alpha)
    assert s.calls[2 + 4 * i + 3] == ("calc_p_precond", fdiv(rz_new, rz)), i
    assert h[i] == rr1          # on_iteration and the stop test see r.r, not r.z
    t.calc_p_precond(vp, vr, vd, fdiv(rz_new, rz))
    rz = rz_new
assert np.array_equal(vx.a, x)
# identity preconditioner: every number of the plain loop, bit for bit
it0, rr0, x0, h0, _, _ = single(A, b, 1000, 1e-20)
it1, rr1, x1, h1, _, _ = psingle(A, b, 1000, 1e-20, np.ones(n))
assert (it1, rr1, h1) == (it0, rr0, h0) and np.array_equal(x1, x0)
# block: the same per column, one call each per iteration
B = np.stack([b, 2 * b[::-1], b * b], axis=1)
itrs, rrb, X, hist, checks, sb = pblock(A, B, 1000, 1e-20, dinv)
assert names(sb.calls) == ["copy", "precond_start"] + ["spmv", "dot", "calc_xr_precond", "calc_p_precond"] * len(hist)
assert sb.calls[1] == ("precond_start", 7)
for j in range(3):
    itj, rrj, xj, hj, _, _ = psingle(A, B[:, j], 1000, 1e-20, dinv)
    assert itj == itrs[j] and rrj == rrb[j] and np.array_equal(xj, X[:, j]), j
print("ok")
''')
    assert out.strip() == "ok"


def test_failed_check_is_followed_by_restart_then_precond_start():
    out = child(STANDIN + r'''
it0, rr0, x0, h0, _, s0 = psingle(A, b, 1000, 1e-20, dinv, check_every=5)
assert names(s0.calls).count("precond_start") == 1 and "restart" not in names(s0.calls)
i = int(np.argmax(np.abs(x0)))
it, rr, x, h, checks, s = psingle(A, b, 1000, 1e-20, dinv, check_every=5, flips=[(7, "x", i, [55])])
fails = [c for c in checks if not c[2]]
assert [(c[0], c[3]) for c in fails] == [(9, 4)], checks
nm = names(s.calls)
at = nm.index("restart")
assert nm[at - 2:at + 2] == ["gap", "copy", "restart", "precond_start"], nm[at - 3:at + 3]
assert nm.count("restart") == 1 and nm.count("precond_start") == 2
assert h[:10] == h0[:10] and it > it0 and true_res(A, b, x) <= 10 * true_res(A, b, x0)
# block: only the failed column is restarted and re-preconditioned
k = 3
B = np.stack([b, 2 * b[::-1], np.sin(np.arange(n)) + 2.0], axis=1)
itrs0, rrb0, X0, hist0, _, _ = pblock(A, B, 1000, 1e-20, dinv, check_every=5)
itrs, rrb, X, hist, checks, sb = pblock(A, B, 1000, 1e-20, dinv, check_every=5, flips=[(7, "x", 17 * k + 1, [55])])
fails = [c for c in checks if not c[2]]
assert [(c[0], c[3], c[4]) for c in fails] == [(9, 4, 1)], fails
at = sb.calls.index(("restart", 2))
assert sb.calls[at - 1] == ("copy_block", 2) and sb.calls[at + 1] == ("precond_start", 2), sb.calls[at - 2:at + 3]
assert [c for c in sb.calls if c[0] == "precond_start"] == [("precond_start", 7), ("precond_start", 2)]
for j in (0, 2):
    assert itrs[j] == itrs0[j] and rrb[j] == rrb0[j] and np.array_equal(X[:, j], X0[:, j]), j
assert itrs[1] > itrs0[1]
assert true_res(A, B[:, 1], X[:, 1]) <= 10 * true_res(A, B[:, 1], X0[:, 1])
print("ok")
''')
    assert out.strip() == "ok"


def test_jacobi_solves_the_badly_scaled_laplacian_that_plain_cg_does_not():
    """laplace5:40,40 scaled S A S, the reference's b, threshold 1e-3, 1000 iterations at most: the stand-in
    PCG converges, the stand-in plain CG does not."""
    out = child(STANDIN + r'''
import sys
sys.path.insert(0, "tests")
from _oracle import laplace5
from _precond import scaled, diagonal
from abft_sparse_cg_amd import generators
cols, rows, vals, n = scaled(*laplace5(40, 40))
A = np.zeros((n, n))
A[rows, cols] = vals
b = generators.reference_rhs(n)
dinv = 1.0 / diagonal(cols, rows, vals, n)
assert np.array_equal(dinv, 1.0 / np.diag(A)) and dinv.max() / dinv.min() == 2.0 ** 24
it, rr, x, h, _, _ = psingle(A, b, 1000, 1e-3, dinv)
print("pcg", it, rr)
assert it < 1000 and rr <= 1e-3 and true_res(A, b, x) <= 1e-3 ** 0.5 + 1e-7 * np.linalg.norm(b)
it0, rr0, x0, h0, _, _ = psingle(A, b, 1000, 1e-3, None)
print("cg", it0, rr0)
assert it0 == 1000 and rr0 > 1e-3
print("ok")
''')
    assert out.strip().endswith("ok"), out
