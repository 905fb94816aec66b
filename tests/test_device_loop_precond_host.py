"""CPU-side checks of the device-scalar loop with Jacobi preconditioning (abft_hip_pcg_iteration_until_dev,
cg_solve_device(precond=)): the header declares the entry and the built library exports it,
and the control flow of cg_solve_device(precond=dinv) -- the trail of four-double records, the batches, when the
host looks, what on_iteration gets -- against cg_solve(precond=dinv) on the numpy stand-in context of
test_device_loop_host.py, extended by the preconditioned calls.  With precond=None the calls are the ones made
before the argument existed.

As there, whatever loads the package runs in a child interpreter."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_device_loop_host import STANDIN as BASE  # noqa: E402
from test_residual_check_host import child  # noqa: E402

NEW = ["abft_hip_pcg_iteration_until_dev"]


def test_header_declares_the_preconditioned_guarded_iteration():
    from test_capi_symbols import declared_symbols
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s


def test_library_exports_the_preconditioned_guarded_iteration():
    out = child("""
import ctypes
from abft_sparse_cg_amd import capi
lib = ctypes.CDLL(capi.LIB_PATH)
missing = [s for s in %r if not hasattr(lib, s) or s not in capi.SIGNATURES]
assert not missing, missing
import abft_sparse_cg_amd as amd
assert callable(amd.HIPContext.pcg_iteration_until_dev)
assert len(capi.SIGNATURES["abft_hip_pcg_iteration_until_dev"][1]) == 14
print("ok")
""" % (NEW,))
    assert out.strip() == "ok"


# the stand-in of test_device_loop_host.py with the preconditioned calls: precond_start, calc_xr_precond and
# calc_p_precond as cg_solve(precond=) makes them, and the guarded preconditioned iteration -- the same numpy
# operations behind the stop test, the scalars in records {r.r, events, r.z, 0.0} of a vector
STANDIN = BASE + r'''
import os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from _oracle import laplace5
from _precond import scaled, diagonal

class PSingle(DSingle):
    def precond_start(self, r, dinv, p):
        self.calls.append(("precond_start",))
        z = dinv.a * r.a
        p.a[:] = z
        return float(np.sum(r.a * z)), float(np.sum(r.a * r.a))
    def calc_xr_precond(self, x, r, p, w, dinv, alpha):
        self.calls.append(("calc_xr_precond", alpha))
        x.a[:] = x.a + alpha * p.a; r.a[:] = r.a - alpha * w.a
        z = dinv.a * r.a
        return float(np.sum(r.a * z)), float(np.sum(r.a * r.a))
    def calc_p_precond(self, p, r, dinv, beta):
        self.calls.append(("calc_p_precond", beta)); p.a[:] = dinv.a * r.a + beta * p.a
    def pcg_iteration_until_dev(self, A, vec, x, r, p, w, dinv, sc, in_at, pw_at, out_at, thr):
        assert vec is p
        self.calls.append(("pcg_until", in_at, pw_at, out_at))
        if self.rec is None:
            self.eager += 1
        def f():
            u = sc.a.view(np.uint64)
            rr = float(sc.a[in_at])
            if not (rr > thr):
                u[out_at], u[out_at + 2] = u[in_at], u[in_at + 2]
                sc.a[out_at + 1], sc.a[out_at + 3] = 0.0, 0.0
                self.frozen += 1
                return
            self.live += 1
            rz = float(sc.a[in_at + 2])
            w.a[:] = self.A @ vec.a
            pw = float(np.sum(vec.a * w.a))
            sc.a[pw_at] = pw
            alpha = fdiv(rz, pw)
            x.a[:] = x.a + alpha * p.a; r.a[:] = r.a - alpha * w.a
            z = dinv.a * r.a
            rz_new, rr_new = float(np.sum(r.a * z)), float(np.sum(r.a * r.a))
            sc.a[out_at:out_at + 4] = (rr_new, 0.0, rz_new, 0.0)
            p.a[:] = z + fdiv(rz_new, rz) * p.a
        self.do(f)

def dense(cols, rows, vals, n):
    M = np.zeros((n, n))
    np.add.at(M, (rows.astype(np.int64), cols.astype(np.int64)), vals)
    return M

sys_ = scaled(*laplace5(9, 7))
PA = dense(*sys_)
pn = sys_[3]
pdinv = 1.0 / diagonal(*sys_)
pb = np.random.default_rng(4).random(pn) + 0.5
assert pdinv.max() / pdinv.min() > 1e5        # far from the identity

def phost(A, b, dinv, max_itrs, conv):
    return single(A, b, max_itrs, conv, cls=PSingle, precond=V(dinv.copy()))

def pdevice(A, b, dinv, max_itrs, conv, stride, graph=True):
    s = PSingle(A)
    n = len(b)
    vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
    hist = []
    def cb(i, v):
        assert s.rec is None
        hist.append((i, v, s.downloads))
    it, rr = cg_solve_device(s, None, vb, vx, vr, vp, vw, max_itrs, conv, on_iteration=cb, stride=stride, graph=graph,
                             precond=V(dinv.copy()))
    return it, rr, vx.a, hist, s

def pcompare(A, b, dinv, max_itrs, conv):
    it0, rr0, x0, h0, _, _ = phost(A, b, dinv, max_itrs, conv)
    for stride in (1, 5, 16):
        for graph in (True, False):
            it, rr, x, h, s = pdevice(A, b, dinv, max_itrs, conv, stride, graph)
            assert it == it0 and np.array_equal(bits([rr]), bits([rr0])), (stride, it, it0, rr, rr0)
            assert [i for i, _, _ in h] == list(range(it0)), (stride, h)      # the callbacks, in order
            assert np.array_equal(bits([v for _, v, _ in h]), bits(h0)), stride
            assert np.array_equal(bits(x), bits(x0)), stride
            # ... and after their batch: iteration i is reported once download i // stride + 1 has been made
            assert all(d == i // stride + 1 for i, _, d in h), (stride, h)
            assert s.live == it0
            want = 0 if it0 == 0 else -(-it0 // stride) + (1 if it0 % stride == 0 and it0 < max_itrs else 0)
            assert s.downloads == want, (stride, graph, it0, s.downloads, want)
            # the trail: record k at 4 k, p.w behind the stride + 1 records
            for c in s.calls:
                if c[0] == "pcg_until":
                    assert c[1] % 4 == 0 and c[3] == c[1] + 4 and c[2] == 4 * (stride + 1) and c[1] < 4 * stride, c
            assert [c[0] for c in s.calls[:2]] == ["copy", "precond_start"]
            assert not any(c[0] in ("dot", "calc_xr", "calc_p", "spmv") for c in s.calls)
            if not graph:
                assert s.launches == 0
            elif it0:
                full = sum(1 for d in range(want) if min(stride, max_itrs - d * stride) == stride)
                assert s.launches == full, (stride, s.launches, full)
                assert s.eager == ((max_itrs - full * stride) if want > full else 0), (stride, s.eager)
    return it0
'''


def test_preconditioned_device_loop_is_cg_solve_precond_on_the_standin():
    out = child(STANDIN + r'''
need = pcompare(PA, pb, pdinv, 1000, 1e-20)
plain = single(PA, pb, 1000, 1e-20)[0]
print("iterations needed", need, "plain CG", plain)
assert 23 < need < 1000
assert pcompare(PA, pb, pdinv, 23, 1e-20) == 23             # stops at max_itrs: no look beyond it
assert pcompare(PA, pb, pdinv, need, 1e-20) == need         # converges on the very last iteration allowed
assert pcompare(PA, pb, pdinv, 1000, 1e-3) > 3
assert pcompare(PA, pb, pdinv, 0, 1e-20) == 0
assert pcompare(PA, np.zeros(pn), pdinv, 1000, 1e-3) == 0   # rr0 = 0.0: nothing enqueued
it, rr, x, h, s = pdevice(PA, np.zeros(pn), pdinv, 1000, 1e-3, 5)
assert (it, rr, h, s.downloads, s.live, s.frozen) == (0, 0.0, [], 0, 0, 0)
assert [c[0] for c in s.calls] == ["copy", "precond_start"]
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_without_precond_the_calls_are_the_ones_made_before():
    """the call list of cg_solve_device without the argument, written out: two copies and a dot, then per batch one
    copy and m guarded iterations over pairs at 2 k, p.w at 2 (stride + 1)"""
    out = child(STANDIN + r'''
class Rec(DSingle):
    def cg_iteration_until_dev(self, A, vec, x, r, p, w, sc, rr_at, pw_at, new_at, thr):
        self.calls.append(("until", rr_at, pw_at, new_at, thr))
        super().cg_iteration_until_dev(A, vec, x, r, p, w, sc, rr_at, pw_at, new_at, thr)
    def pcg_iteration_until_dev(self, *a):
        raise AssertionError("preconditioned call without precond")
    precond_start = pcg_iteration_until_dev

def run(**kw):
    s = Rec(A)
    vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
    it, rr = cg_solve_device(s, None, vb, vx, vr, vp, vw, 7, 1e-20, stride=3, graph=False, **kw)
    return it, rr, s.calls, vx.a

want = [("copy",), ("copy",), ("dot",)]
for m in (3, 3, 1):
    want += [("copy",)] + [("until", 2 * k, 8, 2 * k + 2, 1e-20) for k in range(m)]
want += [("destroy",)] * 3                                   # the two views and the trail
for kw in ({}, {"precond": None}):
    it, rr, calls, x = run(**kw)
    assert it == 7 and calls == want, calls
print("ok")
''')
    assert out.strip().endswith("ok"), out
