"""CPU-side checks of the device-scalar loop with a stop test (abft_hip_cg_iteration_until_dev, cg_solve_device,
--device-loop): the header declares the entry and the built library exports it, the CLI parses the flag like
the other flags and refuses the combinations the loop does not cover, and the control flow of cg_solve_device --
batches, the trail of pairs, when the host looks, what it hands to on_iteration -- checked against a numpy
stand-in context (that of test_residual_check_host.py, extended by the guarded iteration and a graph that
records calls and replays them).

As there, whatever loads the package runs in a child interpreter."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_residual_check_host import STANDIN as BASE, child  # noqa: E402

NEW = ["abft_hip_cg_iteration_until_dev"]


def test_header_declares_the_guarded_iteration():
    from test_capi_symbols import declared_symbols
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s


def test_library_exports_the_guarded_iteration():
    out = child("""
import ctypes
from abft_sparse_cg_amd import capi
lib = ctypes.CDLL(capi.LIB_PATH)
missing = [s for s in %r if not hasattr(lib, s) or s not in capi.SIGNATURES]
assert not missing, missing
import abft_sparse_cg_amd as amd
assert callable(amd.cg_solve_device) and amd.DEFAULT_STRIDE >= 1
for m in ("cg_iteration_until_dev", "graph_begin", "graph_end", "graph_launch", "graph_destroy"):
    assert callable(getattr(amd.HIPContext, m)), m
print("ok")
""" % (NEW,))
    assert out.strip() == "ok"


def test_device_loop_flag_is_parsed_like_the_other_flags():
    out = child("""
from abft_sparse_cg_amd import cg
assert cg.parse(["cg"])["device_loop"] == 0
assert cg.parse(["cg", "--device-loop", "8"])["device_loop"] == 8
assert cg.parse(["cg", "--device-loop", "1", "--rhs", "1", "--precond", "none", "--check-every", "0",
                 "--vector-ecc", "none"])["device_loop"] == 1
bad = [["--device-loop"], ["--device-loop", "0"], ["--device-loop", "-3"], ["--device-loop", "x"]]
combos = [["--rhs", "3"], ["--precond", "jacobi"], ["--check-every", "5"], ["--vector-ecc", "secded"],
          ["--flip-vector", "3:x:0:1"]]
for b in bad + [["--device-loop", "8"] + c for c in combos] + [c + ["--device-loop", "8"] for c in combos]:
    try:
        cg.parse(["cg"] + b)
    except SystemExit as e:
        assert e.code == 1, b
    else:
        raise AssertionError(b)
print("ok")
""")
    assert out.strip().endswith("ok")
    assert out.count("Invalid --device-loop") == 4, out
    for flag in ("--rhs", "--precond", "--check-every", "--vector-ecc", "--flip-vector"):
        assert out.count("--device-loop cannot be combined with %s" % flag) == 2, (flag, out)


# the stand-in with views, the guarded iteration (the operations of Single's spmv, dot, calc_xr and calc_p behind the
# stop test, the scalars in a vector) and a graph: calls made between graph_begin and graph_end are recorded, not run
STANDIN = BASE + r'''
from abft_sparse_cg_amd.context import cg_solve_device

class DSingle(Single):
    def __init__(self, A):
        super().__init__(A)
        self.rec, self.downloads, self.live, self.frozen, self.launches, self.eager = None, 0, 0, 0, 0, 0
    def do(self, f):
        if self.rec is not None:
            self.rec.append(f)
        else:
            f()
    def create_vector(self, n):
        return V(np.zeros(n))
    def view_vector(self, parent, off, n):
        return V(parent.a[off:off + n])
    def upload(self, v, a):
        assert self.rec is None
        v.a[:] = a
    def download(self, v):
        assert self.rec is None          # nothing that synchronises inside a capture
        self.downloads += 1
        return v.a.copy()
    def copy_vector(self, d, s):
        self.calls.append(("copy",))
        def f():
            d.a[:] = s.a
        self.do(f)
    def cg_iteration_until_dev(self, A, vec, x, r, p, w, sc, rr_at, pw_at, new_at, thr):
        assert vec is p
        if self.rec is None:
            self.eager += 1
        def f():
            rr = float(sc.a[rr_at])
            if not (rr > thr):
                sc.a.view(np.uint64)[new_at] = sc.a.view(np.uint64)[rr_at]
                sc.a[new_at + 1] = 0.0
                self.frozen += 1
                return
            self.live += 1
            w.a[:] = self.A @ vec.a
            pw = float(np.sum(vec.a * w.a))
            sc.a[pw_at] = pw
            alpha = fdiv(rr, pw)
            x.a[:] = x.a + alpha * p.a; r.a[:] = r.a - alpha * w.a
            rr_new = float(np.sum(r.a * r.a))
            sc.a[new_at], sc.a[new_at + 1] = rr_new, 0.0
            p.a[:] = r.a + fdiv(rr_new, rr) * p.a
        self.do(f)
    def graph_begin(self):
        assert self.rec is None
        self.rec = []
    def graph_end(self):
        g, self.rec = self.rec, None
        return g
    def graph_launch(self, g):
        self.launches += 1
        for f in g:
            f()
    def graph_destroy(self, g):
        del g[:]

def device(A, b, max_itrs, conv, stride, graph=True):
    s = DSingle(A)
    n = len(b)
    vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
    hist = []
    it, rr = cg_solve_device(s, None, vb, vx, vr, vp, vw, max_itrs, conv,
                             on_iteration=lambda i, v: hist.append((i, v)), stride=stride, graph=graph)
    return it, rr, vx.a, hist, s

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)

def compare(A, b, max_itrs, conv):
    """every stride, graph on and off, against cg_solve on the same stand-in -> the iteration count"""
    it0, rr0, x0, h0, _, _ = single(A, b, max_itrs, conv)
    for stride in (1, 3, 16):
        for graph in (True, False):
            it, rr, x, h, s = device(A, b, max_itrs, conv, stride, graph)
            assert it == it0 and np.array_equal(bits([rr]), bits([rr0])), (stride, it, it0, rr, rr0)
            assert [i for i, _ in h] == list(range(it0)), (stride, h)          # the callbacks, in order
            assert np.array_equal(bits([v for _, v in h]), bits(h0)), stride
            assert np.array_equal(bits(x), bits(x0)), stride
            assert s.live == it0
            # one look per batch: ceil(live / stride), plus one batch of frozen iterations when the loop stops on a
            # batch's last iteration with iterations to spare (the host reads pair k only for k < m)
            want = 0 if it0 == 0 else -(-it0 // stride) + (1 if it0 % stride == 0 and it0 < max_itrs else 0)
            assert s.downloads == want, (stride, graph, it0, s.downloads, want)
            if not graph:
                assert s.launches == 0
            elif it0:
                full = sum(1 for d in range(want) if min(stride, max_itrs - d * stride) == stride)
                assert s.launches == full, (stride, s.launches, full)           # a short last batch is enqueued eagerly
                assert s.eager == ((max_itrs - full * stride) if want > full else 0), (stride, s.eager)
    return it0
'''


def test_device_loop_is_cg_solve_bit_for_bit_on_the_standin():
    out = child(STANDIN + r'''
need = compare(A, b, 1000, 1e-20)
print("iterations needed", need)
assert 23 < need < 1000
assert compare(A, b, 23, 1e-20) == 23                   # stops at max_itrs: no look beyond it
assert compare(A, b, need, 1e-20) == need               # converges on the very last iteration allowed
assert compare(A, b, 1000, 1e-3) > 3
assert compare(A, b, 0, 1e-20) == 0
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_zero_rhs_and_nan_residuals_stop_as_the_host_loop_does():
    out = child(STANDIN + r'''
# b = 0: rr0 = 0.0 is not above the threshold; nothing is enqueued, nothing downloaded
assert compare(A, np.zeros(n), 1000, 1e-3) == 0
assert compare(A, np.zeros(n), 1000, 0.0) == 0
it, rr, x, h, s = device(A, np.zeros(n), 1000, 1e-3, 3)
assert (it, rr, h, s.downloads, s.live, s.frozen) == (0, 0.0, [], 0, 0, 0)
assert [c[0] for c in s.calls] == ["copy", "copy", "dot"]
# an rr that turns NaN: b so large that r.r overflows -- inf > threshold is live, alpha = inf / inf is NaN, the next
# rr is NaN and `rr > threshold` is false from then on
big = b * 1e160
it0, rr0, x0, h0, _, _ = single(A, big, 1000, 1e-3)
assert it0 == 1 and rr0 != rr0 and np.isinf(float(np.sum(big * big)))
assert compare(A, big, 1000, 1e-3) == 1
it, rr, x, h, s = device(A, big, 1000, 1e-3, 16)
assert s.live == 1 and s.frozen == 15 and s.downloads == 1
# a NaN in b: rr0 is NaN, no iteration at all
bad = b.copy(); bad[5] = float("nan")
assert compare(A, bad, 1000, 1e-3) == 0
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_stride_must_be_a_positive_whole_number():
    out = child(STANDIN + r'''
for stride in (0, -1, 2.5):
    try:
        device(A, b, 10, 1e-3, stride)
    except ValueError:
        pass
    else:
        raise AssertionError(stride)
print("ok")
''')
    assert out.strip() == "ok"
