"""CPU-side checks of the device-resident block loop (abft_hip_cg_block_iteration_until_dev,
abft_hip_block_loop_reserve, cg_solve_block_device): the header declares the two entries and
the built library exports them, and the control flow of cg_solve_block_device -- the trail of (2K + 2)-double
records, the batches, when the host looks, what on_iteration gets -- against cg_solve_block(fused=True) on the
recording numpy stand-in of test_block_fused_host.py, extended by views, a graph that records calls and replays
them, and the guarded block iteration (its mask formed from the record, frozen words moved as uint64).

As there, whatever loads the package runs in a child interpreter."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_block_fused_host import STANDIN as BASE, child  # noqa: E402

NEW = ["abft_hip_cg_block_iteration_until_dev", "abft_hip_block_loop_reserve"]


def test_header_declares_the_block_loop_entries():
    from test_capi_symbols import declared_symbols
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s


def test_library_exports_the_block_loop_entries():
    out = child("""
import ctypes
from abft_sparse_cg_amd import capi
lib = ctypes.CDLL(capi.LIB_PATH)
missing = [s for s in %r if not hasattr(lib, s) or s not in capi.SIGNATURES]
assert not missing, missing
import abft_sparse_cg_amd as amd
assert callable(amd.cg_solve_block_device)
assert callable(amd.HIPContext.cg_block_iteration_until_dev) and callable(amd.HIPContext.block_loop_reserve)
assert len(capi.SIGNATURES["abft_hip_cg_block_iteration_until_dev"][1]) == 12
assert len(capi.SIGNATURES["abft_hip_block_loop_reserve"][1]) == 3
print("ok")
""" % (NEW,))
    assert out.strip() == "ok"


# Rec with views, a download that counts, a graph (calls made between graph_begin and graph_end are recorded, not
# run) and the guarded block iteration: the numpy operations of Rec's spmm_dot, calc_r_block and calc_px_block behind
# the per-column stop test, the scalars in records of a vector
STANDIN = BASE + r'''
from abft_sparse_cg_amd.context import cg_solve_block_device, fdiv

class DRec(Rec):
    def __init__(self, A):
        super().__init__(A)
        self.rec, self.downloads, self.live, self.frozen, self.launches, self.eager = None, 0, 0, 0, 0, 0
        self.reserved = 0
    def do(self, f):
        if self.rec is not None:
            self.rec.append(f)
        else:
            f()
    def create_vector(self, n):
        return V(np.zeros(n))
    def view_vector(self, parent, off, n):
        return V(parent.a[off:off + n])
    def destroy_vector(self, v):
        self.calls.append(("destroy",))
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
    def block_loop_reserve(self, A, k):
        assert self.rec is None          # eager only
        self.calls.append(("reserve", k)); self.reserved += 1
    def cg_block_iteration_until_dev(self, A, X, R, P, W, k, sc, in_at, pw_at, out_at, thr, dinv=None):
        self.calls.append(("block_until", in_at, pw_at, out_at, dinv is not None))
        if self.rec is None:
            self.eager += 1
        else:
            assert self.reserved         # reserved before the first capture
        def f():
            u = sc.a.view(np.uint64)
            rec = 2 * k + 2
            active = sum(1 << j for j in range(k) if sc.a[in_at + j] > thr)
            self._mm(P, W, k)            # the SpMM always runs
            pw = sums(P, W, k)
            sc.a[pw_at:pw_at + k] = pw; sc.a[pw_at + k] = 0.0
            if not active:
                u[out_at:out_at + 2 * k] = u[in_at:in_at + 2 * k]
                sc.a[out_at + 2 * k:out_at + rec] = 0.0
                self.frozen += 1
                return
            self.live += 1
            on = [(active >> j) & 1 for j in range(k)]
            num = sc.a[in_at + k:in_at + 2 * k].copy()
            alpha = [fdiv(num[j], pw[j]) if on[j] else 0.0 for j in range(k)]
            got = self._r(R, W, k, alpha, active, dinv)
            rz_new, rr_new = (got, got) if dinv is None else got
            beta = [fdiv(rz_new[j], num[j]) if on[j] else 0.0 for j in range(k)]
            self._x(X, P, k, alpha, active); self._p(P, R, k, beta, active, dinv)
            new = np.concatenate([rr_new, rz_new]).view(np.uint64)
            old = u[in_at:in_at + 2 * k].copy()
            keep = np.array(on + on, dtype=bool)
            u[out_at:out_at + 2 * k] = np.where(keep, new, old)   # frozen words: moved as integers
            sc.a[out_at + 2 * k:out_at + rec] = 0.0
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

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)

def vecs(B):
    n, k = B.shape
    return [V(B.copy(), k)] + [V(np.zeros((n, k)), k) for _ in range(4)]

def dinv_of(A, pre):
    return V(1.0 / np.diag(A).copy()) if pre else None

def host(A, B, pre, max_itrs, conv):
    s = Rec(A)
    v = vecs(B)
    s.x = v[1]
    hist = []
    itrs, rr = cg_solve_block(s, None, *v, max_itrs, conv, on_iteration=lambda i, r, a: hist.append((i, r, a)),
                              precond=dinv_of(A, pre), fused=True)
    return list(itrs), rr, v[1].a, hist

def device(A, B, pre, max_itrs, conv, stride, graph=True):
    s = DRec(A)
    v = vecs(B)
    s.x = v[1]
    hist = []
    def cb(i, r, a):
        assert s.rec is None
        hist.append((i, r, a, s.downloads))
    itrs, rr = cg_solve_block_device(s, None, *v, max_itrs, conv, on_iteration=cb, stride=stride, graph=graph,
                                     precond=dinv_of(A, pre))
    return list(itrs), rr, v[1].a, hist, s

def compare(A, B, pre, max_itrs, conv):
    """every stride, graph on and off, against cg_solve_block(fused=True) on the same stand-in -> the counts"""
    k = B.shape[1]
    it0, rr0, x0, h0 = host(A, B, pre, max_itrs, conv)
    T = len(h0)
    assert T == max(it0)
    for stride in (1, 5, 16):
        for graph in (True, False):
            it, rr, x, h, s = device(A, B, pre, max_itrs, conv, stride, graph)
            assert it == it0, (stride, it, it0)
            assert np.array_equal(bits(rr), bits(rr0)) and np.array_equal(bits(x), bits(x0)), stride
            # the callback triples (itr, rr, active), in order ...
            assert [(i, a) for i, _, a, _ in h] == [(i, a) for i, _, a in h0], stride
            assert all(np.array_equal(bits(r), bits(r0)) for (_, r, _, _), (_, r0, _) in zip(h, h0)), stride
            # ... and after their batch: iteration i is reported once download i // stride + 1 has been made
            assert all(d == i // stride + 1 for i, _, _, d in h), (stride, h)
            assert s.live == T
            # one look per batch: ceil(T / stride), plus one batch of frozen iterations when the loop stops on a
            # batch's last iteration with iterations to spare (the host reads record i only for i < m)
            want = 0 if T == 0 else -(-T // stride) + (1 if T % stride == 0 and T < max_itrs else 0)
            assert s.downloads == want, (stride, graph, T, s.downloads, want)
            # the trail: record i at (2k + 2) i, P.W behind the stride + 1 records
            rec = 2 * k + 2
            for c in s.calls:
                if c[0] == "block_until":
                    assert c[1] % rec == 0 and c[3] == c[1] + rec and c[2] == rec * (stride + 1) and c[1] < rec * stride, c
                    assert c[4] == pre
            names = [c[0] for c in s.calls]
            assert names[:3 - pre] == (["copy", "precond_start"] if pre else ["copy", "copy", "dot_block"])
            assert not set(names) & {"spmm", "spmm_dot", "calc_r", "calc_px", "calc_xr", "calc_p"}
            assert names.count("dot_block") == (0 if pre else 1)
            if T == 0:
                assert len(names) == 3 - pre and s.frozen == 0      # nothing more enqueued
            if not graph:
                assert s.launches == 0 and s.reserved == 0
            elif T:
                full = sum(1 for d in range(want) if min(stride, max_itrs - d * stride) == stride)
                assert s.launches == full, (stride, s.launches, full)           # a short last batch is enqueued eagerly
                assert s.eager == ((max_itrs - full * stride) if want > full else 0), (stride, s.eager)
                assert s.reserved == (1 if full else 0)
    return it0

# a system that needs more than 23 iterations with and without Jacobi: the badly scaled 9 x 7 Laplacian of
# test_device_loop_precond_host.py, four right-hand sides of very different size
import os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from _oracle import laplace5
from _precond import scaled

def dense(cols, rows, vals, n):
    M = np.zeros((n, n))
    np.add.at(M, (rows.astype(np.int64), cols.astype(np.int64)), vals)
    return M

sys_ = scaled(*laplace5(9, 7))
PA = dense(*sys_)
PB = (np.random.default_rng(4).random((sys_[3], 4)) + 0.5) * np.array([1e-3, 1.0, 30.0, 5.0])
'''


def test_block_device_loop_is_the_fused_block_loop_on_the_standin():
    out = child(STANDIN + r'''
for pre in (False, True):
    need = compare(PA, PB, pre, 1000, 1e-20)
    print("precond", pre, "iterations needed per column", need)
    assert 23 < max(need) < 1000 and len(set(need)) >= 3       # columns stop at different iterations
    assert compare(PA, PB, pre, 23, 1e-20) == [23] * 4          # stops at max_itrs: no look beyond it
    assert compare(PA, PB, pre, max(need), 1e-20) == need       # converges on the very last iteration allowed
    it3 = compare(PA, PB, pre, 1000, 1e-3)
    assert it3[0] == 0 and min(it3[1:]) > 3                     # column 0 frozen from the start
    assert compare(PA, PB, pre, 0, 1e-20) == [0] * 4
    assert compare(PA, np.zeros_like(PB), pre, 1000, 1e-3) == [0] * 4   # B = 0: nothing enqueued
    it, rr, x, h, s = device(PA, np.zeros_like(PB), pre, 1000, 1e-3, 5)
    assert (it, list(rr), h, s.downloads, s.live, s.frozen) == ([0] * 4, [0.0] * 4, [], 0, 0, 0)
    assert len(compare(PA, PB[:, 1:2].copy(), pre, 1000, 1e-10)) == 1   # K = 1
    assert len(set(compare(A, B, pre, 1000, 1e-10))) >= 3       # test_block_fused_host.py's system
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_a_column_frozen_from_the_start_and_the_call_list():
    """column 0 below the threshold from the start while the others run; the call list of one solve written out"""
    out = child(STANDIN + r'''
B2 = B.copy(); B2[:, 0] *= 1e-9
it0, rr0, x0, h0 = host(A, B2, False, 7, 1e-10)
assert it0[0] == 0 and it0[1:] == [7, 7, 7] and all(a == 0b1110 for _, _, a in h0)
it, rr, x, h, s = device(A, B2, False, 7, 1e-10, 3, graph=False)
assert it == it0 and np.array_equal(bits(x), bits(x0)) and not x[:, 0].any()
want = [("copy",), ("copy",), ("dot_block",)]
for m in (3, 3, 1):
    want += [("copy",)] + [("block_until", 10 * i, 40, 10 * i + 10, False) for i in range(m)]
want += [("destroy",)] * 3                                   # the two views and the trail
assert s.calls == want, s.calls
for stride in (0, -1, 2.5):
    try:
        device(A, B, False, 10, 1e-3, stride)
    except ValueError:
        pass
    else:
        raise AssertionError(stride)
print("ok")
''')
    assert out.strip().endswith("ok"), out
