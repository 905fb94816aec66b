"""CPU-side checks of the device-resident loop on protected vectors (abft_hip_calc_r_vecc, abft_hip_calc_px_vecc,
abft_hip_cg_vecc_iteration_until_dev, cg_solve_device(vector_ecc=True)): the header declares
the three entries and the built library exports them; the numpy model of the two-kernel tail and of the guarded
iteration (tests/_devloop_vecc.py) is held word for word against the model of the calls it replaces
(tests/_vecc.py); and the control flow of cg_solve_device with the flag -- the start, the batches, the two scrubs
at the end, the refusals, and today's calls with the flag off -- runs on the stand-in context of
test_device_loop_host.py, extended by the protected calls.

As there, whatever loads the package runs in a child interpreter."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _devloop_vecc as M  # noqa: E402
import _vecc  # noqa: E402
from test_device_loop_host import STANDIN as BASE, child  # noqa: E402

U = np.uint64
NEW = ["abft_hip_calc_r_vecc", "abft_hip_calc_px_vecc", "abft_hip_cg_vecc_iteration_until_dev"]


def test_header_declares_the_three_entries():
    from test_capi_symbols import declared_symbols
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s


def test_library_exports_the_three_entries():
    out = child("""
import ctypes
from abft_sparse_cg_amd import capi
lib = ctypes.CDLL(capi.LIB_PATH)
missing = [s for s in %r if not hasattr(lib, s) or s not in capi.SIGNATURES]
assert not missing, missing
import abft_sparse_cg_amd as amd
for m in ("calc_r_vecc", "calc_px_vecc", "cg_vecc_iteration_until_dev"):
    assert callable(getattr(amd.HIPContext, m)), m
import inspect
assert inspect.signature(amd.cg_solve_device).parameters["vector_ecc"].default is False
print("ok")
""" % (NEW,))
    assert out.strip() == "ok"


# ---- the model of the two-kernel tail against the model of calc_xr + calc_p ----

def same_sum(a, b):
    return (np.isnan(a) and np.isnan(b)) or np.float64(a).view(U) == np.float64(b).view(U)


def operands(name, n):
    return [_vecc.family(name, n, _vecc.operand_seed(n, k)) for k in range(4)]


@pytest.mark.parametrize("name", sorted(_vecc.FAMILIES))
@pytest.mark.parametrize("n", [1, 2, 255, 1025])
def test_model_of_the_tail_is_calc_xr_and_calc_p_word_for_word(name, n):
    xw, rw, pw, ww = operands(name, n)
    for alpha in (0.37251, -1.0, 0.0, 1e308):
        beta = -alpha / 3
        xs, rs, rr = _vecc.calc_xr(xw, rw, pw, ww, alpha)
        ps = _vecc.calc_p(pw, rs, beta)
        r2, rr2 = M.calc_r(rw, ww, alpha)
        x2, p2 = M.calc_px(xw, pw, r2, alpha, beta)
        _vecc.assert_words(r2, rs, "r")
        _vecc.assert_words(x2, xs, "x")
        _vecc.assert_words(p2, ps, "p")
        assert np.array_equal(r2, rs) and np.array_equal(x2, xs) and np.array_equal(p2, ps)  # one model: NaNs too
        assert same_sum(rr2, rr), (rr2, rr)


@pytest.mark.parametrize("op", range(4))
def test_model_of_the_tail_repairs_a_flipped_word_as_calc_xr_and_calc_p_do(op):
    n = 257
    clean = operands("finite", n)
    xs, rs, rr = _vecc.calc_xr(*clean, 0.71)
    ps = _vecc.calc_p(clean[2], rs, 0.125)
    for index, bit in ((0, 0), (128, 3), (n - 1, 55)):
        v = list(clean)
        v[op] = M.flipped(v[op], index, [bit])
        xw, rw, pw, ww = v
        r2, rr2 = M.calc_r(rw, ww, 0.71)
        x2, p2 = M.calc_px(xw, pw, r2, 0.71, 0.125)
        assert np.array_equal(r2, rs) and np.array_equal(x2, xs) and np.array_equal(p2, ps), (index, bit)
        assert same_sum(rr2, rr)


def small_csr(n=60):
    rng = np.random.default_rng(5)
    ent = sorted({(i, i) for i in range(n)} | {(int(i), int(j)) for i, j in rng.integers(0, n, (3 * n, 2))})
    rows, cols = np.array([e[0] for e in ent]), np.array([e[1] for e in ent])
    return _vecc.csr_of(cols, rows, rng.standard_normal(len(ent)), n), n


def test_model_of_the_guarded_iteration():
    csr, n = small_csr()
    rng = np.random.default_rng(6)
    xw, rw, pw = (_vecc.encode(rng.standard_normal(n)) for _ in range(3))
    rr = _vecc.dot(rw, rw)
    live = M.iteration(csr, xw, rw, pw, rr, 0.5 * rr)
    assert live["live"]
    ww, fused = _vecc.spmv(*csr, pw)
    alpha = M.fdiv(rr, fused)
    xs, rs, rr_new = _vecc.calc_xr(xw, rw, pw, ww, alpha)
    assert np.array_equal(live["w"], ww) and np.array_equal(live["r"], rs) and np.array_equal(live["x"], xs)
    assert np.array_equal(live["p"], _vecc.calc_p(pw, rs, M.fdiv(rr_new, rr)))
    assert same_sum(live["pw"], fused) and same_sum(live["rr_new"], rr_new)
    # the device's sums instead of the model's: every word follows them
    other = M.iteration(csr, xw, rw, pw, rr, 0.0, p_dot_w=fused * (1 + 2.0 ** -40), rr_new=rr_new * (1 - 2.0 ** -40))
    assert not np.array_equal(other["r"], live["r"]) and not np.array_equal(other["p"], live["p"])
    # a flip in any operand: the words of the clean iteration
    for name, at in (("x", 0), ("r", 17), ("p", n - 1)):
        v = dict(x=xw, r=rw, p=pw)
        v[name] = M.flipped(v[name], at, [44])
        hit = M.iteration(csr, v["x"], v["r"], v["p"], rr, 0.0)
        assert all(np.array_equal(hit[k], live[k]) for k in "xrpw"), name
    # frozen: at the threshold, above it, a NaN -- every word kept (a flipped one included), the bits handed on
    nan = np.array([0x7FF8000000ABCDEF], U).view(np.float64)[0]
    bad = M.flipped(rw, 3, [9])
    for cur, thr in ((rr, rr), (rr, np.inf), (nan, 0.0)):
        f = M.iteration(csr, xw, bad, pw, cur, thr)
        assert not f["live"] and f["x"] is xw and f["r"] is bad and f["p"] is pw and f["w"] is None
        assert np.float64(f["rr_new"]).view(U) == np.float64(cur).view(U)
    assert M.OPERAND == {"vec": 0, "x": 1, "r": 2, "p": 3, "w": 4}


# ---- cg_solve_device(vector_ecc=True) on the stand-in ----
# The stand-in's vectors hold plain doubles (encode and scrub only leave their names in the call list): what is
# checked here is who is called when, and that the loop is cg_solve(vector_ecc=True)'s, bit for bit, on it.
STANDIN = BASE + r'''
from abft_sparse_cg_amd.capi import FMT_CSR, FMT_COO

class Mat:
    def __init__(self, fmt=FMT_CSR, layout="stream"):
        self.fmt, self.layout = fmt, layout

class VSingle(DSingle):
    def vecc_supported(self, mat):
        return mat.fmt == FMT_CSR and mat.layout == "stream"
    def matrix_info(self, mat):
        return (mat.layout,)
    def encode_vector(self, v):
        self.calls.append(("encode",))
    def scrub_vector(self, v):
        self.calls.append(("scrub",)); return 0, 0
    def dot_vecc(self, a, b):
        self.calls.append(("dot_vecc",)); return float(np.sum(a.a * b.a))
    def spmv_vecc(self, A, x, y):
        self.calls.append(("spmv_vecc",)); y.a[:] = self.A @ x.a
    def calc_xr_vecc(self, x, r, p, w, alpha):
        self.calls.append(("calc_xr_vecc", alpha))
        x.a[:] = x.a + alpha * p.a; r.a[:] = r.a - alpha * w.a
        return float(np.sum(r.a * r.a))
    def calc_p_vecc(self, p, r, beta):
        self.calls.append(("calc_p_vecc", beta)); p.a[:] = r.a + beta * p.a
    def cg_iteration_until_dev(self, *a):
        self.calls.append(("until",)); super().cg_iteration_until_dev(*a)
    def cg_vecc_iteration_until_dev(self, *a):
        self.calls.append(("vecc_until",)); super().cg_iteration_until_dev(*a)

def run(A, b, max_itrs, conv, stride=16, graph=True, mat=None, host=False, **kw):
    s = VSingle(A)
    n = len(b)
    vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
    hist = []
    if host:
        it, rr = cg_solve(s, mat or Mat(), vb, vx, vr, vp, vw, max_itrs, conv, on_iteration=lambda i, v: hist.append(v), **kw)
    else:
        it, rr = cg_solve_device(s, mat or Mat(), vb, vx, vr, vp, vw, max_itrs, conv,
                                 on_iteration=lambda i, v: hist.append(v), stride=stride, graph=graph, **kw)
    return it, rr, vx.a, hist, s

def kinds(s):
    return [c[0] for c in s.calls]
'''


def test_protected_device_loop_makes_the_expected_calls():
    out = child(STANDIN + r'''
START, END = ["encode", "encode", "copy", "scrub", "copy", "dot_vecc"], ["scrub", "scrub"]
it0, rr0, x0, h0, s0 = run(A, b, 1000, 1e-20, host=True, vector_ecc=True)
assert kinds(s0)[:6] == START and kinds(s0)[-2:] == END and 23 < it0 < 1000
for stride in (1, 3, 16):
    for graph in (True, False):
        for max_itrs in (1000, 23, it0):
            want = min(it0, max_itrs)
            it, rr, x, h, s = run(A, b, max_itrs, 1e-20, stride, graph, vector_ecc=True)
            assert it == want == len(h) == s.live, (stride, graph, it, want)
            assert np.array_equal(bits(h), bits(h0[:want])) and bits([rr])[0] == bits(h0[want - 1:want])[0]
            if max_itrs >= it0:
                assert np.array_equal(bits(x), bits(x0))
            k = kinds(s)
            assert k[:6] == START and k[-2:] == END, k
            assert k[-5:-2] == ["destroy"] * 3  # the trail and its two views
            body = k[6:-5]
            # batches: the copy of the last pair to the first, then the guarded protected iterations -- a replayed
            # graph leaves its calls in the list once, when it is captured
            assert set(body) == {"copy", "vecc_until"} and body[0] == "copy", body
            assert "until" not in k and "dot" not in k and "spmv_vecc" not in k
            looks = -(-want // stride) + (1 if want % stride == 0 and want < max_itrs else 0)
            assert s.downloads == looks, (stride, graph, s.downloads, looks)
            if not graph:
                assert body.count("vecc_until") == s.live + s.frozen and body.count("copy") == looks
# nothing to do: the start, then the two scrubs, nothing enqueued and nothing downloaded
for kw in (dict(b=np.zeros(n), max_itrs=1000), dict(b=b, max_itrs=0)):
    it, rr, x, h, s = run(A, kw["b"], kw["max_itrs"], 1e-3, 3, vector_ecc=True)
    assert (it, h, s.downloads, s.live, s.frozen) == (0, [], 0, 0, 0)
    assert kinds(s) == START + END, kinds(s)
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_protected_device_loop_refuses_precond_and_other_layouts_before_anything_runs():
    out = child(STANDIN + r'''
cases = [(dict(precond=V(np.ones(n))), None, "precond"), ({}, Mat(FMT_COO), "COO"), ({}, Mat(FMT_CSR, "panels"), "panels"),
         ({}, Mat(FMT_CSR, "sweep"), "sweep")]
for kw, mat, text in cases:
    s = VSingle(A)
    vs = [V(b.copy())] + [V(np.zeros(n)) for _ in range(4)]
    try:
        cg_solve_device(s, mat or Mat(), *vs, 1000, 1e-3, vector_ecc=True, **kw)
    except ValueError as e:
        assert text in str(e), (text, str(e))
    else:
        raise AssertionError(text)
    assert s.calls == [] and s.downloads == 0
    assert np.array_equal(vs[0].a, b) and not any(v.a.any() for v in vs[1:])
# a stride that is no whole number is refused first, as without the flag
try:
    run(A, b, 10, 1e-3, 2.5, vector_ecc=True)
except ValueError:
    pass
else:
    raise AssertionError("stride")
print("ok")
''')
    assert out.strip() == "ok", out


def test_flag_off_makes_todays_calls():
    out = child(STANDIN + r'''
def todays(A, b, max_itrs, conv, stride, graph):
    # the plain device loop as it stood before the flag (context.cg_solve_device)
    s = VSingle(A)
    n = len(b)
    vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
    s.copy_vector(vr, vb); s.copy_vector(vp, vr)
    rr = s.dot(vr, vr)
    if max_itrs == 0 or not rr > conv:
        return s
    done = 0
    trail = s.create_vector(2 * (stride + 1) + 2)
    first, last = s.view_vector(trail, 0, 2), s.view_vector(trail, 2 * stride, 2)
    trail.a[2 * stride] = rr
    g = None
    while True:
        m = min(stride, max_itrs - done)
        def batch():
            s.copy_vector(first, last)
            for k in range(m):
                s.cg_iteration_until_dev(None, vp, vx, vr, vp, vw, trail, 2 * k, 2 * (stride + 1), 2 * k + 2, conv)
        if graph and m == stride:
            if g is None:
                s.graph_begin(); batch(); g = s.graph_end()
            s.graph_launch(g)
        else:
            batch()
        t = s.download(trail)
        live = next((k for k in range(m) if not t[2 * k] > conv), m)
        done += live
        if live < m or done >= max_itrs:
            for v in (first, last, trail):
                s.destroy_vector(v)
            return s

for bb, max_itrs, conv in ((b, 1000, 1e-20), (b, 23, 1e-20), (b, 1000, 1e-3), (b, 0, 1e-3), (np.zeros(n), 1000, 1e-3)):
    for stride in (1, 3, 16):
        for graph in (True, False):
            want = todays(A, bb, max_itrs, conv, stride, graph)
            for kw in ({}, dict(vector_ecc=False)):
                it, rr, x, h, s = run(A, bb, max_itrs, conv, stride, graph, **kw)
                assert s.calls == want.calls, (stride, graph, kw, kinds(s), kinds(want))
                assert (s.downloads, s.live, s.frozen, s.launches, s.eager) == \
                    (want.downloads, want.live, want.frozen, want.launches, want.eager), (stride, graph)
                assert not {"encode", "scrub", "dot_vecc", "vecc_until"} & set(kinds(s))
it, rr, x, h, s = run(A, np.zeros(n), 1000, 1e-3, 3)
assert kinds(s) == ["copy", "copy", "dot"]
print("ok")
''')
    assert out.strip().endswith("ok"), out
