"""CPU-side checks of Jacobi-preconditioned CG on protected vectors (abft_hip_precond_start_vecc,
abft_hip_calc_r_precond_vecc, abft_hip_calc_px_precond_vecc, abft_hip_pcg_vecc_iteration_until_dev,
cg_solve / cg_solve_device(vector_ecc=True, precond=ctx.jacobi(A, protected=True))):

 - the numpy model (tests/_vecc_precond.py) with dinv == 1.0 is the model of the plain protected calls (tests/_vecc.py)
   word for word, and both of its sums have the same bits;
 - the model loop converges on the badly scaled Laplacian on which the unpreconditioned protected loop does not;
 - the range over which the GPU tests compare r.r histories is fixed HERE, from two orders of the model's own sums;
 - the call sequences of the two solvers on a stand-in context, the refusals, and today's calls with the arguments off;
 - the header, capi.SIGNATURES and the built library agree on the four new symbols.

Whatever loads the package runs in a child interpreter, as in the sibling host tests."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vecc  # noqa: E402
import _vecc_precond as P  # noqa: E402
import test_device_loop_precond_host as PRECOND_HOST  # noqa: E402
import test_device_loop_vecc_host as VECC_HOST  # noqa: E402
from _oracle import rhs  # noqa: E402
from test_device_loop_host import STANDIN as BASE, child  # noqa: E402

U = np.uint64
NEW = ["abft_hip_precond_start_vecc", "abft_hip_calc_r_precond_vecc", "abft_hip_calc_px_precond_vecc",
       "abft_hip_pcg_vecc_iteration_until_dev"]

# ---- the compared range of the GPU history tests ----
# The system of the solver tests: scaled_laplace(32, 32, 6), b = rhs(1024, 1), x0 = 0.  Two runs of the model loop that
# differ only in the order of every sum's adds (serial, and a balanced tree) are two legitimate evaluations of the
# same iteration; where THEY part by more than the project's bar for histories (1e-10 relative) no device order can be
# held to it either.  Down to r.r <= 1e-6 (88 iterations) they agree to 6.3e-12; at 1e-10 (103 iterations) they are
# 1.2e-9 apart.  The range is tightened, the bar stays: the GPU tests stop at HISTORY_THRESHOLD.
SYSTEM = (32, 32, 6)
HISTORY_THRESHOLD = 1e-6
HISTORY_BAR = 1e-10
MAX_ITRS = 400


def system():
    mat = P.scaled_laplace(*SYSTEM)
    return mat, _vecc.csr_of(*mat), rhs(mat[3], 1), P.jacobi(mat)


_runs = {}


def model_run(precond=True, total="serial"):
    """the model loop on the system, computed once per process: -> (iterations, history)"""
    key = (precond, total)
    if key not in _runs:
        mat, csr, b, dinv = system()
        it, hist, _ = P.pcg_loop(csr, b, dinv if precond else None, MAX_ITRS, HISTORY_THRESHOLD,
                                 total=_vecc.serial_sum if total == "serial" else P.pairwise_sum)
        _runs[key] = (it, hist)
    return _runs[key]


def test_header_declares_the_four_entries():
    from test_capi_symbols import declared_symbols
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s


def test_library_signatures_and_methods_agree_on_the_four_entries():
    out = child("""
import ctypes, inspect
from abft_sparse_cg_amd import capi
lib = ctypes.CDLL(capi.LIB_PATH)
missing = [s for s in %r if not hasattr(lib, s) or s not in capi.SIGNATURES]
assert not missing, missing
import abft_sparse_cg_amd as amd
for s in %r:
    assert callable(getattr(amd.HIPContext, s[len("abft_hip_"):])), s
# dinv is one more handle: the preconditioned entries take one pointer more than their plain protected counterparts
S = capi.SIGNATURES
assert len(S["abft_hip_calc_r_precond_vecc"][1]) == len(S["abft_hip_calc_r_vecc"][1]) + 1
assert len(S["abft_hip_calc_px_precond_vecc"][1]) == len(S["abft_hip_calc_px_vecc"][1]) + 1
assert S["abft_hip_pcg_vecc_iteration_until_dev"] == S["abft_hip_pcg_iteration_until_dev"]
assert S["abft_hip_precond_start_vecc"] == S["abft_hip_precond_start"]
assert inspect.signature(amd.HIPContext.jacobi).parameters["protected"].default is False
print("ok")
""" % (NEW, NEW))
    assert out.strip() == "ok"


def test_jacobi_protected_encodes_in_place_and_marks_the_vector():
    out = child(r"""
import abft_sparse_cg_amd as amd

class L:
    def abft_hip_matrix_diag_inverse(self, *a):
        return 0

class Fake:
    L, h, calls = L(), None, []
    def create_vector(self, n):
        class Vec:
            h = None
        self.calls.append("create"); return Vec()
    def destroy_vector(self, v):
        self.calls.append("destroy")
    def encode_vector(self, v):
        self.calls.append("encode"); self.encoded = v

class Mat:
    h, n_out = None, 5

f = Fake()
d = amd.HIPContext.jacobi(f, Mat())
assert f.calls == ["create"] and not hasattr(d, "protected") and d.bad == 0      # today's call and object
d = amd.HIPContext.jacobi(f, Mat(), strict=True, protected=False)
assert f.calls == ["create"] * 2 and not hasattr(d, "protected")
d = amd.HIPContext.jacobi(f, Mat(), protected=True)
assert f.calls == ["create", "create", "create", "encode"] and f.encoded is d and d.protected is True
print("ok")
""")
    assert out.strip() == "ok", out


# ---- the model with dinv == 1.0 against the model of the plain protected calls ----

def same_sum(a, b):
    return (np.isnan(a) and np.isnan(b)) or np.float64(a).view(U) == np.float64(b).view(U)


def operands(name, n):
    return [_vecc.family(name, n, _vecc.operand_seed(n, k)) for k in range(4)]


@pytest.mark.parametrize("name", sorted(_vecc.FAMILIES))
@pytest.mark.parametrize("n", [1, 2, 255, 1025])
def test_model_with_unit_dinv_is_calc_xr_and_calc_p_word_for_word(name, n):
    xw, rw, pw, ww = operands(name, n)
    one = _vecc.encode(np.ones(n))
    for alpha in (0.37251, -1.0, 0.0, 1e308):
        beta = -alpha / 3
        xs, rs, rr = _vecc.calc_xr(xw, rw, pw, ww, alpha)
        ps = _vecc.calc_p(pw, rs, beta)
        r2, rz2, rr2 = P.calc_r_precond(rw, ww, one, alpha)
        x2, p2 = P.calc_px_precond(xw, pw, r2, one, alpha, beta)
        for got, want, what in ((r2, rs, "r"), (x2, xs, "x"), (p2, ps, "p")):
            _vecc.assert_words(got, want, what)
            assert np.array_equal(got, want), what  # one model: NaNs too
        assert same_sum(rr2, rr) and same_sum(rz2, rr2), (rz2, rr2, rr)
    p0, rz0, rr0 = P.precond_start(rw, one)
    assert np.array_equal(_vecc.strip(p0).view(U), _vecc.value(rw).view(U))  # a copy of r
    assert same_sum(rr0, _vecc.dot(rw, rw)) and same_sum(rz0, rr0)


def test_model_forms_z_from_the_stored_r_and_never_truncates_it():
    # r' = enc(r - alpha w) loses bits; z' = dinv * r' is formed from THAT r', and the sum uses all 53 bits of z'
    rw, ww = _vecc.encode(np.array([1.0])), _vecc.encode(np.array([2.0 ** -46]))
    dw = _vecc.encode(np.array([1.0 / 3.0]))
    rs, rz, rr = P.calc_r_precond(rw, ww, dw, -1.0)
    assert _vecc.strip(rs)[0] == 1.0 and rr == 1.0  # 1 + 2^-46 truncated toward zero
    d = float(_vecc.strip(dw)[0])
    assert rz == d * 1.0 and d != 1.0 / 3.0  # dinv's own truncation is part of M; nothing else is cut
    r, d = 1.125, 1.0 + 2.0 ** -44  # both survive enc; z = d r = 1.125 + 2^-44 + 2^-47 has a bit below the cut
    pw, rz, _ = P.precond_start(_vecc.encode(np.array([r])), _vecc.encode(np.array([d])))
    cut = float(_vecc.strip(pw)[0])
    assert cut == 1.125 + 2.0 ** -44 and d * r != cut  # p holds enc(z) ...
    assert rz == r * (d * r) and rz != r * cut  # ... and the sum the z that was never truncated


@pytest.mark.parametrize("op", ["x", "r", "p", "w", "dinv"])
def test_model_repairs_a_flipped_word_in_any_operand(op):
    n = 257
    xw, rw, pw, ww = operands("finite", n)
    dw = _vecc.encode(np.random.default_rng(8).random(n) + 0.25)
    clean = dict(x=xw, r=rw, p=pw, w=ww, dinv=dw)
    rs, rz, rr = P.calc_r_precond(rw, ww, dw, 0.71)
    xs, ps = P.calc_px_precond(xw, pw, rs, dw, 0.71, 0.125)
    p0 = P.precond_start(rw, dw)
    for index, bit in ((0, 0), (128, 3), (n - 1, 55)):
        v = dict(clean)
        v[op] = P.flipped(v[op], index, [bit])
        r2, rz2, rr2 = P.calc_r_precond(v["r"], v["w"], v["dinv"], 0.71)
        x2, p2 = P.calc_px_precond(v["x"], v["p"], rs if op != "r" else P.flipped(rs, index, [bit]), v["dinv"], 0.71, 0.125)
        assert np.array_equal(r2, rs) and np.array_equal(x2, xs) and np.array_equal(p2, ps), (index, bit)
        assert same_sum(rz2, rz) and same_sum(rr2, rr)
        got = P.precond_start(v["r"], v["dinv"])
        assert np.array_equal(got[0], p0[0]) and same_sum(got[1], p0[1]) and same_sum(got[2], p0[2])


def test_model_of_the_guarded_iteration():
    csr, n = VECC_HOST.small_csr()
    rng = np.random.default_rng(6)
    xw, rw, pw = (_vecc.encode(rng.standard_normal(n)) for _ in range(3))
    dw = _vecc.encode(rng.random(n) + 0.25)
    _, rz, rr = P.precond_start(rw, dw)
    live = P.iteration(csr, xw, rw, pw, dw, (rr, rz), 0.5 * rr)
    assert live["live"]
    ww, fused = _vecc.spmv(*csr, pw)
    alpha = P.fdiv(rz, fused)
    rs, rz_new, rr_new = P.calc_r_precond(rw, ww, dw, alpha)
    xs, ps = P.calc_px_precond(xw, pw, rs, dw, alpha, P.fdiv(rz_new, rz))
    assert all(np.array_equal(live[k], v) for k, v in (("w", ww), ("r", rs), ("x", xs), ("p", ps)))
    assert same_sum(live["pw"], fused) and same_sum(live["out"][0], rr_new) and same_sum(live["out"][1], rz_new)
    # a flip in any operand: the words of the clean iteration
    for name, at in (("x", 0), ("r", 17), ("p", n - 1), ("dinv", 30)):
        v = dict(x=xw, r=rw, p=pw, dinv=dw)
        v[name] = P.flipped(v[name], at, [44])
        hit = P.iteration(csr, v["x"], v["r"], v["p"], v["dinv"], (rr, rz), 0.0)
        assert all(np.array_equal(hit[k], live[k]) for k in "xrpw"), name
    # frozen: at the threshold, above it, a NaN -- every word kept (a flipped one included), the record handed on
    nan = np.array([0x7FF8000000ABCDEF], U).view(np.float64)[0]
    bad = P.flipped(rw, 3, [9])
    for cur, thr in ((rr, rr), (rr, np.inf), (nan, 0.0)):
        f = P.iteration(csr, xw, bad, pw, dw, (cur, rz), thr)
        assert not f["live"] and f["x"] is xw and f["r"] is bad and f["p"] is pw and f["w"] is None
        assert np.float64(f["out"][0]).view(U) == np.float64(cur).view(U) and f["out"][1] == rz
    assert P.OPERAND == {"vec": 0, "x": 1, "r": 2, "p": 3, "w": 4, "dinv": 5}


# ---- the model solves ----

def test_scaled_laplace_is_symmetric_badly_scaled_and_jacobi_undoes_it():
    mat, csr, b, dinv = system()
    cols, rows, vals, n = mat
    assert n == 1024 and np.all(np.diff(rows.astype(np.int64)) >= 0)
    A = np.zeros((n, n))
    A[rows, cols] = vals
    assert np.array_equal(A, A.T)
    diag = np.diag(A)
    assert np.all(diag > 0) and 0.99e6 <= diag.max() / diag.min() <= 1.01e6
    s = np.sqrt(dinv)
    assert np.allclose(s[:, None] * A * s[None, :], s[:, None] * A.T * s[None, :])
    assert np.allclose(np.diag(s[:, None] * A * s[None, :]), 1.0)
    assert np.linalg.eigvalsh(A).min() > 0


def test_model_loop_converges_where_the_unpreconditioned_one_does_not():
    it, hist = model_run()
    assert 20 < it < MAX_ITRS and hist[-1] <= HISTORY_THRESHOLD < hist[-2]
    it_plain, hist_plain = model_run(precond=False)
    print("PCG %d iterations; plain protected CG %d (max_itrs %d), last r.r %.3g" % (it, it_plain, MAX_ITRS, hist_plain[-1]))
    assert it_plain > it  # more iterations, or none enough: the count is max_itrs then
    assert it_plain < MAX_ITRS or not (hist_plain[-1] <= HISTORY_THRESHOLD)


def test_compared_range_two_orders_of_the_models_sums_agree_to_the_bar():
    it, hist = model_run()
    it2, hist2 = model_run(total="pairwise")
    assert it == it2
    err = max(abs(a - b) / abs(b) for a, b in zip(hist, hist2))
    print("serial against pairwise sums over %d iterations down to r.r <= %g: %.3g" % (it, HISTORY_THRESHOLD, err))
    assert err <= HISTORY_BAR, err


# ---- cg_solve / cg_solve_device on the stand-in ----
# The stand-in's vectors hold plain doubles (encode and scrub only leave their names in the call list): what is checked
# is who is called when and with what, and that the two loops are one iteration, bit for bit.  PSingle is the stand-in
# of the plain preconditioned loop, VSingle that of the plain protected one; PV has both and the new calls.
STANDIN = PRECOND_HOST.STANDIN + VECC_HOST.STANDIN[len(BASE):] + r'''
class PV(VSingle, PSingle):
    def precond_start_vecc(self, r, dinv, p):
        self.calls.append(("precond_start_vecc",))
        z = dinv.a * r.a
        p.a[:] = z
        return float(np.sum(r.a * z)), float(np.sum(r.a * r.a))
    def calc_r_precond_vecc(self, r, w, dinv, alpha):
        self.calls.append(("calc_r_precond_vecc", alpha))
        r.a[:] = r.a - alpha * w.a
        z = dinv.a * r.a
        return float(np.sum(r.a * z)), float(np.sum(r.a * r.a))
    def calc_px_precond_vecc(self, x, p, r, dinv, alpha, beta):
        self.calls.append(("calc_px_precond_vecc", alpha, beta))
        x.a[:] = x.a + alpha * p.a; p.a[:] = dinv.a * r.a + beta * p.a
    def pcg_vecc_iteration_until_dev(self, A, vec, x, r, p, w, dinv, sc, in_at, pw_at, out_at, thr):
        PSingle.pcg_iteration_until_dev(self, A, vec, x, r, p, w, dinv, sc, in_at, pw_at, out_at, thr)
        self.calls[-1] = ("pvecc_until",) + self.calls[-1][1:]

def prot(d):
    v = V(d.copy()); v.protected = True
    return v

def prun(max_itrs, conv, stride=None, graph=True, mat=None, b=pb, precond="protected", **kw):
    """stride None: cg_solve; -> (it, rr, x, history, stand-in, the precond object)"""
    s = PV(PA)
    vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(pn)), V(np.zeros(pn)), V(np.zeros(pn)), V(np.zeros(pn))
    d = prot(pdinv) if precond == "protected" else precond
    hist = []
    if d is not None:
        kw["precond"] = d
    if stride is None:
        it, rr = cg_solve(s, mat or Mat(), vb, vx, vr, vp, vw, max_itrs, conv, on_iteration=lambda i, v: hist.append(v), **kw)
    else:
        it, rr = cg_solve_device(s, mat or Mat(), vb, vx, vr, vp, vw, max_itrs, conv,
                                 on_iteration=lambda i, v: hist.append(v), stride=stride, graph=graph, **kw)
    return it, rr, vx.a, hist, s, d

START = ["encode", "encode", "copy", "scrub", "precond_start_vecc"]
END = ["scrub", "scrub", "scrub"]
'''


def test_host_loop_makes_the_specified_call_sequence():
    out = child(STANDIN + r'''
it, rr, x, h, s, d = prun(1000, 1e-20, vector_ecc=True)
k = kinds(s)
assert 23 < it < 1000 and len(h) == it
assert k[:5] == START and k[-3:] == END, k
assert k[5:-3] == ["spmv_vecc", "dot_vecc", "calc_r_precond_vecc", "calc_px_precond_vecc"] * it
body = s.calls[5:-3]
for i in range(it):
    r_call, px_call = body[4 * i + 2], body[4 * i + 3]
    assert bits([r_call[1]])[0] == bits([px_call[1]])[0]          # one alpha for both halves
# it is the plain preconditioned loop's arithmetic: same history, same x, bit for bit
it0, rr0, x0, h0, _, _ = phost(PA, pb, pdinv, 1000, 1e-20)
assert it == it0 and np.array_equal(bits(h), bits(h0)) and np.array_equal(bits(x), bits(x0))
# alpha = rz / p.w and beta = rz_new / rz, rz the first sum of the call before: the calls replayed by hand
s2 = PV(PA)
vb, vx, vr, vp, vw = V(pb.copy()), V(np.zeros(pn)), V(np.zeros(pn)), V(np.zeros(pn)), V(np.zeros(pn))
dv = prot(pdinv)
for i in range(3):
    if i == 0:
        vr.a[:] = vb.a; rz_i, _ = s2.precond_start_vecc(vr, dv, vp)
    s2.spmv_vecc(None, vp, vw); pw = s2.dot_vecc(vp, vw)
    alpha = fdiv(rz_i, pw)
    assert bits([alpha])[0] == bits([body[4 * i + 2][1]])[0], i
    rz_new, _ = s2.calc_r_precond_vecc(vr, vw, dv, alpha)
    assert bits([fdiv(rz_new, rz_i)])[0] == bits([body[4 * i + 3][2]])[0], i
    s2.calc_px_precond_vecc(vx, vp, vr, dv, alpha, fdiv(rz_new, rz_i)); rz_i = rz_new
# nothing to do: the start, then the three scrubs
for kw in (dict(b=np.zeros(pn), max_itrs=1000), dict(b=pb, max_itrs=0)):
    it, rr, x, h, s, d = prun(kw["max_itrs"], 1e-3, b=kw["b"], vector_ecc=True)
    assert (it, h) == (0, []) and kinds(s) == START + END, kinds(s)
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_device_loop_makes_the_specified_calls_and_is_the_host_loop_bit_for_bit():
    out = child(STANDIN + r'''
it0, rr0, x0, h0, s0, _ = prun(1000, 1e-20, vector_ecc=True)
for stride in (1, 3, 16):
    for graph in (True, False):
        for max_itrs in (1000, 23, it0):
            want = min(it0, max_itrs)
            it, rr, x, h, s, d = prun(max_itrs, 1e-20, stride, graph, vector_ecc=True)
            assert it == want == len(h) == s.live, (stride, graph, it, want)
            assert np.array_equal(bits(h), bits(h0[:want])) and bits([rr])[0] == bits(h0[want - 1:want])[0]
            if max_itrs >= it0:
                assert np.array_equal(bits(x), bits(x0))
            k = kinds(s)
            assert k[:5] == START and k[-3:] == END, k
            assert k[-6:-3] == ["destroy"] * 3  # the trail and its two views
            body = s.calls[5:-6]
            assert {c[0] for c in body} == {"copy", "pvecc_until"} and body[0][0] == "copy", body
            for c in body:  # the trail: record i at 4 i, p.w behind the stride + 1 records
                if c[0] == "pvecc_until":
                    assert c[1] % 4 == 0 and c[3] == c[1] + 4 and c[2] == 4 * (stride + 1) and c[1] < 4 * stride, c
            assert not {"until", "vecc_until", "pcg_until", "dot", "dot_vecc", "spmv_vecc",
                        "precond_start"} & set(k)
            looks = -(-want // stride) + (1 if want % stride == 0 and want < max_itrs else 0)
            assert s.downloads == looks, (stride, graph, s.downloads, looks)
            if not graph:
                assert [c[0] for c in body].count("pvecc_until") == s.live + s.frozen
                assert [c[0] for c in body].count("copy") == looks
for kw in (dict(b=np.zeros(pn), max_itrs=1000), dict(b=pb, max_itrs=0)):
    it, rr, x, h, s, d = prun(kw["max_itrs"], 1e-3, 3, b=kw["b"], vector_ecc=True)
    assert (it, h, s.downloads, s.live, s.frozen) == (0, [], 0, 0, 0) and kinds(s) == START + END, kinds(s)
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_refusals_come_before_any_call():
    out = child(STANDIN + r'''
def refused(text, stride, **kw):
    s = PV(PA)
    vs = [V(pb.copy())] + [V(np.zeros(pn)) for _ in range(4)]
    d = kw.get("precond")
    before = None if d is None else d.a.copy()
    mat = kw.pop("mat", None) or Mat()
    try:
        if stride is None:
            cg_solve(s, mat, *vs, 1000, 1e-3, **kw)
        else:
            cg_solve_device(s, mat, *vs, 1000, 1e-3, stride=stride, **kw)
    except ValueError as e:
        assert all(t in str(e) for t in text), (text, str(e))
    else:
        raise AssertionError(text)
    assert s.calls == [] and s.downloads == 0, (text, s.calls)
    assert np.array_equal(vs[0].a, pb) and not any(v.a.any() for v in vs[1:])
    assert d is None or np.array_equal(d.a, before)

for stride in (None, 4):
    # an unencoded dinv would be misread as codewords
    refused(["precond", "ctx.jacobi(A, protected=True)"], stride, vector_ecc=True, precond=V(pdinv.copy()))
    # a protected dinv in a loop that multiplies with plain doubles
    refused(["precond", "ctx.jacobi(A, protected=True)", "vector_ecc"], stride, precond=prot(pdinv))
    refused(["precond"], stride, vector_ecc=False, precond=prot(pdinv))
    # the matrices spmv_vecc does not run on
    refused(["COO"], stride, vector_ecc=True, precond=prot(pdinv), mat=Mat(FMT_COO))
    refused(["panels"], stride, vector_ecc=True, precond=prot(pdinv), mat=Mat(FMT_CSR, "panels"))
    refused(["sweep"], stride, vector_ecc=True, precond=prot(pdinv), mat=Mat(FMT_CSR, "sweep"))
# the block loops have no protected form: a protected dinv is refused there too
from abft_sparse_cg_amd.context import cg_solve_block_device
for solve in (cg_solve_block, cg_solve_block_device):
    s = PV(PA)
    vs = [V(np.zeros((pn, 2)), 2) for _ in range(5)]
    try:
        solve(s, Mat(), *vs, 10, 1e-3, precond=prot(pdinv))
    except ValueError as e:
        assert "precond" in str(e) and "ctx.jacobi(A, protected=True)" in str(e), str(e)
    else:
        raise AssertionError(solve.__name__)
    assert s.calls == []
refused(["check_every"], None, vector_ecc=True, precond=prot(pdinv), check_every=5)
refused(["check_every"], None, vector_ecc=True, check_every=5)
print("ok")
''')
    assert out.strip() == "ok", out


def test_without_the_new_arguments_the_calls_are_todays():
    out = child(STANDIN + r'''
# vector_ecc alone: the plain protected loops
it, rr, x, h, s, _ = prun(1000, 1e-20, precond=None, vector_ecc=True)
k = kinds(s)
assert k[:6] == ["encode", "encode", "copy", "scrub", "copy", "dot_vecc"] and k[-2:] == ["scrub", "scrub"]
assert k[6:-2] == ["spmv_vecc", "dot_vecc", "calc_xr_vecc", "calc_p_vecc"] * it
it, rr, x, h, s, _ = prun(1000, 1e-20, 3, False, precond=None, vector_ecc=True)
k = kinds(s)
assert k[:6] == ["encode", "encode", "copy", "scrub", "copy", "dot_vecc"] and k[-2:] == ["scrub", "scrub"]
assert set(k[6:-5]) == {"copy", "vecc_until"}
# an unprotected precond alone: the plain preconditioned loops, dinv never scrubbed or encoded
it, rr, x, h, s, _ = prun(1000, 1e-20, precond=V(pdinv.copy()))
k = kinds(s)
assert k[:2] == ["copy", "precond_start"] and k[2:] == ["spmv", "dot", "calc_xr_precond", "calc_p_precond"] * it, k[:12]
it, rr, x, h, s, _ = prun(1000, 1e-20, 3, False, precond=V(pdinv.copy()))
k = kinds(s)
assert k[:2] == ["copy", "precond_start"] and set(k[2:-3]) == {"copy", "pcg_until"} and k[-3:] == ["destroy"] * 3
# neither: the plain loops
it, rr, x, h, s, _ = prun(1000, 1e-20, precond=None)
k = kinds(s)
assert k[:3] == ["copy", "copy", "dot"] and k[3:] == ["spmv", "dot", "calc_xr", "calc_p"] * it
it, rr, x, h, s, _ = prun(1000, 1e-20, 3, False, precond=None)
k = kinds(s)
assert k[:3] == ["copy", "copy", "dot"] and set(k[3:-3]) == {"copy", "until"}
print("ok")
''')
    assert out.strip() == "ok", out
