"""CPU-side checks of the protected block iteration (abft_hip_spmm_dot_vecc, abft_hip_dot_block_vecc,
abft_hip_calc_r_block_vecc, abft_hip_calc_px_block_vecc, cg_solve_block(vector_ecc=True)):

 - the block model (tests/_vecc_block.py) is, column by column, the model of the single protected calls (tests/_vecc.py):
   _vecc.spmv / _vecc.calc_xr / _vecc.calc_p on column j; an inactive column keeps its words, a flipped one comes back
   repaired;
 - the model loop on the system of the GPU solver tests stops where the issue says it does, under two orders of its
   sums, and the two histories stay within the bar the GPU tests hold the device to;
 - cg_solve_block(vector_ecc=True) on a stand-in context: the exact call sequence, every refusal before any call with
   the vectors untouched, and without the keyword today's calls;
 - the header, capi.SIGNATURES, the built library and HIPContext agree on the four new entries.

Whatever loads the package runs in a child interpreter, as in the sibling host tests."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vecc  # noqa: E402
import _vecc_block as B  # noqa: E402
from _oracle import laplace5, rhs  # noqa: E402
from test_residual_check_host import STANDIN as BASE, child  # noqa: E402

U = np.uint64
NEW = ["abft_hip_spmm_dot_vecc", "abft_hip_dot_block_vecc", "abft_hip_calc_r_block_vecc",
       "abft_hip_calc_px_block_vecc"]
MASKS = {"all": lambda k: (1 << k) - 1, "none": lambda k: 0, "one": lambda k: 1 << (k - 1),
         "alternating": lambda k: 0x55 & ((1 << k) - 1)}


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
S = capi.SIGNATURES
# each takes what its plain twin takes
for s in ("spmm_dot", "dot_block", "calc_r_block", "calc_px_block"):
    assert S["abft_hip_%%s_vecc" %% s] == S["abft_hip_" + s], s
params = list(inspect.signature(amd.cg_solve_block).parameters)
assert params[-1] == "vector_ecc" and params[-2] == "fused", params      # last: positional calls are unchanged
assert inspect.signature(amd.cg_solve_block).parameters["vector_ecc"].default is False
print("ok")
""" % (NEW, NEW))
    assert out.strip() == "ok"


# ---- the block model against the model of the single calls ----

def same_sum(a, b):
    return (np.isnan(a) and np.isnan(b)) or np.float64(a).view(U) == np.float64(b).view(U)


def operands(name, n, k, count):
    return [B.block(_vecc.family(name, n * k, _vecc.operand_seed(n * k, c)), k) for c in range(count)]


def small_csr(n=37):
    rng = np.random.default_rng(21)
    rows, cols, vals = [], [], []
    for i in range(n):
        if i % 7 == 3:
            continue  # an empty row
        for c in sorted(set(rng.integers(0, n, 1 + i % 5).tolist() + [i])):
            rows.append(i), cols.append(c), vals.append(rng.standard_normal())
    return _vecc.csr_of(cols, rows, vals, n), n


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_spmm_dot_is_spmv_column_by_column(k):
    csr, n = small_csr()
    P = B.block(_vecc.encode(_vecc.salted(n * k, 5 + k)), k)
    W, pw = B.spmm_dot(csr, P)
    for j in range(k):
        yw, fused = _vecc.spmv(*csr, P[:, j])
        assert np.array_equal(W[:, j], yw) and same_sum(pw[j], fused), j
    # a flip in P: the clean call's words and sums
    hit = B.flipped(P, 5, k - 1, [52])
    W2, pw2 = B.spmm_dot(csr, hit)
    assert np.array_equal(W2, W) and all(same_sum(a, b) for a, b in zip(pw2, pw))


@pytest.mark.parametrize("name", sorted(_vecc.FAMILIES))
@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_vector_calls_are_the_single_models_column_by_column(name, mask, k):
    n = 33
    X, R, P, W = operands(name, n, k, 4)
    active = MASKS[mask](k)
    alpha = [_vecc.SCALARS[(j + k) % len(_vecc.SCALARS)] for j in range(k)]
    beta = [_vecc.SCALARS[(2 * j + 1) % len(_vecc.SCALARS)] for j in range(k)]
    R2, sums = B.calc_r_block(R, W, alpha, active)
    X2, P2 = B.calc_px_block(X, P, R2, alpha, beta, active)
    dots = B.dot_block(R2, R2)
    for j in range(k):
        if B.on(active, j):
            xs, rs, rr = _vecc.calc_xr(X[:, j], R[:, j], P[:, j], W[:, j], alpha[j])
            ps = _vecc.calc_p(P[:, j], rs, beta[j])
            assert np.array_equal(R2[:, j], rs) and np.array_equal(X2[:, j], xs) and np.array_equal(P2[:, j], ps), j
            assert same_sum(sums[j], rr), j
        else:  # kept, every bit
            assert np.array_equal(R2[:, j], R[:, j]) and np.array_equal(X2[:, j], X[:, j]), j
            assert np.array_equal(P2[:, j], P[:, j]), j
        assert same_sum(sums[j], dots[j]), j  # the sums are dot_block(R, R) of the R the call leaves
        assert same_sum(dots[j], _vecc.dot(R2[:, j], R2[:, j])), j


@pytest.mark.parametrize("op", ["X", "R", "P", "W"])
@pytest.mark.parametrize("where", ["active", "inactive"])
def test_a_flip_in_any_operand_and_column_leaves_the_clean_calls_words(op, where):
    n, k, active = 33, 3, 0b101
    X, R, P, W = operands("finite", n, k, 4)
    alpha, beta = [0.37251, 0.0, -1.0], [0.5, 0.0, 0.25]
    R0, s0 = B.calc_r_block(R, W, alpha, active)
    X0, P0 = B.calc_px_block(X, P, R0, alpha, beta, active)
    j = 2 if where == "active" else 1
    for i, bit in ((0, 0), (16, 7), (n - 1, 63)):
        v = dict(X=X, R=R, P=P, W=W)
        v[op] = B.flipped(v[op], i, j, [bit])
        R1, s1 = B.calc_r_block(v["R"], v["W"], alpha, active)
        X1, P1 = B.calc_px_block(v["X"], v["P"], B.flipped(R0, i, j, [bit]) if op == "R" else R0, alpha, beta, active)
        assert np.array_equal(R1, R0) and np.array_equal(X1, X0) and np.array_equal(P1, P0), (i, bit)
        assert all(same_sum(a, b) for a, b in zip(s1, s0))
        assert not _vecc.decode(R1)[1].any() and not _vecc.decode(X1)[1].any() and not _vecc.decode(P1)[1].any()
    # two flips in one inactive word: not repairable, the word stays as it is
    bad = B.flipped(X, 4, 1, [9, 40])
    X1, _ = B.calc_px_block(bad, P, R0, alpha, beta, active)
    assert X1[4, 1] == bad[4, 1] and _vecc.decode(X1[4:5, 1])[1][0] == 2


# ---- the model loop on the system of the GPU solver tests ----
SYSTEM = (40, 40)
K = 4
HISTORY_BAR = 1e-10  # the project's bar for r.r histories
_runs = {}


def pairwise_sum(terms):
    t = np.asarray(terms, dtype=np.float64)
    while t.size > 1:
        if t.size % 2:
            t = np.concatenate([t, [0.0]])
        t = t[0::2] + t[1::2]
    return float(t[0]) if t.size else 0.0


def system():
    cols, rows, vals, n = laplace5(*SYSTEM)
    return _vecc.csr_of(cols, rows, vals, n), np.stack([rhs(n, 1 + j) for j in range(K)], axis=1)


def model_run(threshold, total="serial"):
    key = (threshold, total)
    if key not in _runs:
        csr, Bm = system()
        _runs[key] = B.cg_block_loop(csr, Bm, 1000, threshold, total=None if total == "serial" else pairwise_sum)
    return _runs[key]


@pytest.mark.parametrize("threshold, counts", [(1e-3, [59, 60, 63, 64]), (1e-10, [107, 108, 108, 108])])
def test_model_loop_stops_where_the_gpu_tests_expect_under_two_orders_of_its_sums(threshold, counts):
    it, hist, _ = model_run(threshold)
    it2, hist2, _ = model_run(threshold, "pairwise")
    assert it == counts and it2 == counts, (it, it2)
    err = max(float(np.max(np.abs(a - b) / np.abs(b))) for a, b in zip(hist, hist2))
    print("serial against pairwise sums down to %g: %.3g relative" % (threshold, err))
    assert err <= HISTORY_BAR
    final = hist[-1]
    assert all(abs(final[j] - threshold) > 1e-3 * threshold for j in range(K)), final  # no count hangs on a rounding


# ---- cg_solve_block on the stand-in ----
# The stand-in's blocks hold plain doubles (encode and scrub only leave their names in the call list): what is checked
# is who is called when and with what.
STANDIN = BASE + r'''
class VBlock(Block):
    info = "stream"
    fmt = 2
    def vecc_supported(self, mat):
        return self.info == "stream"
    def matrix_info(self, mat):
        return (self.info,)
    def encode_vector(self, v):
        self.calls.append(("encode", v.name))
    def scrub_vector(self, v):
        self.calls.append(("scrub", v.name)); return 0, 0
    def copy_vector(self, d, s):
        self.calls.append(("copy", d.name, s.name)); d.a[:] = s.a
    def dot_block_vecc(self, a, b, k):
        self.calls.append(("dot_block_vecc", a.name, b.name, k))
        return np.array([float(np.sum(col(a, j) * col(b, j))) for j in range(k)])
    def spmm_dot_vecc(self, A, P, W, k, drain=True):
        self.calls.append(("spmm_dot_vecc", P.name, W.name, k, drain))
        for j in range(k):
            W.a[:, j] = self.A @ col(P, j)
        return np.array([float(np.sum(col(P, j) * col(W, j))) for j in range(k)])
    def calc_r_block_vecc(self, R, W, k, alpha, active):
        self.calls.append(("calc_r_block_vecc", R.name, W.name, k, tuple(alpha), active))
        for j in range(k):
            if (active >> j) & 1:
                R.a[:, j] = R.a[:, j] - alpha[j] * W.a[:, j]
        return np.array([float(np.sum(col(R, j) * col(R, j))) for j in range(k)])
    def calc_px_block_vecc(self, X, P, R, k, alpha, beta, active):
        self.calls.append(("calc_px_block_vecc", X.name, P.name, R.name, k, tuple(alpha), tuple(beta), active))
        for j in range(k):
            if (active >> j) & 1:
                X.a[:, j] = X.a[:, j] + alpha[j] * P.a[:, j]
                P.a[:, j] = R.a[:, j] + beta[j] * P.a[:, j]

class Mat:
    fmt = 2

def vectors(Bm):
    n, k = Bm.shape
    out = []
    for name, a in (("B", Bm.copy()), ("X", np.zeros((n, k))), ("R", np.full((n, k), 7.0)), ("P", np.full((n, k), 8.0)),
                    ("W", np.full((n, k), 9.0))):
        v = V(a, k); v.name = name; out.append(v)
    return out

k = 3
Bm = np.stack([b * (j + 1) ** 3 for j in range(k)], axis=1)   # scaled columns: they stop at different iterations
'''


def test_protected_block_loop_makes_exactly_the_documented_calls():
    out = child(STANDIN + r'''
import abft_sparse_cg_amd.context as C
C.FMT_CSR = 2
s = VBlock(A)
vs = vectors(Bm)
seen = []
itrs, rr = cg_solve_block(s, Mat(), *vs, 1000, 1e-6, on_iteration=lambda i, r, act: seen.append((i, r.copy(), act)),
                          fused=False, vector_ecc=True)
calls = s.calls
assert calls[:6] == [("encode", "B"), ("encode", "X"), ("copy", "R", "B"), ("scrub", "R"), ("copy", "P", "R"),
                     ("dot_block_vecc", "R", "R", k)], calls[:6]
assert calls[-2:] == [("scrub", "X"), ("scrub", "B")], calls[-2:]
body = calls[6:-2]
assert len(body) == 3 * len(seen) and len(set(itrs)) > 1, (len(body), len(seen), itrs)
rr_prev = np.array([float(np.sum(Bm[:, j] * Bm[:, j])) for j in range(k)])
done = [0] * k
for i, (it, r, act) in enumerate(seen):
    want = sum(1 << j for j in range(k) if done[j] < 1000 and rr_prev[j] > 1e-6)
    a, b, c = body[3 * i:3 * i + 3]
    assert a == ("spmm_dot_vecc", "P", "W", k, False), a
    assert b[:4] == ("calc_r_block_vecc", "R", "W", k) and b[5] == want, b
    assert c[:5] == ("calc_px_block_vecc", "X", "P", "R", k) and c[7] == want and c[5] == b[4], c
    for j in range(k):
        if not (want >> j) & 1:
            assert b[4][j] == 0.0 and c[6][j] == 0.0          # alpha and beta of a stopped column
            assert r[j] == rr_prev[j]
        else:
            done[j] += 1
    assert it == i and act == want
    rr_prev = r
assert done == itrs and not any(rr_prev[j] > 1e-6 for j in range(k))
# `fused` is ignored: the same calls
s2 = VBlock(A)
cg_solve_block(s2, Mat(), *vectors(Bm), 1000, 1e-6, fused=True, vector_ecc=True)
assert s2.calls == calls
# and the loop is the plain fused iteration, operation for operation (the stand-in's blocks hold plain doubles)
it0, rr0, x0, hist0, _, _ = block(A, Bm, 1000, 1e-6)
assert it0 == itrs
print("ok")
''')
    assert out.strip() == "ok", out


def test_every_refusal_comes_before_any_call_and_leaves_the_vectors_untouched():
    out = child(STANDIN + r'''
import abft_sparse_cg_amd.context as C
C.FMT_CSR = 2
class Dinv:
    pass
prot = Dinv(); prot.protected = True
cases = [(dict(check_every=5), "check_every", "stream"), (dict(precond=Dinv()), "precond", "stream"),
         (dict(precond=prot), "precond", "stream"), (dict(), "streaming layout", "panels")]
for kw, word, info in cases:
    s = VBlock(A); s.info = info
    vs = vectors(Bm)
    before = [v.a.copy() for v in vs]
    try:
        cg_solve_block(s, Mat(), *vs, 1000, 1e-6, vector_ecc=True, **kw)
    except ValueError as e:
        assert word in str(e) and "vector_ecc" in str(e), (word, str(e))
    else:
        raise AssertionError(kw)
    assert s.calls == [], (kw, s.calls)
    assert all(np.array_equal(a, v.a) for a, v in zip(before, vs))
# without vector_ecc a protected precond keeps its refusal and its message
s = VBlock(A)
try:
    cg_solve_block(s, Mat(), *vectors(Bm), 1000, 1e-6, precond=prot)
except ValueError as e:
    assert "a protected precond (ctx.jacobi(A, protected=True)) without vector_ecc" in str(e), str(e)
else:
    raise AssertionError("protected precond")
assert s.calls == []
print("ok")
''')
    assert out.strip() == "ok", out


def test_without_the_keyword_the_calls_are_todays():
    out = child(STANDIN + r'''
def run(**kw):
    s = VBlock(A)
    vs = vectors(Bm)
    res = cg_solve_block(s, None, *vs, 1000, 1e-6, **kw)
    return s.calls, res, [v.a.copy() for v in vs]
c0, r0, v0 = run()
c1, r1, v1 = run(vector_ecc=False)
assert c0 == c1 and r0[0] == r1[0] and np.array_equal(r0[1], r1[1]) and all(np.array_equal(a, b) for a, b in zip(v0, v1))
names = [c[0] for c in c0]
assert names[:3] == ["copy", "copy", "dot"] and set(names[3:]) == {"spmv", "dot", "calc_xr", "calc_p"}, names[:8]
assert names[3:7] == ["spmv", "dot", "calc_xr", "calc_p"]
assert not any("vecc" in n or n in ("encode", "scrub") for n in names)
print("ok")
''')
    assert out.strip() == "ok", out
