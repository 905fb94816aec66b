"""CPU-side checks of the device-resident block loop on protected vectors (abft_hip_cg_block_vecc_iteration_until_dev,
cg_solve_block_device(vector_ecc=True)):

 - the header, capi.SIGNATURES, the built library and HIPContext agree on the new entry, and cg_solve_block_device has
   `vector_ecc` last;
 - the model of one guarded iteration (tests/_devloop_block_vecc.py) is _vecc_block's spmm_dot + calc_r_block +
   calc_px_block with the mask of the live columns: every mask of K = 3, the all-frozen launch that keeps every word, a
   frozen column of a mixed launch that comes back repaired, a NaN record word that keeps its payload;
 - the model loop, driven record by record, reproduces _vecc_block.cg_block_loop on the system of the GPU solver tests;
 - cg_solve_block_device(vector_ecc=True) on the stand-in context of test_device_loop_block_host.py, extended by the
   protected calls: the exact call sequence, the refusals, and without the keyword today's calls.

Whatever loads the package runs in a child interpreter, as in the sibling host tests."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vecc  # noqa: E402
import _vecc_block as B  # noqa: E402
import _devloop_block_vecc as D  # noqa: E402
from test_block_vecc_host import K, model_run, small_csr, system  # noqa: E402
from test_device_loop_block_host import STANDIN as BASE, child  # noqa: E402

U = np.uint64
NEW = "abft_hip_cg_block_vecc_iteration_until_dev"
PAYLOAD = np.array([0x7FF8000000ABCDEF, 0xFFF0000000000123, 0x7FF4000000000001], dtype=U).view(np.float64)


def test_header_declares_the_entry():
    from test_capi_symbols import declared_symbols
    assert NEW in declared_symbols()


def test_library_signature_method_and_keyword_agree():
    out = child("""
import ctypes, inspect
from abft_sparse_cg_amd import capi
lib = ctypes.CDLL(capi.LIB_PATH)
s = %r
assert hasattr(lib, s) and s in capi.SIGNATURES
import abft_sparse_cg_amd as amd
assert callable(amd.HIPContext.cg_block_vecc_iteration_until_dev)
S = capi.SIGNATURES
plain = S["abft_hip_cg_block_iteration_until_dev"]
# the plain entry without its dinv
assert S[s][0] == plain[0] and len(S[s][1]) == 11 and list(S[s][1]) == list(plain[1][:6]) + list(plain[1][7:])
m = list(inspect.signature(amd.HIPContext.cg_block_vecc_iteration_until_dev).parameters)
assert m == ["self", "mat", "X", "R", "P", "W", "k", "scalars", "in_at", "pw_at", "out_at", "threshold"], m
sig = inspect.signature(amd.cg_solve_block_device)
params = list(sig.parameters)
assert params[-1] == "vector_ecc" and params[-2] == "precond", params   # last: positional calls are unchanged
assert sig.parameters["vector_ecc"].default is False
print("ok")
""" % (NEW,))
    assert out.strip() == "ok"


# ---- the model of one guarded iteration ----
THR = 0.1 + 0.2


def state(k=3, seed=0):
    csr, n = small_csr()
    X, R, P = (B.block(_vecc.encode(_vecc.salted(n * k, 17 * c + seed + k)), k) for c in range(3))
    return csr, n, X, R, P


def record(k, mask, cold_rr, cold_rz):
    """r.r = 2 + j and r.z = 3 + j in the live columns, the cold words in the others"""
    rr = np.array([2.0 + j if B.on(mask, j) else cold_rr[j] for j in range(k)])
    rz = np.array([3.0 + j if B.on(mask, j) else cold_rz[j] for j in range(k)])
    return np.concatenate([rr, rz])


@pytest.mark.parametrize("mask", range(8))
def test_every_mask_is_the_three_host_calls_with_that_mask(mask):
    k = 3
    csr, n, X, R, P = state(k)
    rec = record(k, mask, [np.nan, PAYLOAD[0], THR], [PAYLOAD[1], PAYLOAD[2], -0.0])
    assert D.live_mask(rec[:k], THR) == mask
    out = D.iteration(csr, X, R, P, rec, THR)
    assert out["active"] == mask
    if not mask:
        assert out["X"] is X and out["R"] is R and out["P"] is P and out["W"] is None
        assert np.array_equal(out["rec"], D.bits(rec))
        return
    W, pw = B.spmm_dot(csr, P)
    alpha = [B.fdiv(rec[k + j], pw[j]) if B.on(mask, j) else 0.0 for j in range(k)]
    R1, sums = B.calc_r_block(R, W, alpha, mask)
    beta = [B.fdiv(sums[j], rec[k + j]) if B.on(mask, j) else 0.0 for j in range(k)]
    X1, P1 = B.calc_px_block(X, P, R1, alpha, beta, mask)
    for name, want in (("X", X1), ("R", R1), ("P", P1), ("W", W)):
        assert np.array_equal(out[name], want), name
    assert np.array_equal(D.bits(out["pw"]), D.bits(pw))
    for j in range(k):
        if B.on(mask, j):  # the new sum in both words
            assert out["rec"][j] == out["rec"][k + j] == D.bits(sums[j:j + 1])[0], j
            assert not np.array_equal(out["X"][:, j], X[:, j]), j  # it ran
        else:  # handed on as integers, not the recomputed sum; the column's words kept
            assert out["rec"][j] == D.bits(rec)[j] and out["rec"][k + j] == D.bits(rec)[k + j], j
            for name, was in (("X", X), ("R", R), ("P", P)):
                assert np.array_equal(out[name][:, j], was[:, j]), (name, j)


def test_a_frozen_launch_keeps_every_word_a_flipped_one_included():
    k = 3
    csr, n, X, R, P = state(k)
    hit = {"X": B.flipped(X, 3, 1, [52]), "R": B.flipped(R, 0, 0, [7]), "P": B.flipped(P, n - 1, 2, [9, 40])}
    rec = record(k, 0, [THR, -1.0, np.nan], [1.0, 2.0, PAYLOAD[0]])
    out = D.iteration(csr, hit["X"], hit["R"], hit["P"], rec, THR)
    assert out["active"] == 0
    for name in "XRP":
        assert np.array_equal(out[name], hit[name]) and _vecc.decode(out[name])[1].any(), name
    assert np.array_equal(out["rec"], D.bits(rec))
    again = D.iteration(csr, out["X"], out["R"], out["P"], out["rec"].view(np.float64), THR)
    assert all(np.array_equal(again[name], hit[name]) for name in "XRP") and np.array_equal(again["rec"], out["rec"])


@pytest.mark.parametrize("op", ["X", "R", "P"])
def test_a_frozen_column_of_a_mixed_launch_comes_back_repaired(op):
    k, mask = 3, 0b101
    csr, n, X, R, P = state(k)
    rec = record(k, mask, [0.0, THR, 0.0], [0.0, 5.0, 0.0])
    clean = D.iteration(csr, X, R, P, rec, THR)
    v = dict(X=X, R=R, P=P)
    v[op] = B.flipped(v[op], 5, 1, [52])  # column 1 is frozen
    out = D.iteration(csr, v["X"], v["R"], v["P"], rec, THR)
    for name in ("X", "R", "P", "W"):
        assert np.array_equal(out[name], clean[name]), name
    assert np.array_equal(out["rec"], clean["rec"])
    assert np.array_equal(out[op][:, 1], dict(X=X, R=R, P=P)[op][:, 1])  # the clean word, every bit
    # two flips in a frozen word: not repairable, the word stays as it is
    v = dict(X=X, R=R, P=P)
    v[op] = B.flipped(v[op], 5, 1, [9, 40])
    out = D.iteration(csr, v["X"], v["R"], v["P"], rec, THR)
    assert out[op][5, 1] == v[op][5, 1] and _vecc.decode(out[op][5:6, 1])[1][0] == 2


def test_a_nan_record_word_keeps_its_payload_and_inf_is_live():
    k = 3
    csr, n, X, R, P = state(k)
    rec = np.concatenate([[PAYLOAD[0], np.inf, PAYLOAD[2]], [PAYLOAD[1], 4.0, PAYLOAD[0]]])
    out = D.iteration(csr, X, R, P, rec, 1e300)
    assert out["active"] == 0b010  # inf above a finite threshold is live, a NaN is frozen
    for j in (0, 2):
        assert out["rec"][j] == D.bits(rec)[j] and out["rec"][k + j] == D.bits(rec)[k + j], j
    assert out["rec"][1] == out["rec"][k + 1] != D.bits(rec)[1]
    frozen = D.iteration(csr, X, R, P, np.concatenate([PAYLOAD, PAYLOAD[::-1]]), 1e300)
    assert frozen["active"] == 0 and np.array_equal(frozen["rec"], D.bits(np.concatenate([PAYLOAD, PAYLOAD[::-1]])))


# ---- the model loop, record by record, on the system of the GPU solver tests ----

@pytest.mark.parametrize("threshold, counts", [(1e-3, [59, 60, 63, 64]), (1e-10, [107, 108, 108, 108])])
def test_model_loop_driven_record_by_record_is_the_host_model_loop(threshold, counts):
    csr, Bm = system()
    assert Bm.shape[1] == K == 4
    it_h, hist_h, x_h = model_run(threshold)
    assert it_h == counts
    it, hist, x = D.cg_block_loop(csr, Bm, 1000, threshold, stride=16)
    assert it == counts, it
    assert len(hist) == len(hist_h) == max(counts)
    assert np.array_equal(D.bits(np.array(hist)), D.bits(np.array(hist_h)))
    assert np.array_equal(x, x_h)


def test_model_loop_early_returns_and_max_itrs():
    csr, Bm = system()
    small = Bm[:, :2].copy()
    assert D.cg_block_loop(csr, small, 0, 1e-3)[:2] == ([0, 0], [])
    assert D.cg_block_loop(csr, 0.0 * small, 1000, 1e-3)[:2] == ([0, 0], [])
    it_h, hist_h, x_h = B.cg_block_loop(csr, small, 7, 1e-3)
    for stride in (1, 3, 16):
        it, hist, x = D.cg_block_loop(csr, small, 7, 1e-3, stride=stride)
        assert it == it_h == [7, 7] and np.array_equal(x, x_h), stride
        assert np.array_equal(D.bits(np.array(hist)), D.bits(np.array(hist_h))), stride


# ---- cg_solve_block_device on the stand-in ----
# DRec of test_device_loop_block_host.py with the protected calls: the blocks hold plain doubles (encode and scrub only
# leave their names in the call list), so the guarded protected iteration is the guarded plain one under its own name
STANDIN = BASE + r'''
import abft_sparse_cg_amd.context as C

class VDRec(DRec):
    info = "stream"
    def vecc_supported(self, mat):
        return self.info == "stream"
    def matrix_info(self, mat):
        return (self.info,)
    def encode_vector(self, v):
        assert self.rec is None
        self.calls.append(("encode", v.name))
    def scrub_vector(self, v):
        assert self.rec is None
        self.calls.append(("scrub", v.name)); return 0, 0
    def dot_block_vecc(self, a, b, k):
        self.calls.append(("dot_block_vecc", a.name, b.name, k)); return sums(a, b, k)
    def spmm_dot_vecc(self, A, x, y, k, drain=True):
        self.calls.append(("spmm_dot_vecc", drain)); self._mm(x, y, k); return sums(x, y, k)
    def calc_r_block_vecc(self, r, w, k, alpha, active):
        self.calls.append(("calc_r_block_vecc",)); return self._r(r, w, k, alpha, active, None)
    def calc_px_block_vecc(self, x, p, r, k, alpha, beta, active):
        self.calls.append(("calc_px_block_vecc",))
        self._x(x, p, k, alpha, active); self._p(p, r, k, beta, active, None)
    def cg_block_vecc_iteration_until_dev(self, A, X, R, P, W, k, sc, in_at, pw_at, out_at, thr):
        assert [v.name for v in (X, R, P, W)] == ["X", "R", "P", "W"]
        super().cg_block_iteration_until_dev(A, X, R, P, W, k, sc, in_at, pw_at, out_at, thr)
        assert self.calls[-1][0] == "block_until"
        self.calls[-1] = ("block_vecc_until", in_at, pw_at, out_at)

class Mat:
    fmt = C.FMT_CSR

def named(B):
    vs = vecs(B)
    for v, name in zip(vs, "BXRPW"):
        v.name = name
    return vs

def vhost(A, B, max_itrs, conv):
    s = VDRec(A)
    v = named(B)
    hist = []
    itrs, rr = cg_solve_block(s, Mat(), *v, max_itrs, conv, on_iteration=lambda i, r, a: hist.append((i, r, a)),
                              vector_ecc=True)
    return list(itrs), rr, v[1].a, hist

def vdevice(A, B, max_itrs, conv, stride, graph=True, **kw):
    s = VDRec(A)
    v = named(B)
    hist = []
    def cb(i, r, a):
        assert s.rec is None
        hist.append((i, r, a, s.downloads))
    kw.setdefault("vector_ecc", True)
    itrs, rr = cg_solve_block_device(s, Mat(), *v, max_itrs, conv, on_iteration=cb, stride=stride, graph=graph, **kw)
    return list(itrs), rr, v[1].a, hist, s

def expected_calls(k, T, max_itrs, stride, graph):
    """the documented call list of a solve with T live iterations"""
    rec = 2 * k + 2
    want = [("encode", "B"), ("encode", "X"), ("copy",), ("scrub", "R"), ("copy",), ("dot_block_vecc", "R", "R", k)]
    if T:
        batches = -(-T // stride) + (1 if T % stride == 0 and T < max_itrs else 0)
        captured = False
        for d in range(batches):
            m = min(stride, max_itrs - d * stride)
            if graph and m == stride:
                if captured:
                    continue                                        # replayed: no call
                want += [("reserve", k)]                            # before the capture
                captured = True
            want += [("copy",)] + [("block_vecc_until", rec * i, rec * (stride + 1), rec * (i + 1)) for i in range(m)]
        want += [("destroy",)] * 3
    return want + [("scrub", "X"), ("scrub", "B")]                  # the two scrubs come last
'''


def test_protected_block_device_loop_makes_exactly_the_documented_calls():
    out = child(STANDIN + r'''
k = 4
for max_itrs, conv in ((1000, 1e-20), (23, 1e-20), (1000, 1e-3)):
    it0, rr0, x0, h0 = vhost(PA, PB, max_itrs, conv)
    T = len(h0)
    assert T == max(it0) and T > 3
    for stride in (1, 3, 16):
        for graph in (True, False):
            it, rr, x, h, s = vdevice(PA, PB, max_itrs, conv, stride, graph)
            assert it == it0, (stride, it, it0)
            assert np.array_equal(bits(rr), bits(rr0)) and np.array_equal(bits(x), bits(x0)), stride
            assert [(i, a) for i, _, a, _ in h] == [(i, a) for i, _, a in h0], stride
            assert all(np.array_equal(bits(r), bits(r0)) for (_, r, _, _), (_, r0, _) in zip(h, h0)), stride
            assert all(d == i // stride + 1 for i, _, _, d in h), (stride, h)   # callbacks after their batch
            assert s.calls == expected_calls(k, T, max_itrs, stride, graph), (max_itrs, conv, stride, graph, s.calls)
            assert s.live == T
            if graph and s.launches:
                assert s.calls.index(("reserve", k)) == 6 and s.reserved == 1   # reserve before the capture
            if not graph:
                assert s.launches == 0 and s.reserved == 0
    print(max_itrs, conv, "iterations per column", it0)
it3 = vhost(PA, PB, 1000, 1e-3)[0]
assert it3[0] == 0 and len(set(it3)) >= 3                          # columns stop at different iterations
# the early returns: the start and the two scrubs, nothing else
for max_itrs, Bz in ((0, PB), (1000, np.zeros_like(PB))):
    for graph in (True, False):
        it, rr, x, h, s = vdevice(PA, Bz, max_itrs, 1e-3, 5, graph)
        assert it == [0] * 4 and h == [] and s.downloads == 0 and s.frozen == 0 and s.live == 0
        assert s.calls == expected_calls(k, 0, max_itrs, 5, graph), s.calls
        assert s.calls[-2:] == [("scrub", "X"), ("scrub", "B")] and len(s.calls) == 8
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_every_refusal_comes_before_any_call_and_leaves_the_arrays_untouched():
    out = child(STANDIN + r'''
class Dinv:
    pass
prot = Dinv(); prot.protected = True
PRECOND = "vector_ecc with a precond: the protected block loop has no Jacobi form"
LAYOUT = "vector_ecc needs a CSR matrix in the streaming layout (this one: %s)"
cases = [(dict(precond=Dinv()), PRECOND, "stream", C.FMT_CSR), (dict(precond=prot), PRECOND, "stream", C.FMT_CSR),
         (dict(), LAYOUT % "panels", "panels", C.FMT_CSR), (dict(), LAYOUT % "COO", "coo", C.FMT_CSR + 1),
         (dict(stride=0), "stride", "stream", C.FMT_CSR), (dict(stride=2.5), "stride", "stream", C.FMT_CSR)]
for kw, text, info, fmt in cases:
    s = VDRec(PA); s.info = info
    m = Mat(); m.fmt = fmt
    vs = named(PB)
    before = [v.a.copy() for v in vs]
    try:
        cg_solve_block_device(s, m, *vs, 1000, 1e-6, vector_ecc=True, **kw)
    except ValueError as e:
        assert text in str(e), (text, str(e))
    else:
        raise AssertionError(kw)
    assert s.calls == [], (kw, s.calls)
    assert all(np.array_equal(a, v.a) for a, v in zip(before, vs))
# the messages are cg_solve_block's
for kw, text, info in ((dict(precond=Dinv()), PRECOND, "stream"), (dict(), LAYOUT % "panels", "panels")):
    s = VDRec(PA); s.info = info
    try:
        cg_solve_block(s, Mat(), *named(PB), 1000, 1e-6, vector_ecc=True, **kw)
    except ValueError as e:
        assert str(e) == text, str(e)
    else:
        raise AssertionError(kw)
# without vector_ecc a protected precond keeps its refusal and its message
for kw in (dict(), dict(vector_ecc=False)):
    s = VDRec(PA)
    try:
        cg_solve_block_device(s, Mat(), *named(PB), 1000, 1e-6, precond=prot, **kw)
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
for pre in (False, True):
    for stride, graph in ((1, True), (5, True), (5, False), (16, True)):
        runs = []
        for kw in (None, dict(vector_ecc=False)):
            s = VDRec(PA)
            v = named(PB)
            args = dict(on_iteration=None, stride=stride, graph=graph, precond=dinv_of(PA, pre))
            if kw is None:
                res = cg_solve_block_device(s, None, *v, 1000, 1e-10, **args)
            else:
                res = cg_solve_block_device(s, None, *v, 1000, 1e-10, **args, **kw)
            runs.append((s.calls, list(res[0]), res[1], [u.a.copy() for u in v]))
        a, b = runs
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(bits(a[2]), bits(b[2]))
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[3], b[3]))
        names = {c[0] for c in a[0]}
        assert "block_until" in names and not names & {"encode", "scrub", "dot_block_vecc", "block_vecc_until"}, names
# and the plain loop's own stand-in gives the same list: the keyword adds no call
it, rr, x, h, s0 = device(PA, PB, False, 1000, 1e-10, 5, True)
s = VDRec(PA)
cg_solve_block_device(s, None, *named(PB), 1000, 1e-10, stride=5, graph=True, vector_ecc=False)
assert s.calls == s0.calls
print("ok")
''')
    assert out.strip() == "ok", out
