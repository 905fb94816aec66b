"""Block right-hand sides on the GPU (abft_hip_spmm, abft_hip_dot_block, abft_hip_calc_xr_block,
abft_hip_calc_p_block, cg_solve_block, the CLI's --rhs): every column of a block result is checked
against the single-vector call on that column, and against the CPU oracle.

    spmm           column j bit-identical to spmv of column j, and to OracleMatrix.spmv
    events         one spmm queues what one spmv queues on a twin matrix; the same repairs
    vector calls   active columns bit-identical to calc_xr / calc_p, inactive ones untouched
    CG             per column the iterations and residuals of cg_solve
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _oracle import CSR, MODES, OracleMatrix, laplace5, ora_dot, random_spd, rhs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 3, 4, 8)


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def holes(n=500, seed=4):
    """square, with empty rows inside and a run of empty rows at the end"""
    cols, rows, vals, _ = random_spd(n, 8, seed)
    keep = (rows % 7 != 3) & (rows < n - 60)
    return cols[keep], rows[keep], vals[keep], n


def long_row(n=4000):
    """a diagonal plus one row longer than an LDS tile (1024 elements) and one just over it"""
    rng = np.random.default_rng(9)
    rows, cols = [], []
    for r in range(n):
        c = {r}
        if r == 5:
            c |= set(range(0, 3000))
        if r == 1200:
            c |= set(int(v) for v in rng.choice(n, 1030, replace=False))
        c = sorted(c)
        rows += [r] * len(c)
        cols += c
    vals = rng.standard_normal(len(rows)) * 10.0 ** rng.integers(-3, 4, size=len(rows))
    return np.array(cols, np.uint32), np.array(rows, np.uint32), vals, n


MATS = {
    "lap": lambda: laplace5(30, 17),
    "rnd": lambda: random_spd(400, 12, seed=3),
    "holes": holes,
    "long": long_row,
}


class Twin:
    """one context; the matrix in the streaming layout; block vectors of K columns and single vectors"""

    def __init__(self, amd, mode, cols, rows, vals, n):
        self.events, self.fatal = [], False
        self.ctx = amd.HIPContext(mode, "csr", on_event=self._on)
        self.n = n
        self.A = self.ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        self.vx, self.vy = self.ctx.create_vector(n), self.ctx.create_vector(n)
        self.blocks = {}

    def _on(self, ev, fatal):
        self.events += ev
        self.fatal |= fatal

    def block(self, k):
        if k not in self.blocks:
            self.blocks[k] = (self.ctx.create_block(self.n, k), self.ctx.create_block(self.n, k))
        return self.blocks[k]

    def spmm(self, X):
        k = X.shape[1]
        bx, by = self.block(k)
        self.ctx.upload(bx, X)
        self.ctx.upload(by, np.full((self.n, k), np.nan))
        self.ctx.spmm(self.A, bx, by, k)
        return self.ctx.download(by)

    def spmv(self, x):
        self.ctx.upload(self.vx, x)
        self.ctx.upload(self.vy, np.full(self.n, np.nan))
        self.ctx.spmv(self.A, self.vx, self.vy)
        y = self.ctx.download(self.vy)
        self.ctx._drain()
        return y

    def take_events(self):
        self.ctx._drain()
        ev, f = self.events, self.fatal
        self.events, self.fatal = [], False
        return ev, f

    def close(self):
        self.ctx.close()


def block_x(n, k, seed=10):
    return np.stack([rhs(n, seed + j) - 0.5 for j in range(k)], axis=1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mat", sorted(MATS))
def test_spmm_columns_are_spmv_bit_for_bit(amd, mode, mat):
    cols, rows, vals, n = MATS[mat]()
    o = OracleMatrix(CSR, mode, cols, rows, vals, n)
    t = Twin(amd, mode, cols, rows, vals, n)
    try:
        assert t.ctx.matrix_info(t.A)[0] == "stream"
        for k in KS:
            X = block_x(n, k)
            Y = t.spmm(X)
            assert Y.shape == (n, k)
            for j in range(k):
                y1 = t.spmv(X[:, j])
                assert bits_equal(Y[:, j], y1), (mat, mode, k, j)
                assert bits_equal(Y[:, j], o.spmv(X[:, j])), (mat, mode, k, j)
        assert t.take_events() == ([], False)
    finally:
        t.close()


@pytest.mark.parametrize("mat", ["lap", "long"])
def test_spmm_after_index_flips_in_none(amd, mat):
    """mode none: a flipped column bit is never seen -- a column >= n_in takes x as 0.0, one inside
    multiplies the wrong entry -- exactly as in spmv and the reference"""
    cols, rows, vals, n = MATS[mat]()
    o = OracleMatrix(CSR, "none", cols, rows, vals, n)
    t = Twin(amd, "none", cols, rows, vals, n)
    try:
        nnz = len(vals)
        for i, bit in ((3, 64 + 31), (nnz // 2, 64 + 20), (nnz // 3, 64 + 1), (nnz - 1, 64 + 27), (17, 64 + 4)):
            o.inject(i, [bit])
            t.ctx.inject_at(t.A, i, [bit])
        for k in (3, 4, 8):
            X = block_x(n, k, seed=30)
            Y = t.spmm(X)
            for j in range(k):
                assert bits_equal(Y[:, j], t.spmv(X[:, j])), (k, j)
                assert bits_equal(Y[:, j], o.spmv(X[:, j])), (k, j)
    finally:
        t.close()


def twin_run(amd, mode, mat, flips, k=4, rowptr=()):
    """the same flips on two matrices: one spmm on the first, one spmv on the second ->
    (spmm events, spmv events, spmm stored words, spmv stored words, Y, y, oracle events)"""
    from abft_sparse_cg_amd import capi
    cols, rows, vals, n = MATS[mat]()
    a, b = Twin(amd, mode, cols, rows, vals, n), Twin(amd, mode, cols, rows, vals, n)
    o = OracleMatrix(CSR, mode, cols, rows, vals, n)
    try:
        for i, bits in flips:
            a.ctx.inject_at(a.A, i, bits)
            b.ctx.inject_at(b.A, i, bits)
            o.inject(i, bits)
        for row, mask in rowptr:
            capi.check(a.ctx.L.abft_hip_inject_rowptr(a.A.h, row, mask))
            capi.check(b.ctx.L.abft_hip_inject_rowptr(b.A.h, row, mask))
            o._view("ora_matrix_csr_rowptr", np.uint32, n + 1)[row] ^= np.uint32(mask)
        X = block_x(n, k, seed=50)
        Y = a.spmm(X)
        y = b.spmv(X[:, 0])
        o.spmv(X[:, 0])
        ea, eb = a.take_events(), b.take_events()
        return ea, eb, a.ctx.stored_words(a.A), b.ctx.stored_words(b.A), Y, y, o.events(), o
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("mode", ["sec7", "sec8", "secded"])
@pytest.mark.parametrize("mat", ["rnd", "long"])
def test_spmm_repairs_once_with_spmvs_events(amd, mode, mat):
    nnz = len(MATS[mat]()[2])
    flips = [(0, [5]), (nnz // 3, [70]), (nnz // 2, [40]), (nnz - 2, [95]), (nnz - 1, [64])]
    if mode != "sec7":
        flips.append((nnz // 5, [88]))  # an ECC bit
    ea, eb, wa, wb, Y, y, eo, o = twin_run(amd, mode, mat, flips)
    assert ea == eb == eo, (ea, eb, eo)
    assert not ea[1] and len(ea[0]) == len(flips)
    assert np.array_equal(wa, wb) and np.array_equal(wa, o.stored_words())
    assert bits_equal(Y[:, 0], y)


@pytest.mark.parametrize("mode,bits,kind", [("sed", [33], 1), ("secded", [3, 40], 4)])
def test_spmm_fatal_ecc_events(amd, mode, bits, kind):
    nnz = len(MATS["rnd"]()[2])
    ea, eb, wa, wb, Y, y, eo, _ = twin_run(amd, mode, "rnd", [(nnz // 2, bits)])
    assert ea == eb == eo and ea[1] and ea[0][0][0] == kind
    assert np.array_equal(wa, wb)
    # the fatal element's product is +0.0 in every column: the rest of Y is still spmv's
    assert bits_equal(Y[:, 0], y)
    # without an event handler the fatal line ends the call, as the reference's exit(1)
    cols, rows, vals, n = MATS["rnd"]()
    ctx = amd.HIPContext(mode, "csr")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        X, Yb = ctx.create_block(n, 3), ctx.create_block(n, 3)
        ctx.upload(X, block_x(n, 3))
        ctx.inject_at(A, nnz // 2, bits)
        with pytest.raises(amd.FatalEvent):
            ctx.spmm(A, X, Yb, 3)
    finally:
        ctx.close()


def test_spmm_constraints_events(amd):
    """row-pointer checks (inject_rowptr) and column size / order checks (index flips): one spmm
    queues the lines one spmv queues"""
    cols, rows, vals, n = MATS["rnd"]()
    nnz = len(vals)
    seen = set()
    for rp in ((7, 1 << 30), (7, 1 << 3), (1, 1 << 5), (n, 1 << 29), (60, 1 << 9), (119, 1 << 1)):
        ea, eb, _, _, Y, y, eo, _ = twin_run(amd, "constraints", "rnd", [], rowptr=[rp])
        assert ea == eb, (rp, ea, eb)
        if eo[1] and eo[0][0][0] in (5, 6):
            assert ea[0][:1] == eo[0][:1]
        seen |= {e[0] for e in ea[0]}
    for flips in ([(nnz // 2, [64 + 30])], [(40, [64 + 3])], [(nnz // 4, [64 + 0]), (nnz - 3, [64 + 2])], [(100, [64 + 8])]):
        for mat in ("rnd", "long"):
            ea, eb, _, _, Y, y, eo, _ = twin_run(amd, "constraints", mat, flips)
            assert ea == eb, (flips, ea, eb)
            if eo[1]:
                assert ea[1] and ea[0][:1] == eo[0][:1], (flips, ea, eo)
            seen |= {e[0] for e in ea[0]}
    assert {5, 6, 7, 8} <= seen, seen


@pytest.mark.parametrize("n", [1000, 1001])
def test_block_vector_calls_against_the_single_ones(amd, n):
    ctx = amd.HIPContext("none", "csr")
    try:
        s = [ctx.create_vector(n) for _ in range(4)]
        for k in KS:
            rng = np.random.default_rng(k)
            x, r, p, w = (rng.standard_normal((n, k)) for _ in range(4))
            alpha = rng.standard_normal(k)
            beta = rng.standard_normal(k)
            active = sum(1 << j for j in range(k) if j % 3 != 1) if k > 1 else 1
            off = [j for j in range(k) if not (active >> j) & 1]
            for j in off:  # an inactive column keeps whatever it holds, bit for bit
                x[::7, j] = np.inf
                p[::5, j] = np.nan
                r[3, j] = -np.inf
            B = [ctx.create_block(n, k) for _ in range(4)]
            for v, a in zip(B, (x, r, p, w)):
                ctx.upload(v, a)
            # dot_block: within 1e-13 of the serial sum; power-of-two columns scale exactly
            d = ctx.dot_block(B[2], B[3], k)
            for j in range(k):
                if j not in off:
                    ref = ora_dot(p[:, j], w[:, j])
                    assert abs(d[j] - ref) <= 1e-13 * float(np.abs(p[:, j] * w[:, j]).sum()), (k, j)
            two = np.stack([w[:, 0] * 2.0 ** j for j in range(k)], axis=1)
            ctx.upload(B[3], two)
            d2 = ctx.dot_block(B[3], B[3], k)
            assert all(d2[j] == d2[0] * 4.0 ** j for j in range(k)), d2
            ctx.upload(B[3], w)
            rr = ctx.calc_xr_block(B[0], B[1], B[2], B[3], k, alpha, active)
            xb, rb = ctx.download(B[0]), ctx.download(B[1])
            ctx.calc_p_block(B[2], B[1], k, beta, active)
            pb = ctx.download(B[2])
            for j in range(k):
                if j in off:
                    assert bits_equal(xb[:, j], x[:, j]) and bits_equal(rb[:, j], r[:, j]) and bits_equal(pb[:, j], p[:, j])
                    assert np.isinf(rr[j]) or np.isnan(rr[j])
                    continue
                for v, a in zip(s, (x[:, j], r[:, j], p[:, j], w[:, j])):
                    ctx.upload(v, a)
                rr1 = ctx.calc_xr(s[0], s[1], s[2], s[3], alpha[j])
                ctx.calc_p(s[2], s[1], beta[j])
                assert bits_equal(xb[:, j], ctx.download(s[0])), (k, j)
                assert bits_equal(rb[:, j], ctx.download(s[1])), (k, j)
                assert bits_equal(pb[:, j], ctx.download(s[2])), (k, j)
                ref = ora_dot(rb[:, j], rb[:, j])
                assert abs(rr[j] - ref) <= 1e-13 * ref and abs(rr1 - ref) <= 1e-13 * ref
            for v in B:
                ctx.destroy_vector(v)
    finally:
        ctx.close()


def solve_both(amd, cols, rows, vals, n, k, itrs, mode="none"):
    """cg_solve_block on k columns and cg_solve on each column alone, conv 0 -> (block run, single runs)"""
    ctx = amd.HIPContext(mode, "csr")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        Bh = np.stack([rhs(n, 1 + j) for j in range(k)], axis=1)
        V = [ctx.create_block(n, k) for _ in range(5)]
        ctx.upload(V[0], Bh)
        ctx.upload(V[1], np.zeros((n, k)))
        hist = []
        it, rr = amd.cg_solve_block(ctx, A, *V, max_itrs=itrs, conv_threshold=0.0,
                                    on_iteration=lambda i, r, act: hist.append(r))
        single = []
        v = [ctx.create_vector(n) for _ in range(5)]
        for j in range(k):
            ctx.upload(v[0], Bh[:, j])
            ctx.upload(v[1], np.zeros(n))
            h1 = []
            it1, rr1 = amd.cg_solve(ctx, A, *v, max_itrs=itrs, conv_threshold=0.0, on_iteration=lambda i, r: h1.append(r))
            single.append((it1, h1))
        return it, np.array(hist), single
    finally:
        ctx.close()


@pytest.mark.parametrize("mat", ["lap", "rnd"])
def test_cg_solve_block_follows_cg_solve(amd, mat):
    """40 iterations at -c 0: the same count per column, residuals within 1e-10 relative.  The
    strongly diagonally dominant random_spd converges by a factor ~10 per iteration and its recursive
    residual is far below the rounding floor of the solution after ~20 iterations (r.r under 1e-20
    of the start: residual norms under 1e-10 relative); from there on both runs carry rounding
    noise only, and the residuals are compared down to that floor."""
    cols, rows, vals, n = MATS[mat]()
    it, hist, single = solve_both(amd, cols, rows, vals, n, 4, 40)
    for j, (it1, h1) in enumerate(single):
        assert it[j] == it1 == 40
        h1 = np.array(h1)
        m = h1 >= h1[0] * 1e-20
        assert mat == "rnd" or m.all()
        assert m.sum() >= 15
        assert np.all(np.abs(hist[m, j] - h1[m]) <= 1e-10 * np.abs(h1[m])), (j, hist[:, j], h1)


def test_cg_solve_block_power_of_two_columns(amd):
    """B[:, j] = 2^j b: every operation scales exactly, so column j's residuals are column 0's times
    4^j bit for bit, its stop iteration under a threshold is predicted from column 0's history, and
    X[:, j] == 2^j X[:, 0]"""
    cols, rows, vals, n = laplace5(40, 33)
    k = 4
    b = rhs(n, 1)
    ctx = amd.HIPContext("secded", "csr")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        V = [ctx.create_block(n, k) for _ in range(5)]
        B = np.stack([b * 2.0 ** j for j in range(k)], axis=1)

        def run(conv, itrs):
            ctx.upload(V[0], B)
            ctx.upload(V[1], np.zeros((n, k)))
            hist = []
            it, _ = amd.cg_solve_block(ctx, A, *V, max_itrs=itrs, conv_threshold=conv,
                                       on_iteration=lambda i, r, act: hist.append(r))
            return it, np.array(hist), ctx.download(V[1])

        it, hist, X = run(0.0, 60)
        assert it == [60] * k
        for j in range(k):
            assert np.array_equal(hist[:, j], hist[:, 0] * 4.0 ** j)
            assert bits_equal(X[:, j], X[:, 0] * 2.0 ** j)
        ctx.upload(V[0], B)
        rr0 = float(ctx.dot_block(V[0], V[0], k)[0])
        h0 = np.concatenate([[rr0], hist[:, 0]])
        conv = float(np.sqrt(h0[20] * h0[21]))  # between two of column 0's residuals
        it, _, _ = run(conv, 60)
        for j in range(k):
            scaled = h0 * 4.0 ** j
            want = next((m for m in range(61) if m == 60 or scaled[m] <= conv), 60)
            assert it[j] == want, (j, it, want)
        assert len(set(it)) > 1
    finally:
        ctx.close()


def test_fullsize_config2_spmm_secded_after_a_flip(amd):
    from abft_sparse_cg_amd import generators
    cols, rows, vals, n = generators.generate("laplace5:3162,3162")
    k = 4
    o = OracleMatrix(CSR, "secded", cols, rows, vals, n)
    events = []
    ctx = amd.HIPContext("secded", "csr", on_event=lambda ev, fatal: events.extend(ev))
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        idx = len(vals) // 2 + 12345
        ctx.inject_at(A, idx, [71])
        o.inject(idx, [71])
        X, Y = ctx.create_block(n, k), ctx.create_block(n, k)
        Xh = block_x(n, k, seed=3)
        ctx.upload(X, Xh)
        ctx.spmm(A, X, Y, k)
        Yh = ctx.download(Y)
        for j in range(k):
            assert bits_equal(Yh[:, j], o.spmv(Xh[:, j], threads=16)), j
        assert events == o.events()[0][:1] == [(2, idx, 71)]
    finally:
        ctx.close()


def test_fullsize_config4_stream_layout_cg(amd):
    from abft_sparse_cg_amd import generators
    cols, rows, vals, n = generators.generate("random:4194304,24,1")
    it, hist, single = solve_both(amd, cols, rows, vals, n, 8, 8, mode="secded")
    for j, (it1, h1) in enumerate(single):
        assert it[j] == it1 == 8
        h1 = np.array(h1)
        assert np.all(np.abs(hist[:, j] - h1) <= 1e-10 * np.abs(h1)), (j, hist[:, j], h1)


def test_refusals(amd):
    cols, rows, vals, n = laplace5(20, 20)
    ctx = amd.HIPContext("sec7", "coo")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        X, Y = ctx.create_block(n, 2), ctx.create_block(n, 2)
        with pytest.raises(amd.AbftError) as e:
            ctx.spmm(A, X, Y, 2)
        assert "COO" in str(e.value) and "create_csr_stream" in str(e.value)
    finally:
        ctx.close()
    ctx = amd.HIPContext("sec7", "csr")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        for k in (0, 9):
            X, Y = ctx.create_vector(n * max(k, 1)), ctx.create_vector(n * max(k, 1))
            with pytest.raises(amd.AbftError) as e:
                ctx.spmm(A, X, Y, k)
            assert ("k = %d outside [1, 8]" % k) in str(e.value)
        X, Y = ctx.create_block(n, 3), ctx.create_block(n, 4)
        with pytest.raises(amd.AbftError) as e:
            ctx.spmm(A, X, Y, 3)
        assert "not a block of" in str(e.value)
    finally:
        ctx.close()
    # the sweep layout (forced), in a child process: spmm refuses it and names the stream create;
    # layout="stream" still gives the streaming layout there
    code = r'''
import sys
sys.path.insert(0, "tests")
import abft_sparse_cg_amd as amd
from _oracle import laplace5
cols, rows, vals, n = laplace5(40, 33)
ctx = amd.HIPContext("sec8", "csr")
A = ctx.create_matrix(cols, rows, vals, n, len(vals))
assert ctx.matrix_info(A)[0] == "sweep", ctx.matrix_info(A)
X, Y = ctx.create_block(n, 2), ctx.create_block(n, 2)
try:
    ctx.spmm(A, X, Y, 2)
except amd.AbftError as e:
    assert "sweep layout" in str(e) and "abft_hip_matrix_create_csr_stream" in str(e), str(e)
else:
    raise AssertionError("spmm ran on the sweep layout")
S = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
assert ctx.matrix_info(S)[0] == "stream"
ctx.spmm(S, X, Y, 2)
ctx.close()
print("ok")
'''
    env = dict(os.environ, ABFT_HIP_LAYOUT="sweep", ABFT_HIP_PANEL_WIDTH="16")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def cli(args):
    p = subprocess.run([sys.executable, "-m", "abft_sparse_cg_amd.cg", "-t", "hip", "-s", "laplace5:40,40",
                        "-i", "300", "-c", "1e-8"] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return re.sub(r"time taken = .*", "time taken", p.stdout)


def test_cli_rhs(amd):
    for mode in ("none", "secded"):
        base = cli(["-m", mode, "--flip-at", "100:7"])
        assert cli(["-m", mode, "--flip-at", "100:7", "--rhs", "1"]) == base
        out = cli(["-m", mode, "--flip-at", "100:7", "--rhs", "3"])
        single = [float(v) for v in re.findall(r"iteration +\d+ :  rr = +(\S+)", base)]
        lines = re.findall(r"iteration +\d+ :  rr = (.*)", out)
        assert all(len(l.split()) == 3 for l in lines)
        it0 = int(re.search(r"rhs 0: ran for (\d+) iterations", out).group(1))
        assert it0 == int(re.search(r"ran for (\d+) iterations", base).group(1)) == len(single)
        assert [float(l.split()[0]) for l in lines[:it0]] == single
        assert len(re.findall(r"rhs \d: total error", out)) == 3
        if mode == "secded":
            assert out.count("[ECC] corrected bit 7 at index 100") == 1
    p = subprocess.run([sys.executable, "-m", "abft_sparse_cg_amd.cg", "-t", "hip", "-s", "laplace5:10,10",
                        "--format", "coo", "--rhs", "2"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 1 and "--rhs" in p.stdout
