"""Residual checks with rollback on the GPU (abft_hip_vector_flip, abft_hip_residual_gap / _restart and
their block forms, abft_hip_copy_block, cg_solve / cg_solve_block with check_every, the CLI's
--check-every / --flip-vector):

    flip_vector      the exact bit effect, also on an x whose update is still deferred
    residual_gap     its SpMV half is spmv bit for bit, in every layout and mode; the two sums as numpy's
    residual_restart r = b - A x bit for bit, p = r, rr = dot(r, r) bit for bit; from x = 0 it is cg_solve's start
    clean runs       a check changes no bit of the rr history or of x
    detection        a flip in x or r is caught at the next check, rolled back and recovered from
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _oracle import CSR, OracleMatrix, laplace5, random_spd, rhs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("none", "constraints", "sed", "sec7", "sec8", "secded")
# laplace5(40, 40) with rhs(n, 1): the recurrence's rr passes 1e-25 where the true residual has reached its
# floor (3.5e-12, read off a clean solve); a clean solve to this threshold runs about 170 iterations
CONV = 1e-25


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def flipped(v, bits):
    u = np.array([v], dtype=np.float64).view(np.uint64)
    for b in bits:
        u ^= np.uint64(1) << np.uint64(b)
    return u.view(np.float64)[0]


def test_flip_vector_bits(amd):
    ctx = amd.HIPContext("none", "csr")
    try:
        n = 1001
        rng = np.random.default_rng(1)
        x, r, p, w = (ctx.create_vector(n) for _ in range(4))
        xs, rs, ps, ws = (rng.standard_normal(n) for _ in range(4))
        for v, a in ((x, xs), (r, rs), (p, ps), (w, ws)):
            ctx.upload(v, a)
        ctx.flip_vector(x, 0, [0])
        ctx.flip_vector(x, n - 1, [63, 52, 51])
        ctx.flip_vector(x, 17, [5, 5])  # twice: no change
        want = xs.copy()
        want[0] = flipped(xs[0], [0])
        want[n - 1] = flipped(xs[n - 1], [63, 52, 51])
        assert bits_equal(ctx.download(x), want)
        # right after a calc_xr whose x += alpha p waits for the next calc_p: the flip sees the updated x
        ctx.upload(x, xs)
        alpha = 0.37
        ctx.calc_xr(x, r, p, w, alpha)
        ctx.flip_vector(x, 300, [55])
        ctx.calc_p(p, r, 0.5)
        want = xs + alpha * ps
        want[300] = flipped(want[300], [55])
        assert bits_equal(ctx.download(x), want)
        for bad in ((-1, [1]), (n, [1]), (0, [64]), (0, [-1])):
            with pytest.raises(amd.AbftError):
                ctx.flip_vector(x, *bad)
    finally:
        ctx.close()


# the single and block checks on one matrix; run in a child so that the layout can be forced
PROBE = r'''
import sys
sys.path.insert(0, "tests")
import numpy as np
import abft_sparse_cg_amd as amd
from _oracle import laplace5, random_spd

def bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))

def close(a, b):
    return abs(a - b) <= 1e-12 * abs(b)

FMT, LAYOUT = sys.argv[1], sys.argv[2]
cols, rows, vals, n = laplace5(40, 33) if LAYOUT != "auto" else random_spd(3000, 12, 5)
rng = np.random.default_rng(3)
for mode in ("none", "constraints", "sed", "sec7", "sec8", "secded"):
    ctx = amd.HIPContext(mode, FMT)
    A = ctx.create_matrix(cols, rows, vals, n, len(vals))
    if LAYOUT == "sweep" and mode != "constraints":
        assert ctx.matrix_info(A)[0] == "sweep", ctx.matrix_info(A)
    b, x, r, p, w, y = (ctx.create_vector(n) for _ in range(6))
    bs, xs, rs = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    for v, a in ((b, bs), (x, xs), (r, rs)):
        ctx.upload(v, a)
    ctx.spmv(A, x, y)
    ys = ctx.download(y)
    g2, t2 = ctx.residual_gap(A, b, x, r, w)
    assert bits_equal(ctx.download(w), ys), mode
    t = bs - ys
    assert close(g2, float(np.sum((t - rs) ** 2))) and close(t2, float(np.sum(t * t))), (mode, g2, t2)
    ctx.upload(r, t)
    g2, t2 = ctx.residual_gap(A, b, x, r, w)
    assert g2 == 0.0 and close(t2, float(np.sum(t * t))), (mode, g2)
    ctx.upload(r, rs)
    rr = ctx.residual_restart(A, b, x, r, p, w)
    assert bits_equal(ctx.download(r), t) and bits_equal(ctx.download(p), t), mode
    assert rr == ctx.dot(r, r), mode
    assert ctx.event_log == [], (mode, ctx.event_log[:4])
    ctx.close()
print("ok")
'''


@pytest.mark.parametrize("fmt,layout", [("csr", "stream"), ("coo", "stream"), ("csr", "sweep"), ("csr", "auto")])
def test_residual_gap_and_restart_in_every_layout_and_mode(fmt, layout):
    env = dict(os.environ)
    if layout == "sweep":
        env.update(ABFT_HIP_LAYOUT="sweep", ABFT_HIP_PANEL_WIDTH="16")
    elif layout == "stream":
        env.update(ABFT_HIP_LAYOUT="stream")
    p = subprocess.run([sys.executable, "-c", PROBE, fmt, layout], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_restart_from_zero_is_cg_solves_start(amd):
    cols, rows, vals, n = laplace5(40, 40)
    ctx = amd.HIPContext("secded", "csr")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        b, x, r, p, w = (ctx.create_vector(n) for _ in range(5))
        ctx.upload(b, rhs(n, 1))
        ctx.upload(x, np.zeros(n))
        h0 = []
        it0, rr0 = amd.cg_solve(ctx, A, b, x, r, p, w, 60, 0.0, on_iteration=lambda i, v: h0.append(v))
        x0 = ctx.download(x)
        ctx.upload(x, np.zeros(n))
        rr = ctx.residual_restart(A, b, x, r, p, w)
        h = []
        for i in range(60):
            ctx.spmv(A, p, w)
            alpha = rr / ctx.dot(p, w)
            rr_new = ctx.calc_xr(x, r, p, w, alpha)
            ctx.calc_p(p, r, rr_new / rr)
            rr = rr_new
            h.append(rr)
        assert h == h0 and bits_equal(ctx.download(x), x0)
    finally:
        ctx.close()


def test_block_forms(amd):
    cols, rows, vals, n = laplace5(37, 23)
    k = 3
    ctx = amd.HIPContext("sec8", "csr")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        B, X, R, P, W, Y = (ctx.create_block(n, k) for _ in range(6))
        rng = np.random.default_rng(8)
        Bs, Xs, Rs, Ps = (rng.standard_normal((n, k)) for _ in range(4))
        Rs[5, 1], Ps[6, 1] = np.nan, np.inf  # an unmasked column keeps even these bits
        for v, a in ((B, Bs), (X, Xs), (R, Rs), (P, Ps)):
            ctx.upload(v, a)
        ctx.spmm(A, X, Y, k)
        Ys = ctx.download(Y)
        Ts = Bs - Ys
        g2, t2 = ctx.residual_gap_block(A, B, X, R, W, k, 0b011)
        assert bits_equal(ctx.download(W), Ys)
        for j in (0, 1):
            want_g = float(np.sum((Ts[:, j] - Rs[:, j]) ** 2)) if j == 0 else None
            if j == 0:
                assert abs(g2[j] - want_g) <= 1e-12 * want_g
            else:
                assert np.isnan(g2[j])  # the NaN in R[:, 1]
            assert abs(t2[j] - float(np.sum(Ts[:, j] ** 2))) <= 1e-12 * t2[j]
        assert g2[2] == 0.0 and t2[2] == 0.0  # inactive
        rr = ctx.residual_restart_block(A, B, X, R, P, W, k, 0b101)
        Rn, Pn = ctx.download(R), ctx.download(P)
        for j in (0, 2):
            assert bits_equal(Rn[:, j], Ts[:, j]) and bits_equal(Pn[:, j], Ts[:, j]), j
        assert bits_equal(Rn[:, 1], Rs[:, 1]) and bits_equal(Pn[:, 1], Ps[:, 1])
        assert bits_equal(rr, ctx.dot_block(R, R, k))
        # the gap of a column set to B - A X is exactly 0
        g2, _ = ctx.residual_gap_block(A, B, X, R, W, k, 0b101)
        assert g2[0] == 0.0 and g2[2] == 0.0
        # copy_block: masked columns copied bit for bit (NaN / inf included), the others untouched
        D = ctx.create_block(n, k)
        Ds = rng.standard_normal((n, k))
        ctx.upload(D, Ds)
        ctx.copy_block(D, P, k, 0b010)
        Dn = ctx.download(D)
        assert bits_equal(Dn[:, 1], Ps[:, 1]) and bits_equal(Dn[:, [0, 2]], Ds[:, [0, 2]])
        with pytest.raises(amd.AbftError):
            ctx.residual_gap_block(A, B, X, R, X, k, 1)  # scratch = an operand
    finally:
        ctx.close()


def solve(amd, ctx, A, n, b, conv, itrs, flips=(), **kw):
    """-> (itr, history, x, checks); flips: (iteration, 'x' | 'r', index, bits)"""
    vb, x, r, p, w = (ctx.create_vector(n) for _ in range(5))
    vecs = {"x": x, "r": r}
    ctx.upload(vb, b)
    ctx.upload(x, np.zeros(n))
    hist, checks = [], []

    def on_it(i, rr):
        hist.append(rr)
        for fi, name, idx, bits in flips:
            if fi == i:
                ctx.flip_vector(vecs[name], idx, bits)

    it, _ = amd.cg_solve(ctx, A, vb, x, r, p, w, itrs, conv, on_iteration=on_it,
                         on_check=lambda *c: checks.append(c), **kw)
    xs = ctx.download(x)
    for v in (vb, x, r, p, w):
        ctx.destroy_vector(v)
    return it, hist, xs, checks


@pytest.mark.parametrize("case", ["lap-csr", "rnd-csr", "rnd-coo", "lap-secded-flip"])
def test_clean_runs_change_nothing(amd, case):
    mat, fmt = case.split("-")[:2]
    mode = "secded" if case.endswith("flip") else "none"
    fmt = "csr" if fmt == "secded" else fmt
    cols, rows, vals, n = laplace5(40, 40) if mat == "lap" else random_spd(2000, 10, 7)
    ctx = amd.HIPContext(mode, fmt, on_event=lambda ev, fatal: None)
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        if case.endswith("flip"):
            ctx.inject_at(A, 1000, [37])  # corrected by the first SpMV
        b = rhs(n, 1)
        it0, h0, x0, _ = solve(amd, ctx, A, n, b, 1e-20, 400)
        for ce in (1, 7, 50):
            it, h, x, checks = solve(amd, ctx, A, n, b, 1e-20, 400, check_every=ce)
            assert it == it0 and h == h0 and bits_equal(x, x0), ce
            assert checks and all(c[2] for c in checks), ce
    finally:
        ctx.close()


def true_res(o, b, x):
    return float(np.linalg.norm(b - o.spmv(x)))


@pytest.mark.parametrize("vec", ["x", "r"])
def test_detection_and_recovery(amd, vec):
    cols, rows, vals, n = laplace5(40, 40)
    o = OracleMatrix(CSR, "none", cols, rows, vals, n)
    b = rhs(n, 1)
    ctx = amd.HIPContext("none", "csr")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        it0, h0, x0, _ = solve(amd, ctx, A, n, b, CONV, 1000)
        clean = true_res(o, b, x0)
        i = n // 2 + 7
        for bit in (62, 55, 52, 51, 45):
            flips = [(10, vec, i, [bit])]
            it, h, x, checks = solve(amd, ctx, A, n, b, CONV, 1000, flips)
            assert it < 1000 and checks == []
            assert not true_res(o, b, x) < 1e3 * clean, (vec, bit, true_res(o, b, x), clean)  # NaN counts as wrong
            # the check after iteration 14 -- or, once rr is not finite, the one before the loop stops
            at = 14 if len(h) > 14 else len(h) - 1
            it, h, x, checks = solve(amd, ctx, A, n, b, CONV, 1000, flips, check_every=5)
            fails = [c for c in checks if not c[2]]
            assert [(c[0], c[3]) for c in fails] == [(at, 9)], (vec, bit, checks)
            assert h[:10] == h0[:10] and checks[-1][2]
            assert true_res(o, b, x) <= 10 * clean, (vec, bit, true_res(o, b, x), clean)
    finally:
        ctx.close()


def test_block_detection_touches_one_column(amd):
    cols, rows, vals, n = laplace5(40, 40)
    o = OracleMatrix(CSR, "none", cols, rows, vals, n)
    k = 3
    Bs = np.stack([rhs(n, 1 + j) for j in range(k)], axis=1)
    ctx = amd.HIPContext("none", "csr")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")

        def run(flips=(), **kw):
            B, X, R, P, W = (ctx.create_block(n, k) for _ in range(5))
            ctx.upload(B, Bs)
            ctx.upload(X, np.zeros((n, k)))
            hist, checks = [], []

            def on_it(i, rr, act):
                hist.append((rr, act))
                for fi, idx, bits in flips:
                    if fi == i:
                        ctx.flip_vector(X, idx, bits)

            itrs, _ = amd.cg_solve_block(ctx, A, B, X, R, P, W, 1000, CONV, on_iteration=on_it,
                                         on_check=lambda *c: checks.append(c), **kw)
            Xs = ctx.download(X)
            for v in (B, X, R, P, W):
                ctx.destroy_vector(v)
            return itrs, hist, Xs, checks

        itrs0, hist0, X0, _ = run()
        itrs, hist, X, checks = run(flips=[(10, (n // 2 + 7) * k + 1, [55])], check_every=5)
        fails = [c for c in checks if not c[2]]
        assert [(c[0], c[3], c[4]) for c in fails] == [(14, 9, 1)], fails
        for j in (0, 2):
            assert itrs[j] == itrs0[j] and bits_equal(X[:, j], X0[:, j]), j
            assert [h[0][j] for h in hist if (h[1] >> j) & 1] == [h[0][j] for h in hist0 if (h[1] >> j) & 1], j
        assert true_res(o, Bs[:, 1], np.ascontiguousarray(X[:, 1])) <= 10 * true_res(o, Bs[:, 1], np.ascontiguousarray(X0[:, 1]))
    finally:
        ctx.close()


def cli(args, rc=0):
    p = subprocess.run([sys.executable, "-m", "abft_sparse_cg_amd.cg", "-t", "hip", "-s", "laplace5:40,40",
                        "-i", "300", "-c", "1e-8"] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == rc, p.stdout + p.stderr
    return re.sub(r"time taken = .*", "time taken", p.stdout)


def total_error(out):
    return float(re.search(r"total error = (\S+)", out).group(1))


def test_cli(amd):
    base = cli([])
    assert cli(["--check-every", "0"]) == base
    clean = total_error(base)
    out = cli(["--check-every", "5", "--flip-vector", "10:x:123:55"])
    fails = re.findall(r"\[ABFT\] residual check failed at iteration (\d+): gap \S+ > \S+; rolled back to iteration (\d+)", out)
    assert fails == [("14", "9")], out
    assert "*** flipping bit 55 of x[123] ***" in out
    assert re.search(r"residual checks: \d+ passed, 1 failed", out)
    assert total_error(out) <= 10 * clean + 1e-6, (total_error(out), clean)
    bad = cli(["--flip-vector", "10:x:123:55"])
    assert "residual check" not in bad and total_error(bad) > 1e3 * clean
    # block: INDEX = row * K + column; only that column is rolled back
    out = cli(["--rhs", "2", "--check-every", "5", "--flip-vector", "10:x:247:55"])
    assert re.findall(r"rhs (\d): \[ABFT\] residual check failed at iteration 14", out) == ["1"], out
    # a check that cannot pass: exit 1 with the exception's message
    out = cli(["--check-every", "5", "--check-tol", "1e-300", "--max-rollbacks", "1"], rc=1)
    assert "[ABFT] residual check failed" in out and "after 1 rollbacks" in out
    assert "Invalid --flip-vector" in cli(["--flip-vector", "1:x:1600:3"], rc=1)


def test_fullsize_config2(amd):
    from abft_sparse_cg_amd import generators
    cols, rows, vals, n = generators.generate("laplace5:3162,3162")
    ctx = amd.HIPContext("secded", "csr", on_event=lambda ev, fatal: None)
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        del cols, rows, vals
        b = generators.reference_rhs(n)
        it0, h0, x0, _ = solve(amd, ctx, A, n, b, 0.0, 200)
        it, h, x, checks = solve(amd, ctx, A, n, b, 0.0, 200, check_every=50)
        assert it == it0 == 200 and h == h0 and bits_equal(x, x0)
        assert [c[0] for c in checks] == [49, 99, 149, 199] and all(c[2] for c in checks)
        it, h, x, checks = solve(amd, ctx, A, n, b, 0.0, 200, flips=[(120, "x", n // 2, [55])], check_every=50)
        assert [(c[0], c[2], c[3]) for c in checks] == [(49, True, None), (99, True, None), (149, False, 99),
                                                        (199, True, None)], checks
        assert h[:121] == h0[:121]
    finally:
        ctx.close()
