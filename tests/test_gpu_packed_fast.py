"""The predicate-free path of the CSR SpMV on packed row blocks the planner has proven safe (ABFT_HIP_PACKED_FAST;
CsrPackedFast, DESIGN.md sections 3 and 4): every case runs the same calls on two contexts, the switch at 1 and at 0,
and compares bit for bit (NaN payloads apart: `same`) -- y and the fused p.w of one SpMV on a vector of special values, and after a few iterations
of the host-scalar loop (chosen alpha and beta: nothing needs to converge) x, r, p, w and every scalar handed back.
abft_hip_packed_stats says which path ran: on these fixtures some packed blocks are fast and some are not, so one
launch crosses both.  No test touches the device's codes: that every code value stays in range on a fast block is
tests/test_packed_fast_host.py's enumeration."""
import os

import numpy as np
import pytest

from _ieee import INF, MAX_SUB, NEG_QNAN, QNAN, TINY, ieee_diff, ieee_equal
from _oracle import laplace5

pytestmark = pytest.mark.gpu

K = 6  # loop iterations: three bursts at ABFT_HIP_LAZY_X=2, one at 4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def band16(length, odd=False, n=12000, nv=16):
    """n x n, rows of `length` consecutive columns from the row's own (clamped into the matrix), 16 values: shift 12, so
    the blocks with cbase + 4096 <= n are stage-fast.  odd: a one-element first row, so later blocks start at odd
    elements.  The palette holds -0.0 and a subnormal beside ordinary values.  nv: only its first nv values (8: shift 13)."""
    pal = np.array([4.0, -1.0, 0.5, -0.0, 2.0, -3.0, MAX_SUB, 7.0, -0.25, 1.5, 9.0, -6.0, 0.125, 3.0, -8.0, 5.0])
    lens = np.full(n, length, np.int64)
    if odd:
        lens[0] = 1
    rows = np.repeat(np.arange(n), lens)
    j = np.arange(len(rows)) - np.repeat(np.cumsum(lens) - lens, lens)
    first = np.minimum(np.arange(n), n - lens)
    cols = first[rows] + j
    vals = pal[(rows + 3 * j) % nv]
    return cols.astype(np.uint32), rows.astype(np.uint32), vals, n


def small_columns_last(n=67600, tail=300):
    """two values, rows of 3; the last `tail` rows hold columns 0 ..: their window of columns is fine, but the last
    block's tile would reach past the codes -- the one block where only the allocation condition fails"""
    lens = np.full(n, 3, np.int64)
    rows = np.repeat(np.arange(n), lens)
    j = np.arange(len(rows)) % 3
    first = np.where(np.arange(n) >= n - tail, np.arange(n) - (n - tail), np.arange(n) * (n - 40000) // n)
    cols = first[rows] + j
    vals = np.where(j == 1, 4.0, -1.0)
    return cols.astype(np.uint32), rows.astype(np.uint32), vals, n


def special_x(n, seed):
    """ordinary values with +-0.0, NaN, +-Inf and subnormals sprinkled in, a run of -0.0 (whole rows of a band then
    hold only -0.0 and +0.0 products: the sum must come out +0.0) and a run of alternating zeros"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    kinds = np.array([0.0, -0.0, QNAN, NEG_QNAN, INF, -INF, TINY, -TINY, MAX_SUB, -MAX_SUB])
    hit = rng.random(n) < 0.05
    x[hit] = rng.choice(kinds, size=int(hit.sum()))
    for start in (40, n // 2 + 1, n - 90):
        x[start:start + 24] = -0.0
        x[start + 24:start + 48:2] = 0.0
        x[start + 25:start + 48:2] = -0.0
        x[start + 48:start + 52] = [1.0, -0.0, 1.0, 1.0]  # a lone -0.0 between ordinary entries
    return x


class env:
    def __init__(self, **kw):
        self.kw, self.old = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = os.environ.get(k)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def play(mat, fast, lazy=None, xin=None, injects=(), iters=K, seed=5):
    """one context: the counters, one SpMV with the fused product on a vector of special values, then `iters`
    iterations of the host-scalar loop on ordinary vectors; `injects`: (element, bits) applied before anything runs"""
    import abft_sparse_cg_amd as amd
    from abft_sparse_cg_amd import capi
    cols, rows, vals, n = mat
    out = {}
    with env(ABFT_HIP_PACKED_FAST=fast, ABFT_HIP_LAZY_X=lazy, ABFT_HIP_X_IN_SPMV=xin):
        ctx = amd.HIPContext("none", "csr")
        try:
            A = ctx.create_matrix(cols, rows, vals, n, len(vals))
            assert ctx.matrix_info(A)[0] == "stream"
            out["stats"] = [ctx.packed_stats(A)]
            for at, flips in injects:
                ctx.inject_at(A, at, flips)
                out["stats"].append(ctx.packed_stats(A))
            V = {c: ctx.create_vector(n) for c in "xrpwsy"}
            sc = ctx.create_vector(2)
            ctx.upload(V["s"], special_x(n, seed))
            ctx.upload(V["y"], np.full(n, np.nan))
            capi.check(ctx.L.abft_hip_spmv_dot_part_dev(ctx.h, A.h, V["s"].h, V["y"].h, 0, sc.device_ptr, capi.PART_ALL))
            out["y"], out["fused"] = ctx.download(V["y"]), ctx.download(sc)[0]
            ctx.upload(V["y"], np.full(n, np.nan))
            ctx.spmv(A, V["s"], V["y"])  # ... and without the fused product
            out["y_plain"] = ctx.download(V["y"])
            rng = np.random.default_rng(seed + 1)
            for c in "xrp":
                ctx.upload(V[c], rng.random(n) - 0.5)
            ctx.upload(V["w"], np.zeros(n))
            sca = []
            for j in range(iters):
                ctx.spmv(A, V["p"], V["w"])
                sca.append(ctx.dot(V["p"], V["w"]))
                sca.append(ctx.calc_xr(V["x"], V["r"], V["p"], V["w"], 0.37 + 0.01 * j))
                ctx.calc_p(V["p"], V["r"], 0.61 - 0.02 * j)
            out["x_in_spmv"], out["lazy"] = ctx.x_in_spmv_stats(), ctx.lazy_x_stats()
            out["scalars"] = np.array(sca)
            for c in "xrpw":
                out[c] = ctx.download(V[c])
        finally:
            ctx.close()
    return out


def same(on, off):
    """bit for bit, by tests/_ieee.py's rule: a NaN matches a NaN of any sign and payload.  Where two NaNs of different
    payloads meet in one row's sum, the one that survives is the first operand of the add, and the compiler is free to
    order the operands of a commutative add differently in the two paths (seen: row 19661 of the Laplacian, whose
    stencil gathers both NaNs of special_x)."""
    for key in ("y", "y_plain", "fused", "scalars", "x", "r", "p", "w"):
        assert ieee_equal(on[key], off[key]), (key, ieee_diff(on[key], off[key]))
    assert on["x_in_spmv"] == off["x_in_spmv"] and on["lazy"] == off["lazy"]


def both(mat, **kw):
    on, off = play(mat, 1, **kw), play(mat, 0, **kw)
    for packed, stage, row in off["stats"]:
        assert packed > 0 and (stage, row) == (0, 0)
    assert [s[0] for s in on["stats"]][0] == off["stats"][0][0]
    same(on, off)
    return on


def test_laplace_crosses_both_paths():
    """two values: shift 15, so the blocks whose base lies within 32768 entries of the vector's end are general; the
    boundary rows make some blocks non-uniform (stage-fast, general rows)"""
    on = both(laplace5(260, 260))
    packed, stage, row = on["stats"][0]
    assert 0 < stage < packed and 0 < row < stage, on["stats"]
    assert np.isnan(on["y"]).any() and np.isinf(on["y"]).any()  # the special vector did reach the output


@pytest.mark.parametrize("odd", [False, True], ids=["even", "odd"])
@pytest.mark.parametrize("length", [1, 2, 3, 4, 5, 7, 8, 9, 16])
def test_band_of_sixteen_values(length, odd):
    on = both(band16(length, odd))
    packed, stage, row = on["stats"][0]
    assert 0 < stage < packed, on["stats"]
    if length in (4, 5, 7, 8):
        assert 0 < row <= stage  # (odd: the first block, with its one short row, is not uniform)
    else:
        assert row == 0  # 1 .. 3: more rows than threads in a block; 9, 16: longer than the row-fast field knows
    # rows whose products are all zeros, a -0.0 among them or alone: +0.0
    y = on["y_plain"]
    assert (bits(y) == 0).any() and not (bits(y) == bits(np.array([-0.0]))[0]).any()


def test_small_columns_in_the_last_rows():
    on = both(small_columns_last())
    packed, stage, row = on["stats"][0]
    # every window of columns fits; the last tile would pass the codes (rows of 3: more rows than threads, no row-fast)
    assert stage == packed - 1 and row == 0, on["stats"]


@pytest.mark.parametrize("which", ["lap260", "band5", "band3odd"])
@pytest.mark.parametrize("depth", [1, 2, 4])
def test_updates_applied_by_a_fast_spmv(depth, which):
    """x-in-SpMV armed and a queue of `depth` updates: the NUPD = 1, 2, 4 instantiations take the fast path"""
    mat = {"lap260": lambda: laplace5(260, 260), "band5": lambda: band16(5), "band3odd": lambda: band16(3, True)}[which]()
    on = both(mat, lazy=depth, xin=1, iters=2 * depth + 2)
    assert 0 < on["stats"][0][1] < on["stats"][0][0]
    if depth == 1:
        assert on["x_in_spmv"][0] > 0, on["x_in_spmv"]
    else:
        bursts, applied, _ = on["lazy"]
        assert bursts > 0 and applied >= bursts, on["lazy"]


def test_word_follows_the_replan_after_an_inject():
    """flips into elements of fast blocks: a value bit (a ninth value: the block packs again, at shift 12 instead of
    13), a low column bit (packs again), a high column bit (the block is demoted: its word goes to 0); the SpMV and
    the loop agree with the switch off afterwards"""
    mat = band16(5, nv=8)
    cols, rows, vals, n = mat
    tile_rows = 204  # 1020 of 1024 elements
    at = [7, 5 * tile_rows + 11, 2 * 5 * tile_rows + 3]  # elements of blocks 0, 1 and 2
    injects = [(at[0], [3]), (at[1], [64]), (at[2], [64 + 20])]
    on = both(mat, injects=injects)
    (p0, s0, r0), (p1, s1, r1), (p2, s2, r2), (p3, s3, r3) = on["stats"]
    assert (p1, s1, r1) == (p0, s0, r0) and (p2, s2, r2) == (p0, s0, r0), on["stats"]
    assert (p3, s3, r3) == (p0 - 1, s0 - 1, r0 - 1), on["stats"]
