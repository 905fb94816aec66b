"""The wiring between the layout planner (csrc/layout_plan.h) and the library: what abft_hip.hip asks, uploads and
attaches.  On one small matrix every layout is created in two modes; what the library reports of each -- the layout,
the launches per SpMV, the panel geometry, the compact and packed tiles -- equals what the library reported before the
planner moved into that header (tests/golden/layout_plan_gpu.json, recorded on an MI355X from the parent commit's
build by tests/golden/make_layout_plan_gpu_golden.py), and one SpMV is bit-equal to the CPU oracle's.  The planner's
own answers are held without a GPU by tests/test_layout_plan_host.py."""
import json
import os

import numpy as np
import pytest

from _ieee import csr_tile
from _oracle import COO, CSR, OracleMatrix, rhs
from test_gpu_packed_csr import bits_equal, compact_stats, packed_stats

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N, PER_ROW = 600, 7
ENV = {"ABFT_HIP_PANEL_WIDTH": "16"}
# (format, ABFT_HIP_LAYOUT): CSR stream / panels / sweep / slice, COO grouped by output / panels
LAYOUTS = [("csr", "stream"), ("csr", "panels"), ("csr", "sweep"), ("csr", "slice"), ("coo", "stream"), ("coo", "panels")]
MODES = ["none", "secded"]


def matrix():
    """600 x 600, 7 ascending random columns per row, three distinct values (so blocks pack)"""
    rng = np.random.default_rng(600)
    cols = np.sort(rng.integers(0, N, size=(N, PER_ROW)), axis=1).reshape(-1).astype(np.uint32)
    rows = np.repeat(np.arange(N, dtype=np.uint32), PER_ROW)
    vals = rng.choice([-1.0, 4.0, 0.5], size=N * PER_ROW)
    return cols, rows, vals, N


def key(fmt, layout, mode):
    return "%s.%s.%s" % (fmt, layout, mode)


def observe(amd, fmt, mode, cols, rows, vals, n):
    """-> (what the library reports of the matrix it created, y of one SpMV); the environment is the caller's"""
    import ctypes as C
    ctx = amd.HIPContext(mode, fmt)
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        npanels, width = C.c_int(), C.c_int()
        assert ctx.L.abft_hip_matrix_panels(A.h, C.byref(npanels), C.byref(width)) == 0
        seen = dict(info=list(ctx.matrix_info(A)), panels=[npanels.value, width.value],
                    compact=list(compact_stats(ctx, A)), packed=list(packed_stats(ctx, A)))
        vx, vy = ctx.create_vector(n), ctx.create_vector(n)
        ctx.upload(vx, rhs(n, 3) - 0.5)
        ctx.upload(vy, np.full(n, np.nan))
        ctx.spmv(A, vx, vy)
        return seen, ctx.download(vy)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "layout_plan_gpu.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def oracle_y():
    cols, rows, vals, n = matrix()
    x = rhs(n, 3) - 0.5
    return {(fmt, mode): OracleMatrix(CSR if fmt == "csr" else COO, mode, cols, rows, vals, n).spmv(x)
            for fmt in ("csr", "coo") for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt,layout", LAYOUTS)
def test_every_layout_as_the_parent_built_it(amd, monkeypatch, golden, oracle_y, fmt, layout, mode):
    for k, v in dict(ENV, ABFT_HIP_LAYOUT=layout).items():
        monkeypatch.setenv(k, v)
    seen, y = observe(amd, fmt, mode, *matrix())
    assert seen == golden["cases"][key(fmt, layout, mode)], key(fmt, layout, mode)
    assert seen["info"][0] == layout  # (the fixture itself: every layout was taken, COO "stream" = grouped by output)
    assert seen["compact"][2] == 0 and seen["packed"][2] == 0
    assert bits_equal(y, oracle_y[fmt, mode])


def test_fixture_reaches_the_compact_and_packed_tiles(golden):
    c = golden["cases"]
    assert c["csr.stream.none"]["compact"][0] == c["csr.stream.none"]["compact"][1] > 0
    assert c["csr.stream.none"]["packed"][0] == c["csr.stream.none"]["packed"][1] > 0
    assert c["csr.stream.secded"]["packed"][:2] == [0, c["csr.stream.none"]["packed"][1]]
    assert all(c[key("csr", lay, m)]["packed"][:2] == [0, 0] for lay in ("panels", "sweep", "slice") for m in MODES)
    assert c["csr.panels.none"]["info"][1] > 1 and c["csr.sweep.none"]["panels"] == [38, 16]


@pytest.mark.parametrize("mode", MODES)
def test_row_one_past_a_tile_on_the_streaming_layout(amd, mode):
    """40 x 40, row 3 with one element more than a CSR tile: a block of its own, walked tile by tile"""
    n, long_row = 40, csr_tile() + 1
    assert long_row == 1025
    parts = [(np.array([r]), np.array([2.0])) if r != 3 else
             (np.arange(long_row) * n // long_row, 1.0 + np.arange(long_row) % 3) for r in range(n)]
    cols = np.concatenate([c for c, _ in parts]).astype(np.uint32)
    rows = np.concatenate([np.full(len(c), r) for r, (c, _) in enumerate(parts)]).astype(np.uint32)
    vals = np.concatenate([v for _, v in parts]).astype(np.float64)
    x = rhs(n, 4) - 0.5
    want = OracleMatrix(CSR, mode, cols, rows, vals, n).spmv(x)
    ctx = amd.HIPContext(mode, "csr")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        assert ctx.matrix_info(A) == ("stream", 1)
        p, t, m = packed_stats(ctx, A)
        assert (t, m) == (3, 0) and p == (2 if mode == "none" else 0)  # rows 0-2, row 3 (not one tile: never packed), rows 4-39
        vx, vy = ctx.create_vector(n), ctx.create_vector(n)
        ctx.upload(vx, x)
        ctx.upload(vy, np.full(n, np.nan))
        ctx.spmv(A, vx, vy)
        assert bits_equal(ctx.download(vy), want)
    finally:
        ctx.close()


def test_inject_into_a_packed_block_reaches_the_device_copies(amd):
    """a value bit (the block is planned anew, with a palette the pool has not held), then a high column bit (the block
    is demoted, its neighbours are not): the SpMV reads what the re-plan wrote"""
    cols, rows, vals, n = matrix()
    x = rhs(n, 3) - 0.5
    o = OracleMatrix(CSR, "none", cols, rows, vals, n)
    ctx = amd.HIPContext("none", "csr")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        p0, t, m = packed_stats(ctx, A)
        assert p0 == t > 2 and m == 0
        vx, vy = ctx.create_vector(n), ctx.create_vector(n)
        ctx.upload(vx, x)
        at = 2 * csr_tile() + 5  # (elements a tile or more apart lie in different blocks: neither the first nor the last)
        for bits, packed in (([30], p0), ([64 + 31], p0 - 1)):
            o.inject(at, bits)
            ctx.inject_at(A, at, bits)
            assert packed_stats(ctx, A) == (packed, t, 0) and compact_stats(ctx, A)[2] == 0
            ctx.upload(vy, np.full(n, np.nan))
            ctx.spmv(A, vx, vy)
            assert bits_equal(ctx.download(vy), o.spmv(x)), bits
            assert np.array_equal(ctx.stored_words(A), o.stored_words())
    finally:
        ctx.close()
