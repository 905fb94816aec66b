"""Mode none on the streaming row-block CSR layout: the SpMV reads the columns of every
single-tile block as 16-bit offsets from a per-block base (CsrCompact).

Checks that compaction happens where it should and nowhere else, that y, the fused p.w and
a CG run are bit-identical with it switched off (ABFT_HIP_COMPACT_COLS=0) and to the oracle,
and that injected column flips keep the compact copy consistent with the stored columns --
the CSR-streaming counterpart of test_coo_silently_corrupted_column_scatters_like_reference."""
import ctypes as C

import numpy as np
import pytest

from _oracle import CSR, OracleMatrix, laplace5, random_spd, rhs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def wide_row(n=70000):
    """Tridiagonal, plus row 1 reaching column n - 1: its block spans more than 65536 columns."""
    ent = []
    for r in range(n):
        cs = {max(r - 1, 0), r, min(r + 1, n - 1)}
        if r == 1:
            cs.add(n - 1)
        ent += [(r, c) for c in sorted(cs)]
    rows = np.array([e[0] for e in ent], np.uint32)
    cols = np.array([e[1] for e in ent], np.uint32)
    vals = np.where(rows == cols, 4.0, -1.0) + 1e-3 * np.random.default_rng(3).random(len(ent))
    return cols, rows, vals, n


def long_row(n=3000, width=1500):
    """Row 5 holds `width` elements (more than one tile): its block is walked tile by tile, wide."""
    ent = []
    for r in range(n):
        cs = set(range(width)) if r == 5 else {max(r - 1, 0), r, min(r + 1, n - 1)}
        ent += [(r, c) for c in sorted(cs)]
    rows = np.array([e[0] for e in ent], np.uint32)
    cols = np.array([e[1] for e in ent], np.uint32)
    vals = 1.0 + np.random.default_rng(4).random(len(ent))
    return cols, rows, vals, n


MATS = {
    "lap9x7": lambda: laplace5(9, 7),
    "lap40": lambda: laplace5(40, 33),
    "lap300": lambda: laplace5(300, 250),
    "rnd300": lambda: random_spd(300, 10, seed=5),
    "wide": wide_row,
    "long": long_row,
}


def stats(ctx, A):
    c, t, m = C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = ctx.L.abft_hip_matrix_compact_stats(A.h, C.byref(c), C.byref(t), C.byref(m))
    assert rc == 0
    return c.value, t.value, m.value


class Run:
    def __init__(self, amd, mode, cols, rows, vals, n):
        self.events = []
        self.ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: self.events.extend(ev))
        self.n = n
        self.A = self.ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        self.vx, self.vy = self.ctx.create_vector(n), self.ctx.create_vector(n)

    def spmv(self, x):
        """-> (y, the fused x.y the dot behind the SpMV returns)"""
        self.ctx.upload(self.vx, x)
        self.ctx.upload(self.vy, np.full(self.n, np.nan))
        self.ctx.spmv(self.A, self.vx, self.vy)
        d = self.ctx.dot(self.vx, self.vy)
        return self.ctx.download(self.vy), d

    def close(self):
        self.ctx.close()


@pytest.mark.parametrize("nx,ny", [(9, 7), (40, 33), (300, 250), (1000, 999)])
def test_laplace_blocks_are_all_compact(amd, nx, ny):
    cols, rows, vals, n = laplace5(nx, ny)
    h = Run(amd, "none", cols, rows, vals, n)
    try:
        c, t, m = stats(h.ctx, h.A)
        assert t > 0 and c == t and m == 0, (c, t, m)
    finally:
        h.close()


def test_wide_and_long_blocks_stay_wide(amd):
    for name in ("wide", "long"):
        cols, rows, vals, n = MATS[name]()
        h = Run(amd, "none", cols, rows, vals, n)
        try:
            c, t, m = stats(h.ctx, h.A)
            assert t > 2 and c == t - 1 and m == 0, (name, c, t, m)
        finally:
            h.close()


@pytest.mark.parametrize("mode", ["constraints", "sed", "sec7", "sec8", "secded"])
def test_other_modes_have_no_compact_blocks(amd, mode):
    cols, rows, vals, n = laplace5(40, 33)
    h = Run(amd, mode, cols, rows, vals, n)
    try:
        c, t, m = stats(h.ctx, h.A)
        assert c == 0 and t > 0 and m == 0
    finally:
        h.close()


def test_switch_off_allocates_nothing(amd, monkeypatch):
    monkeypatch.setenv("ABFT_HIP_COMPACT_COLS", "0")
    cols, rows, vals, n = laplace5(40, 33)
    h = Run(amd, "none", cols, rows, vals, n)
    try:
        c, t, m = stats(h.ctx, h.A)
        assert c == 0 and t > 0 and m == 0
    finally:
        h.close()


@pytest.mark.parametrize("name", sorted(MATS))
def test_spmv_and_fused_dot_match_wide_path_and_oracle(amd, monkeypatch, name):
    cols, rows, vals, n = MATS[name]()
    x = rhs(n, 7) - 0.5
    want = OracleMatrix(CSR, "none", cols, rows, vals, n).spmv(x)
    out = {}
    for on in ("1", "0"):
        monkeypatch.setenv("ABFT_HIP_COMPACT_COLS", on)
        h = Run(amd, "none", cols, rows, vals, n)
        try:
            out[on] = h.spmv(x)
            assert (stats(h.ctx, h.A)[0] > 0) == (on == "1")
        finally:
            h.close()
    assert bits_equal(out["1"][0], want) and bits_equal(out["0"][0], want)
    assert bits_equal(out["1"][1], out["0"][1])


# column bits of the 96-bit CSR word are 64..95
FLIPS = {
    "inside_span": [64],          # +-1: the offset is rewritten
    "offset_rewritten": [64 + 12],  # +-4096: outside the block's span, still within 65535 of its base
    "goes_wide": [64 + 16],       # +-65536: the block turns wide, the column may stay below N
    "past_n": [64 + 31],          # far past N: no gather, as the reference's bounds
    "below_base": [64 + 1, 64 + 2],  # may fall below the base: wraps to a large offset -> wide
    "value": [3, 63],
}


@pytest.mark.parametrize("kind", sorted(FLIPS))
def test_injections_on_compact_blocks_match_oracle(amd, kind):
    cols, rows, vals, n = laplace5(300, 250)  # N = 75 000 > 65 536: a column +65536 can stay inside the vector
    nnz = len(vals)
    x = rhs(n, 9) - 0.5
    rng = np.random.default_rng(100 + sorted(FLIPS).index(kind))
    o = OracleMatrix(CSR, "none", cols, rows, vals, n)
    h = Run(amd, "none", cols, rows, vals, n)
    try:
        c0, t, _ = stats(h.ctx, h.A)
        assert c0 == t
        for _ in range(6):
            i = int(rng.integers(0, nnz))
            o.inject(i, FLIPS[kind])
            h.ctx.inject_at(h.A, i, FLIPS[kind])
        for _ in range(2):
            y, _ = h.spmv(x)
            assert bits_equal(y, o.spmv(x)), kind
        assert np.array_equal(h.ctx.stored_words(h.A), o.stored_words())
        c1, t1, m = stats(h.ctx, h.A)
        assert m == 0 and t1 == t
        if kind == "value":
            assert c1 == c0
        if kind in ("goes_wide", "past_n"):
            assert c1 < c0
        if kind in ("inside_span", "offset_rewritten"):
            assert c1 >= c0 - 6
    finally:
        h.close()


def test_cg_bit_identical_with_and_without_compaction(amd, monkeypatch):
    cols, rows, vals, n = laplace5(1000, 1000)
    b = rhs(n, 1)
    out = {}
    for on in ("1", "0"):
        monkeypatch.setenv("ABFT_HIP_COMPACT_COLS", on)
        ctx = amd.HIPContext("none", "csr")
        try:
            A = ctx.create_matrix(cols, rows, vals, n, len(vals))
            assert (stats(ctx, A)[0] > 0) == (on == "1")
            vb, vx, vr, vp, vw = (ctx.create_vector(n) for _ in range(5))
            ctx.upload(vb, b)
            ctx.upload(vx, np.zeros(n))
            it, rr = amd.cg_solve(ctx, A, vb, vx, vr, vp, vw, max_itrs=25, conv_threshold=0.0)
            assert it == 25
            out[on] = [ctx.download(v) for v in (vx, vr, vp, vw)] + [np.array([rr])]
        finally:
            ctx.close()
    for a, b2 in zip(out["1"], out["0"]):
        assert bits_equal(a, b2)
