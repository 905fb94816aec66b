"""Mode none on the streaming row-block CSR layout: the SpMV reads every block with at most 16
distinct values and a column span that fits as one 16-bit code per element -- column offset and
value palette index together (CsrPacked).

Checks that packing happens where it should and nowhere else, that y, the fused p.w and a CG run
are bit-identical with it switched off (ABFT_HIP_PACKED=0) and to the oracle, and that injected
flips into packed blocks re-plan them so that the codes always decode to the stored words."""
import ctypes as C

import numpy as np
import pytest

from _ieee import ieee_diff, ieee_equal
from _oracle import CSR, OracleMatrix, laplace5, random_spd, rhs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def tridiag(n, value_of, extra=()):
    """Tridiagonal pattern plus `extra` (row, col) entries; value_of(rows, cols, k) -> values."""
    ent = set()
    for r in range(n):
        ent |= {(r, max(r - 1, 0)), (r, r), (r, min(r + 1, n - 1))}
    ent |= set(extra)
    ent = sorted(ent)
    rows = np.array([e[0] for e in ent], np.uint32)
    cols = np.array([e[1] for e in ent], np.uint32)
    vals = np.asarray(value_of(rows, cols, np.arange(len(ent))), np.float64)
    return cols, rows, vals, n


def seventeen_values():
    """Every block holds 17 distinct values: none packs."""
    return tridiag(3000, lambda r, c, k: 1.0 + (k % 17))


def three_values_wide_span():
    """Block 0 holds 3 values (k = 2, 14 bits of span) and spans 20 000 columns: compact, not
    packed.  Every other block holds 2 values over a short span and packs."""
    def vals(r, c, k):
        v = np.where(r == c, 4.0, -1.0)
        v[(r == 1) & (c == 20000)] = 0.5
        return v
    return tridiag(40000, vals, extra=[(1, 20000)])


def wide_row(n=70000):
    """Tridiagonal, plus row 1 reaching column n - 1: its block spans more than 65536 columns."""
    return tridiag(n, lambda r, c, k: np.where(r == c, 4.0, -1.0), extra=[(1, n - 1)])


def long_row(n=3000, width=1500):
    """Row 5 holds `width` elements (more than one tile): its block is walked tile by tile."""
    return tridiag(n, lambda r, c, k: np.where(r == c, 4.0, -1.0), extra=[(5, c) for c in range(width)])


def special_values():
    """Two-valued stencil blocks salted with +0.0 / -0.0, NaNs of different payloads, +-inf and
    subnormals: at most 8 distinct patterns per block, so every block still packs."""
    sp = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -2.5e-310], np.float64)
    nans = np.array([0x7FF8000000000001, 0xFFF0000000000123], np.uint64).view(np.float64)
    pool = np.concatenate([sp, nans])

    def vals(r, c, k):
        v = np.where(r == c, 4.0, -1.0)
        hit = k % 37 == 5
        v[hit] = pool[(k[hit] // 37) % len(pool)]
        return v
    return tridiag(20000, vals)


MATS = {
    "lap40": lambda: laplace5(40, 33),
    "lap300": lambda: laplace5(300, 250),
    "rnd300": lambda: random_spd(300, 10, seed=5),
    "seventeen": seventeen_values,
    "three_wide": three_values_wide_span,
    "wide": wide_row,
    "long": long_row,
    "special": special_values,
}


def packed_stats(ctx, A):
    p, t, m = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert ctx.L.abft_hip_matrix_packed_stats(A.h, C.byref(p), C.byref(t), C.byref(m)) == 0
    return p.value, t.value, m.value


def compact_stats(ctx, A):
    c, t, m = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert ctx.L.abft_hip_matrix_compact_stats(A.h, C.byref(c), C.byref(t), C.byref(m)) == 0
    return c.value, t.value, m.value


class Run:
    def __init__(self, amd, mode, cols, rows, vals, n, **kw):
        self.ctx = amd.HIPContext(mode, "csr")
        self.n = n
        self.n_in = kw.get("n_in") or n
        # a shard (n_in, index_base) takes the library's layout: the streaming one for banded matrices
        self.A = self.ctx.create_matrix(cols, rows, vals, n, len(vals), layout=None if kw else "stream", **kw)
        self.vx, self.vy = self.ctx.create_vector(self.n_in), self.ctx.create_vector(n)
        self.sc = self.ctx.create_vector(2)

    def spmv(self, x, part=None):
        """-> (y, the fused x.y of spmv_dot) -- y from a plain SpMV, or from its two parts"""
        from abft_sparse_cg_amd import capi
        L, hc = self.ctx.L, self.ctx.h
        self.ctx.upload(self.vx, x)
        self.ctx.upload(self.vy, np.full(self.n, np.nan))
        if part is None:
            capi.check(L.abft_hip_spmv_dot_part_dev(hc, self.A.h, self.vx.h, self.vy.h, 0, self.sc.device_ptr,
                                                    capi.PART_ALL))
            return self.ctx.download(self.vy), self.ctx.download(self.sc)[0]
        self.ctx.spmv(self.A, self.vx, self.vy, capi.PART_INTERIOR)
        self.ctx.spmv(self.A, self.vx, self.vy, capi.PART_BOUNDARY)
        return self.ctx.download(self.vy), None

    def close(self):
        self.ctx.close()


@pytest.mark.parametrize("nx,ny", [(9, 7), (40, 33), (300, 250), (1000, 999)])
def test_laplace_blocks_are_all_packed(amd, nx, ny):
    cols, rows, vals, n = laplace5(nx, ny)
    h = Run(amd, "none", cols, rows, vals, n)
    try:
        p, t, m = packed_stats(h.ctx, h.A)
        assert t > 0 and p == t and m == 0, (p, t, m)
        assert compact_stats(h.ctx, h.A) == (t, t, 0)  # the compact columns are there as before
    finally:
        h.close()


@pytest.mark.parametrize("name,expect", [("rnd300", "none"), ("seventeen", "none"), ("wide", "all_but_one"),
                                         ("long", "all_but_one"), ("three_wide", "all_but_one"),
                                         ("special", "all")])
def test_which_blocks_pack(amd, name, expect):
    cols, rows, vals, n = MATS[name]()
    h = Run(amd, "none", cols, rows, vals, n)
    try:
        p, t, m = packed_stats(h.ctx, h.A)
        assert t > 2 and m == 0
        if name == "seventeen":  # (a last block of fewer than 17 elements may pack)
            assert p <= 1, (p, t)
        else:
            assert p == {"none": 0, "all_but_one": t - 1, "all": t}[expect], (name, p, t)
        if name == "three_wide":
            assert compact_stats(h.ctx, h.A)[0] == t  # block 0 stays compact
    finally:
        h.close()


@pytest.mark.parametrize("mode", ["constraints", "sed", "sec7", "sec8", "secded"])
def test_other_modes_have_no_packed_blocks(amd, mode):
    cols, rows, vals, n = laplace5(40, 33)
    h = Run(amd, mode, cols, rows, vals, n)
    try:
        p, t, m = packed_stats(h.ctx, h.A)
        assert p == 0 and t > 0 and m == 0
    finally:
        h.close()


@pytest.mark.parametrize("compact", ["1", "0"])
def test_switch_off_packs_nothing(amd, monkeypatch, compact):
    monkeypatch.setenv("ABFT_HIP_PACKED", "0")
    monkeypatch.setenv("ABFT_HIP_COMPACT_COLS", compact)
    cols, rows, vals, n = laplace5(40, 33)
    h = Run(amd, "none", cols, rows, vals, n)
    try:
        p, t, m = packed_stats(h.ctx, h.A)
        assert p == 0 and t > 0 and m == 0
        assert (compact_stats(h.ctx, h.A)[0] == t) == (compact == "1")
    finally:
        h.close()


def test_packing_without_compact_columns(amd, monkeypatch):
    monkeypatch.setenv("ABFT_HIP_COMPACT_COLS", "0")
    cols, rows, vals, n = laplace5(300, 250)
    x = rhs(n, 3) - 0.5
    h = Run(amd, "none", cols, rows, vals, n)
    try:
        p, t, m = packed_stats(h.ctx, h.A)
        assert p == t and m == 0 and compact_stats(h.ctx, h.A)[0] == 0
        assert bits_equal(h.spmv(x)[0], OracleMatrix(CSR, "none", cols, rows, vals, n).spmv(x))
    finally:
        h.close()


@pytest.mark.parametrize("name", sorted(MATS))
def test_spmv_and_fused_dot_match_unpacked_and_oracle(amd, monkeypatch, name):
    cols, rows, vals, n = MATS[name]()
    x = rhs(n, 7) - 0.5
    want = OracleMatrix(CSR, "none", cols, rows, vals, n).spmv(x)
    out = {}
    for on in ("1", "0"):
        monkeypatch.setenv("ABFT_HIP_PACKED", on)
        h = Run(amd, "none", cols, rows, vals, n)
        try:
            out[on] = h.spmv(x)
            if on == "0":
                assert packed_stats(h.ctx, h.A)[0] == 0
        finally:
            h.close()
    assert ieee_equal(out["1"][0], want), ieee_diff(out["1"][0], want)
    assert bits_equal(out["1"][0], out["0"][0])
    assert bits_equal(out["1"][1], out["0"][1])


@pytest.mark.parametrize("name", ["lap300", "special", "three_wide"])
def test_partial_spmv_matches_unpacked(amd, monkeypatch, name):
    cols, rows, vals, n = MATS[name]()
    x = rhs(n, 5) - 0.5
    want = OracleMatrix(CSR, "none", cols, rows, vals, n).spmv(x)
    out = {}
    for on in ("1", "0"):
        monkeypatch.setenv("ABFT_HIP_PACKED", on)
        h = Run(amd, "none", cols, rows, vals, n)
        try:
            h.ctx.set_interior(h.A, 40, n - 300)
            out[on] = h.spmv(x, part=True)[0]
        finally:
            h.close()
    assert ieee_equal(out["1"], want), ieee_diff(out["1"], want)
    assert bits_equal(out["1"], out["0"])


def test_row_block_shard_matches_unpacked(amd, monkeypatch):
    cols, rows, vals, n = laplace5(300, 250)
    r0, r1 = 20000, 52000
    m = (rows >= r0) & (rows < r1)
    base = int(np.argmax(m))
    x = rhs(n, 11) - 0.5
    shard = (cols[m], rows[m] - r0, vals[m], r1 - r0)
    want = OracleMatrix(CSR, "none", *shard, n_in=n, index_base=base).spmv(x)
    out = {}
    for on in ("1", "0"):
        monkeypatch.setenv("ABFT_HIP_PACKED", on)
        h = Run(amd, "none", *shard, n_in=n, index_base=base)
        try:
            p, t, mm = packed_stats(h.ctx, h.A)
            assert mm == 0 and (p == t if on == "1" else p == 0)
            out[on] = h.spmv(x)
        finally:
            h.close()
    assert bits_equal(out["1"][0], want)
    assert bits_equal(out["1"][0], out["0"][0]) and bits_equal(out["1"][1], out["0"][1])


# the 96-bit CSR word: value bits 0..63, column bits 64..95.  -1.0 and 4.0 differ in the sign and
# in exponent bits 53..62: flipping all of them turns one palette entry into the other
SWAP = [63] + list(range(53, 63))
FLIPS = {
    "value_in_palette": SWAP,            # -1 <-> 4: the palette stays {-1, 4}
    "value_sign": [63],                  # a new value: the palette grows past 2^k (2 -> 3)
    "value_mantissa": [3],
    "col_inside_span": [64],             # +-1
    "col_mid_span": [64 + 13],           # +-8192: still inside 15 bits of span, or below the base
    "col_outside_span": [64 + 15],       # +-32768: the block no longer packs; compact or wide
    "col_past_n": [64 + 31],             # far past N: no gather, as the reference's bounds
    "value_and_col": [5, 64 + 2],
}


@pytest.mark.parametrize("kind", sorted(FLIPS))
def test_injections_on_packed_blocks_match_oracle(amd, kind):
    cols, rows, vals, n = laplace5(300, 250)  # N = 75 000
    nnz = len(vals)
    x = rhs(n, 9) - 0.5
    rng = np.random.default_rng(200 + sorted(FLIPS).index(kind))
    o = OracleMatrix(CSR, "none", cols, rows, vals, n)
    h = Run(amd, "none", cols, rows, vals, n)
    try:
        p0, t, _ = packed_stats(h.ctx, h.A)
        assert p0 == t
        for _ in range(6):
            i = int(rng.integers(0, nnz))
            o.inject(i, FLIPS[kind])
            h.ctx.inject_at(h.A, i, FLIPS[kind])
            assert packed_stats(h.ctx, h.A)[2] == 0
        for _ in range(2):
            y, _ = h.spmv(x)
            assert bits_equal(y, o.spmv(x)), kind
        assert np.array_equal(h.ctx.stored_words(h.A), o.stored_words())
        p1, t1, m = packed_stats(h.ctx, h.A)
        assert m == 0 and t1 == t
        assert compact_stats(h.ctx, h.A)[2] == 0
        if kind.startswith("value") and kind != "value_and_col":
            assert p1 == p0  # a new value keeps the block packed (k grows)
        if kind in ("col_outside_span", "col_past_n"):
            assert p1 < p0
    finally:
        h.close()


def test_repeated_flips_grow_one_palette_past_16(amd):
    """One block: flips into 16 of its elements, each a different mantissa bit -- its palette
    grows through 3, 5, 9 entries (k = 2, 3, 4) and at 17 the block no longer packs.  Flipping
    them all back leaves the block demoted (the compact path) and its SpMV right."""
    cols, rows, vals, n = laplace5(300, 250)
    x = rhs(n, 13) - 0.5
    o = OracleMatrix(CSR, "none", cols, rows, vals, n)
    h = Run(amd, "none", cols, rows, vals, n)
    try:
        p0, t, _ = packed_stats(h.ctx, h.A)
        first = 0  # elements of block 0 (a block holds ~1000)
        for j in range(16):
            i, bit = first + j, [j]
            o.inject(i, bit)
            h.ctx.inject_at(h.A, i, bit)
            p, _, m = packed_stats(h.ctx, h.A)
            assert m == 0
            if j < 14:  # 2 + j + 1 <= 16 values: still packed
                assert p == p0, j
            if j in (0, 2, 6, 14, 15):
                y, _ = h.spmv(x)
                assert bits_equal(y, o.spmv(x)), j
        assert packed_stats(h.ctx, h.A)[0] == p0 - 1  # 18 values
        assert compact_stats(h.ctx, h.A)[0] == t  # demoted to the compact path
        for j in range(16):
            o.inject(first + j, [j])
            h.ctx.inject_at(h.A, first + j, [j])
        assert packed_stats(h.ctx, h.A)[0] == p0 - 1  # a demoted block stays demoted ...
        y, _ = h.spmv(x)
        assert bits_equal(y, o.spmv(x))  # ... and right
        assert np.array_equal(h.ctx.stored_words(h.A), o.stored_words())
    finally:
        h.close()


def test_cg_bit_identical_with_and_without_packing(amd, monkeypatch):
    cols, rows, vals, n = laplace5(1000, 1000)
    b = rhs(n, 1)
    out = {}
    for on in ("1", "0"):
        monkeypatch.setenv("ABFT_HIP_PACKED", on)
        ctx = amd.HIPContext("none", "csr")
        try:
            A = ctx.create_matrix(cols, rows, vals, n, len(vals))
            assert (packed_stats(ctx, A)[0] > 0) == (on == "1")
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


def _device_free_bytes():
    lib = C.CDLL(None)  # the runtime libabft_hip.so is bound to (loaded RTLD_GLOBAL)
    if not hasattr(lib, "hipMemGetInfo"):
        lib = C.CDLL("libamdhip64.so")
    lib.hipMemGetInfo.restype = C.c_int
    lib.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    free, total = C.c_size_t(), C.c_size_t()
    assert lib.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_switch_off_allocates_no_codes(amd, monkeypatch):
    """ABFT_HIP_PACKED=0 allocates nothing for packing: the device memory a matrix takes is smaller
    by at least its 2-byte codes than with packing on."""
    cols, rows, vals, n = laplace5(2000, 2000)
    nnz = len(vals)
    taken = {}
    for on in ("1", "0"):
        monkeypatch.setenv("ABFT_HIP_PACKED", on)
        ctx = amd.HIPContext("none", "csr")
        try:
            before = _device_free_bytes()
            A = ctx.create_matrix(cols, rows, vals, n, nnz, layout="stream")
            taken[on] = before - _device_free_bytes()
            assert (packed_stats(ctx, A)[0] > 0) == (on == "1")
        finally:
            ctx.close()
    assert taken["1"] - taken["0"] >= 2 * nnz, taken
