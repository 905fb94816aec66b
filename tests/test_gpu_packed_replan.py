"""Packed CSR blocks (CsrPacked) where a random draw comes too rarely: the palette pool running
out, a captured graph replayed across re-plans, every shift boundary of the planner by
construction, and a block that starts at an odd element index beside a neighbour planned
differently.  tools/fuzz_parity.py's packed family covers the rest at random.

What these tests know of the layout is the documented rule only: a block is a contiguous run of
whole rows of at most one tile of elements.  So two elements a tile or more apart lie in different
blocks, and a row of more than half a tile is a block of its own (no neighbour fits beside it)."""
import ctypes as C

import numpy as np
import pytest

from _ieee import csr_tile, ieee_diff, ieee_equal
from _oracle import CSR, OracleMatrix, laplace5, rhs
from test_gpu_packed_csr import SWAP, Run, bits_equal, compact_stats, packed_stats

pytestmark = pytest.mark.gpu

# palettes the pool holds beyond those of create: ABFT_PAL_SPARE of abft_hip.hip (tests/test_fuzz_generator.py
# compares this constant with the source)
PAL_SPARE = 1024


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def u64(v):
    return int(np.float64(v).view(np.uint64))


def check(h, o, x, what):
    y, _ = h.spmv(x)
    want = o.spmv(x)
    assert ieee_equal(y, want), (what, ieee_diff(y, want))
    assert np.array_equal(h.ctx.stored_words(h.A), o.stored_words()), what
    assert packed_stats(h.ctx, h.A)[2] == 0 and compact_stats(h.ctx, h.A)[2] == 0, what


def test_palette_pool_runs_out(amd):
    """One element of block 0 walks through a Gray code of its 11 lowest mantissa bits: every inject
    flips one bit and gives the block a value set that no block has had -- {-1, 4, v_j} with a new
    v_j -- so each one takes a palette of the pool.  The block holds 3 values throughout.  The pool
    has room for PAL_SPARE palettes beyond those of create: the inject that needs one more demotes
    its block; after that, in other blocks, an inject that needs a new set demotes its block and one
    that lands on a set the pool holds keeps it packed."""
    tile = csr_tile()
    cols, rows, vals, n = laplace5(100, 80)
    nnz = len(vals)
    x = rhs(n, 21) - 0.5
    o = OracleMatrix(CSR, "none", cols, rows, vals, n)
    h = Run(amd, "none", cols, rows, vals, n)

    def inject(i, bits):
        o.inject(i, bits)
        h.ctx.inject_at(h.A, i, bits)  # (raises if the call returns an error)
        return packed_stats(h.ctx, h.A)

    try:
        p0, t, m0 = packed_stats(h.ctx, h.A)
        assert p0 == t and t > 4 and m0 == 0
        # the model: the value sets that exist, as sorted tuples of patterns; every block of the Laplacian starts with {-1, 4}
        sets = {tuple(sorted((u64(-1.0), u64(4.0))))}
        new_sets = 0
        e = 1  # row 0 is (4, -1, -1): its block keeps a 4 and a -1 whatever element 1 becomes
        assert vals[0] == 4.0 and vals[e] == -1.0 and vals[2] == -1.0 and rows[2] == 0
        cur = u64(vals[e])
        demoted_at = None
        for j in range(1, PAL_SPARE + 4):
            bit = ((j ^ (j >> 1)) ^ ((j - 1) ^ ((j - 1) >> 1))).bit_length() - 1  # Gray code: one bit per step
            cur ^= 1 << bit
            s = tuple(sorted({u64(-1.0), u64(4.0), cur}))
            fresh = s not in sets
            if demoted_at is None:  # (a demoted block is not planned again: it takes no palette)
                new_sets += fresh
                sets.add(s)
            p, t1, m = inject(e, [bit])
            assert m == 0 and t1 == t
            if new_sets <= PAL_SPARE:
                assert p == p0, (j, new_sets)
            else:
                assert p == p0 - 1, (j, new_sets)
                demoted_at = demoted_at or j
            if j in (1, 2, PAL_SPARE // 2, PAL_SPARE - 1, PAL_SPARE, PAL_SPARE + 1, PAL_SPARE + 2):
                check(h, o, x, "step %d" % j)
        assert new_sets == PAL_SPARE + 1 and demoted_at == PAL_SPARE + 1
        sets.discard(s)  # the set that found no room exists nowhere

        # the pool is full.  Other blocks (elements a tile or more apart are in different blocks):
        far = [int(np.flatnonzero((rows == r) & (vals == -1.0))[0]) for r in (n // 4, n // 2, 3 * n // 4, n - 1)]
        assert all(b - a >= tile for a, b in zip([e] + far, far))
        # -1 -> 4: the set stays {-1, 4} (every row keeps another -1), which the pool holds: still packed
        p, _, m = inject(far[0], SWAP)
        assert (p, m) == (p0 - 1, 0)
        check(h, o, x, "existing set, same block's own")
        # the first set block 0 made, {-1, 4, -1 ^ bit 0}, made again in another block: the pool holds it
        first = tuple(sorted({u64(-1.0), u64(4.0), u64(-1.0) ^ 1}))
        assert first in sets
        p, _, m = inject(far[1], [0])
        assert (p, m) == (p0 - 1, 0)
        check(h, o, x, "existing set, another block's")
        # a set that no block has had: no room, the block is demoted
        assert tuple(sorted({u64(-1.0), u64(4.0), u64(-1.0) ^ (1 << 40)})) not in sets
        p, _, m = inject(far[2], [40])
        assert (p, m) == (p0 - 2, 0)
        check(h, o, x, "new set, pool full")
        # ... and flipped back it stays demoted; the last block still re-plans onto {-1, 4}
        p, _, m = inject(far[2], [40])
        assert (p, m) == (p0 - 2, 0)
        p, _, m = inject(far[3], SWAP)
        assert (p, m) == (p0 - 2, 0)
        check(h, o, x, "end")
        assert compact_stats(h.ctx, h.A) == (t, t, 0)  # the demoted blocks read compact columns
        assert nnz == len(vals)
    finally:
        h.close()


@pytest.mark.parametrize("where", ["one_block", "three_blocks"])
@pytest.mark.parametrize("compact", ["1", "0"])
def test_graph_replay_across_replans(amd, monkeypatch, compact, where):
    """A captured abft_hip_spmv_dot_dev holds the pointers of the codes, the descriptors and the palette
    pool: replayed after an inject that packs the block anew with a new palette, one that demotes a
    block to compact columns and one that demotes a block to wide columns, it must read what the
    re-plan wrote."""
    from abft_sparse_cg_amd import capi
    monkeypatch.setenv("ABFT_HIP_COMPACT_COLS", compact)
    tile = csr_tile()
    cols, rows, vals, n = laplace5(300, 250)
    x = rhs(n, 17) - 0.5
    o = OracleMatrix(CSR, "none", cols, rows, vals, n)
    h = Run(amd, "none", cols, rows, vals, n)
    L = h.ctx.L
    try:
        p0, t, _ = packed_stats(h.ctx, h.A)
        assert p0 == t
        h.ctx.upload(h.vx, x)
        capi.check(L.abft_hip_spmv_dot_dev(h.ctx.h, h.A.h, h.vx.h, h.vy.h, 0, h.sc.device_ptr))  # (first use outside the capture)
        h.ctx.synchronize()
        capi.check(L.abft_hip_graph_begin(h.ctx.h))
        capi.check(L.abft_hip_spmv_dot_dev(h.ctx.h, h.A.h, h.vx.h, h.vy.h, 0, h.sc.device_ptr))
        g = C.c_void_p()
        capi.check(L.abft_hip_graph_end(h.ctx.h, C.byref(g)))

        def replay(what):
            h.ctx.upload(h.vy, np.full(n, np.nan))
            h.ctx.upload(h.sc, np.full(2, np.nan))
            capi.check(L.abft_hip_graph_launch(g))
            y, dot = h.ctx.download(h.vy), float(h.ctx.download(h.sc)[0])
            want = o.spmv(x)
            assert bits_equal(y, want), what
            assert abs(dot - float(x @ want)) <= 1e-12 * float(np.abs(x * want).sum()), what
            assert packed_stats(h.ctx, h.A)[2] == 0 and compact_stats(h.ctx, h.A)[2] == 0, what

        replay("before")
        mid = int(np.searchsorted(rows, 20000))  # columns near 20 000: bit 15 is clear, so flipping it adds 32 768 (still below N)
        assert all(cols[mid + d] & 0x8000 == 0 and cols[mid + d] + 0x8000 < n for d in (3, 2 * tile))
        at = [mid, mid + 3, mid + 7] if where == "one_block" else [mid, mid + 2 * tile, mid + 4 * tile]
        steps = [("new palette", [63], p0), ("to compact", [64 + 15], p0 - 1),
                 ("to wide", [64 + 31], p0 - 1 if where == "one_block" else p0 - 2)]
        for (what, bits, p_want), i in zip(steps, at):
            o.inject(i, bits)
            h.ctx.inject_at(h.A, i, bits)
            assert packed_stats(h.ctx, h.A)[0] == p_want, what
            replay(what)
            replay(what + ", again")
        c, _, _ = compact_stats(h.ctx, h.A)
        assert c == (0 if compact == "0" else t - 1)  # the block with a column past N reads wide columns
        L.abft_hip_graph_destroy(g)
    finally:
        h.close()


# ---- single rows as blocks: a row of more than half a tile shares its block with no other row ----

N_IN = 140000


def row_block(length, lo, span, nvals, first_value, rng):
    """-> (columns, values) of one row: `length` columns in [lo, lo + span] with both ends taken,
    exactly `nvals` distinct values first_value, first_value + 1, ..."""
    assert 2 <= length <= span + 1 or (span == 0 and length == 1)
    inner = rng.choice(np.arange(1, span), size=length - 2, replace=False) if length > 2 else np.zeros(0, np.int64)
    c = lo + np.sort(np.concatenate([[0, span], inner])).astype(np.int64)
    v = first_value + (rng.permutation(length) % nvals)
    assert len(np.unique(v)) == nvals
    return c, v.astype(np.float64)


def rows_matrix(parts):
    cols = np.concatenate([c for c, _ in parts]).astype(np.uint32)
    rows = np.concatenate([np.full(len(c), r) for r, (c, _) in enumerate(parts)]).astype(np.uint32)
    return cols, rows, np.concatenate([v for _, v in parts]), len(parts)


def packs_by_rule(nvals, span):
    """DESIGN.md / abft_internal.h: k = ceil(log2(#values)), at most 16 values, max - min column < 2^(16 - k)"""
    if nvals > 16:
        return False
    k = 0
    while (1 << k) < nvals:
        k += 1
    return span < (1 << (16 - k))


BOUNDARY_CASES = sorted({(nv, s) for k in range(5) for nv in ([1 << k] + ([(1 << k) + 1] if k < 4 else []))
                         for s in ((1 << (16 - k)) - 1, 1 << (16 - k), (1 << (15 - k)) - 1, 1 << (15 - k))}
                        | {(16, 4095), (16, 4096), (17, 700), (17, 4095)})


@pytest.mark.parametrize("nvals,span", BOUNDARY_CASES)
@pytest.mark.parametrize("parity", [0, 1])
def test_shift_boundaries(amd, nvals, span, parity):
    """One row of 601 elements (a block of its own) with exactly `nvals` values over columns that span
    exactly `span`, after a first row of 600 + parity elements (so that the block under test starts at
    an even or an odd element index): it packs exactly when the rule says so, and y is right either way."""
    rng = np.random.default_rng(1000 * nvals + span)
    assert 2 * 600 > csr_tile() >= 602
    parts = [row_block(600 + parity, 5, 800, 2, -3.0, rng), row_block(601, 2000 + parity, span, nvals, 1.0, rng)]
    cols, rows, vals, n = rows_matrix(parts)
    x = rhs(N_IN, 5) - 0.5
    o = OracleMatrix(CSR, "none", cols, rows, vals, n, n_in=N_IN, index_base=0)
    h = Run(amd, "none", cols, rows, vals, n, n_in=N_IN, index_base=0)
    try:
        p, t, m = packed_stats(h.ctx, h.A)
        assert (t, m) == (2, 0)
        assert p == 1 + packs_by_rule(nvals, span), (nvals, span, p)
        assert compact_stats(h.ctx, h.A)[0] == 1 + (span <= 65535)
        check(h, o, x, "created")
        # one more value in the row under test (a low mantissa bit of a small integer): the rule again, with nvals + 1
        i = 600 + parity + 300
        o.inject(i, [30])
        h.ctx.inject_at(h.A, i, [30])
        assert packed_stats(h.ctx, h.A)[0] == 1 + (packs_by_rule(nvals, span) and packs_by_rule(nvals + 1, span))
        check(h, o, x, "one more value")
    finally:
        h.close()


@pytest.mark.parametrize("neighbour", ["packed_other", "compact", "wide"])
def test_odd_first_element_beside_another_plan(amd, neighbour):
    """Block 0 (row 0, 601 elements) is packed with 2 values at base 1000.  Block 1 starts at the odd
    element 601 -- the code in the slot before it is block 0's, relative to block 0's base and palette --
    and is packed with 5 values at another base and shift, or compact (17 values), or wide (a span of
    65536 or more).  Then block 0 is re-planned (a third value: another palette and shift), and then
    demoted (a column far away): block 1's row must not change."""
    rng = np.random.default_rng(77)
    spec = {"packed_other": (5, 8000), "compact": (17, 60000), "wide": (3, 70000)}[neighbour]
    parts = [row_block(601, 1000, 3000, 2, -2.0, rng), row_block(601, 50001, spec[1], spec[0], 1.0, rng),
             row_block(601, 300, 1200, 4, 0.5, rng)]
    cols, rows, vals, n = rows_matrix(parts)
    x = rhs(N_IN, 6) - 0.5
    o = OracleMatrix(CSR, "none", cols, rows, vals, n, n_in=N_IN, index_base=0)
    h = Run(amd, "none", cols, rows, vals, n, n_in=N_IN, index_base=0)
    try:
        p, t, m = packed_stats(h.ctx, h.A)
        assert (t, m) == (3, 0) and p == (3 if neighbour == "packed_other" else 2)
        assert compact_stats(h.ctx, h.A)[0] == (2 if neighbour == "wide" else 3)
        check(h, o, x, "created")
        for what, i, bits, drop in [("last element of block 0: a third value", 600, [50], 0),
                                    ("first element of block 1: a new value", 601, [50], 1 if neighbour == "compact" else 0),
                                    ("block 0 demoted by its last column", 600, [64 + 17], 1)]:
            o.inject(i, bits)
            h.ctx.inject_at(h.A, i, bits)
            p1 = packed_stats(h.ctx, h.A)[0]
            if neighbour == "compact" and i == 601:
                drop = 0  # (block 1 was not packed)
            assert p1 == p - drop, (what, p1, p)
            p = p1
            check(h, o, x, what)
    finally:
        h.close()
