"""Protected vectors on the GPU: the codec, the scrub, the four protected CG
calls against the numpy model of tests/_vecc.py (vectors and words bit for bit, sums within the 1e-13
of test_vector_kernels -- relative to the sum of the terms' magnitudes: tree sums against the model's serial ones), single flips in every operand of
every entry, the fused product's bookkeeping, the refusals, and cg_solve(vector_ecc=True) clean and
under flips.

A flip in a vector that several calls read before one rewrites it is reported by each of them: a flip
in p after an iteration gives three lines (spmv_vecc and calc_p_vecc: operand 0, calc_xr_vecc: operand
2), not one; the command-line test asserts those three."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _vecc
from _oracle import laplace5, rhs
from test_gpu_packed_csr import compact_stats, long_row, packed_stats, three_values_wide_span, wide_row

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = np.uint64
LENGTHS = [1, 2, 63, 64, 65, 257, 1025, 4099]
BITS = [0, 3, 7, 30, 51, 55, 62]
CORRECTED, DOUBLE = 10, 11


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


class Box:
    """a context that collects its events instead of printing them"""

    def __init__(self, amd, mode="none", fmt="csr"):
        self.events, self.fatal = [], False
        self.ctx = amd.HIPContext(mode, fmt, on_event=self._on)

    def _on(self, ev, fatal):
        self.events.extend(ev)
        self.fatal = self.fatal or fatal

    def take(self):
        self.ctx._drain()
        ev, self.events, self.fatal = self.events, [], False
        return ev

    def vec(self, stored, offset=0):
        """a vector holding the given words; offset > 0: a view at that (odd) offset of a longer one"""
        stored = np.asarray(stored)
        n = len(stored)
        v = self.ctx.create_vector(n + offset)
        if offset:
            v = self.ctx.view_vector(v, offset, n)
        self.ctx.upload(v, stored.view(np.float64))
        return v

    def words(self, v):
        return self.ctx.download(v).view(U).copy()

    def matrix(self, cols, rows, vals, n, layout="stream"):
        return self.ctx.create_matrix(cols, rows, vals, n, len(vals), layout=layout)


def close(got, want, aw, bw):
    """test_vector_kernels' bar for a tree sum against the serial one: 1e-13 of the sum of the terms' magnitudes"""
    with np.errstate(all="ignore"):
        scale = float(np.abs(_vecc.strip(aw) * _vecc.strip(bw)).sum())
    return abs(got - want) <= 1e-13 * scale


def bits_of(x):
    return np.float64(x).view(U)


# ---- 1. codec ----

@pytest.mark.parametrize("offset", [0, 1, 3])
def test_encode_matches_the_model(amd, offset):
    box = Box(amd)
    for n in LENGTHS:
        raw = _vecc.salted(n, 100 + n)
        v = box.vec(raw.view(U), offset)
        box.ctx.encode_vector(v)
        assert np.array_equal(box.words(v), _vecc.encode(raw)), n
    assert box.take() == []
    box.ctx.close()


# ---- 2, 3. scrub ----

def test_scrub_repairs_every_single_flip(amd):
    box = Box(amd)
    clean = _vecc.encode(_vecc.salted(64 * 7, 2))
    v = box.vec(clean)
    for j in range(64):
        box.ctx.flip_vector(v, 7 * j + 3, [j])
    assert box.ctx.scrub_vector(v) == (64, 0)
    assert sorted(box.take()) == sorted((CORRECTED, 7 * j + 3, j) for j in range(64))
    assert np.array_equal(box.words(v), clean)
    assert box.ctx.scrub_vector(v) == (0, 0) and box.take() == []
    box.ctx.close()


def test_scrub_counts_double_flips_and_leaves_them(amd):
    box = Box(amd)
    rng = np.random.default_rng(3)
    clean = _vecc.encode(_vecc.salted(1025, 3))
    v = box.vec(clean, offset=1)
    bad = clean.copy()
    for i in rng.permutation(1025)[:40]:
        a, b = rng.choice(64, 2, replace=False)
        box.ctx.flip_vector(v, int(i), [int(a), int(b)])
        bad[i] ^= U((1 << int(a)) | (1 << int(b)))
    assert box.ctx.scrub_vector(v) == (0, 40)
    assert box.fatal and box.events[-1][0] == DOUBLE and all(e[0] == DOUBLE for e in box.events)
    box.take()
    assert np.array_equal(box.words(v), bad)
    box.ctx.close()


# ---- 4. kernels against the model ----

def ragged(n=2600, long_at=11, width=1100):
    """rows with 0-5 random entries, every seventh row empty, row `long_at` longer than one tile"""
    rng = np.random.default_rng(9)
    ent = set()
    for r in range(n):
        if r % 7 != 3:
            ent |= {(r, int(c)) for c in rng.integers(0, n, rng.integers(1, 6))}
    ent |= {(long_at, c) for c in range(2, 2 + width)}
    ent = sorted(ent)
    rows = np.array([e[0] for e in ent], np.uint32)
    cols = np.array([e[1] for e in ent], np.uint32)
    return cols, rows, rng.standard_normal(len(ent)), n


def check_spmv(amd, mode, mat, expect=None):
    cols, rows, vals, n = mat
    box = Box(amd, mode)
    A = box.matrix(cols, rows, vals, n)
    if expect is not None:
        expect(box.ctx, A)
    xw = _vecc.encode(np.random.default_rng(n).standard_normal(n))
    x, y = box.vec(xw), box.vec(np.zeros(n, U))
    want, fused = _vecc.spmv(*_vecc.csr_of(cols, rows, vals, n), xw)
    box.ctx.spmv_vecc(A, x, y)
    got_fused = box.ctx.dot_vecc(x, y)  # served from the SpMV's own product
    assert np.array_equal(box.words(y), want)
    assert np.array_equal(box.words(x), xw)
    assert close(got_fused, fused, xw[:n], want), (got_fused, fused)
    box.ctx.encode_vector(box.vec(np.zeros(1, U)))  # (any write: forgets the fused product)
    alone = box.ctx.dot_vecc(x, y)
    assert close(alone, fused, xw[:n], want), (alone, fused)
    assert box.take() == []
    box.ctx.close()


@pytest.mark.parametrize("mode", ["none", "constraints", "sed", "sec7", "sec8", "secded"])
def test_spmv_vecc_all_modes(amd, mode):
    check_spmv(amd, mode, laplace5(40, 40))


@pytest.mark.parametrize("mode", ["none", "secded"])
def test_spmv_vecc_ragged_rows_and_a_long_row(amd, mode):
    mat = ragged()
    assert np.bincount(mat[1], minlength=mat[3]).max() >= 1025 and (np.bincount(mat[1], minlength=mat[3]) == 0).any()
    check_spmv(amd, mode, mat)


def test_spmv_vecc_packed_compact_and_wide_blocks(amd):
    def packed(ctx, A):
        p, t, _ = packed_stats(ctx, A)
        assert p > 0

    def compact(ctx, A):
        (p, t, _), (c, _, _) = packed_stats(ctx, A), compact_stats(ctx, A)
        assert p < t and c > 0  # block 0: compact, not packed

    def wide(ctx, A):
        c, t, _ = compact_stats(ctx, A)
        assert c < t  # the block that spans more than 65536 columns

    check_spmv(amd, "none", laplace5(40, 40), packed)
    check_spmv(amd, "none", three_values_wide_span(), compact)
    check_spmv(amd, "none", wide_row(), wide)
    check_spmv(amd, "none", long_row())


@pytest.mark.parametrize("offset", [0, 1])
def test_vector_kernels_match_the_model(amd, offset):
    box = Box(amd)
    for n in LENGTHS:
        rng = np.random.default_rng(n)
        xw, rw, pw, ww = (_vecc.encode(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)) for _ in range(4))
        x, r, p, w = (box.vec(a, offset) for a in (xw, rw, pw, ww))
        assert close(box.ctx.dot_vecc(p, w), _vecc.dot(pw, ww), pw, ww), n
        alpha, beta = 0.37251, -1.3125e-3
        xs, rs, rr = _vecc.calc_xr(xw, rw, pw, ww, alpha)
        got = box.ctx.calc_xr_vecc(x, r, p, w, alpha)
        assert np.array_equal(box.words(x), xs) and np.array_equal(box.words(r), rs), n
        assert close(got, rr, rs, rs), (n, got, rr)
        assert bits_of(got) == bits_of(box.ctx.dot_vecc(r, r)), n  # r.r is dot_vecc(r, r) of the r it leaves
        box.ctx.calc_p_vecc(p, r, beta)
        assert np.array_equal(box.words(p), _vecc.calc_p(pw, rs, beta)), n
        assert np.array_equal(box.words(w), ww), n
    assert box.take() == []
    box.ctx.close()


# ---- 5. a flip in each operand of each entry ----

SPMV_FLIPS = {
    # an interior point: five rows gather it, and row `at` reads it for the fused product (general path)
    "secded-laplace": ("secded", lambda: laplace5(40, 40), 20 * 40 + 20),
    "packed-laplace": ("none", lambda: laplace5(40, 40), 20 * 40 + 20),  # every block packed
    "compact-and-packed": ("none", three_values_wide_span, 20000),  # row 1 (block 0: compact) and rows 19999-20001 (packed)
    "wide": ("none", wide_row, 69999),  # row 1's block spans more than 65536 columns
    # row 5 is walked tile by tile: it gathers x[5] in its first tile and reads it for its fused product
    "long-row-none": ("none", long_row, 5),
    "long-row-secded": ("secded", long_row, 5),
}


@pytest.mark.parametrize("case", sorted(SPMV_FLIPS))
def test_flips_in_the_spmv_input(amd, case):
    mode, make, at = SPMV_FLIPS[case]
    cols, rows, vals, n = make()
    assert np.count_nonzero(cols == at) >= 3
    box = Box(amd, mode)
    A = box.matrix(cols, rows, vals, n)
    xw = _vecc.encode(np.random.default_rng(1).standard_normal(n))
    x, y = box.vec(xw), box.vec(np.zeros(n, U))
    box.ctx.spmv_vecc(A, x, y)
    pw0 = box.ctx.dot_vecc(x, y)
    y0 = box.words(y)
    for bit in BITS:
        box.ctx.flip_vector(x, at, [bit])
        box.ctx.upload(y, np.zeros(n))
        box.ctx.spmv_vecc(A, x, y)
        pw = box.ctx.dot_vecc(x, y)
        assert box.take() == [(CORRECTED, at, bit)], bit
        assert np.array_equal(box.words(y), y0) and bits_of(pw) == bits_of(pw0), bit
        flipped = xw.copy()
        flipped[at] ^= U(1 << bit)
        assert np.array_equal(box.words(x), flipped), bit  # the input is not written back
        box.ctx.flip_vector(x, at, [bit])
    box.ctx.close()


def test_flip_in_a_matrix_element_and_in_the_entry_it_gathers(amd):
    """the matrix element fails its own check and is repaired in the SpMV's cold loop, which gathers -- and
    decodes -- the vector entry again"""
    cols, rows, vals, n = laplace5(40, 40)
    at = 20 * 40 + 20
    elem = int(np.flatnonzero((cols == at) & (rows == at - 1))[0])
    box = Box(amd, "secded")
    A = box.matrix(cols, rows, vals, n)
    xw = _vecc.encode(np.random.default_rng(1).standard_normal(n))
    x, y = box.vec(xw), box.vec(np.zeros(n, U))
    box.ctx.spmv_vecc(A, x, y)
    pw0 = box.ctx.dot_vecc(x, y)
    y0 = box.words(y)
    box.ctx.inject_at(A, elem, [37])
    box.ctx.flip_vector(x, at, [55])
    box.ctx.spmv_vecc(A, x, y)
    pw = box.ctx.dot_vecc(x, y)
    assert sorted(box.take()) == [(2, elem, 37), (CORRECTED, at, 55)]
    assert np.array_equal(box.words(y), y0) and bits_of(pw) == bits_of(pw0)
    box.ctx.close()


@pytest.mark.parametrize("n,at", [(1025, 1024), (4099, 2048)])
def test_flips_in_the_vector_kernels(amd, n, at):
    box = Box(amd)
    rng = np.random.default_rng(n)
    clean = [_vecc.encode(rng.standard_normal(n)) for _ in range(4)]
    alpha, beta = 0.71, 0.125
    ref = [box.vec(a) for a in clean]
    dot0 = box.ctx.dot_vecc(ref[2], ref[3])
    rr0 = box.ctx.calc_xr_vecc(*ref, alpha)
    x0, r0 = box.words(ref[0]), box.words(ref[1])
    box.ctx.calc_p_vecc(ref[2], ref[1], beta)
    p0 = box.words(ref[2])
    assert box.take() == []
    for bit in BITS:
        for op in range(2):  # dot_vecc(a, b): neither is written back
            v = [box.vec(clean[2]), box.vec(clean[3])]
            box.ctx.flip_vector(v[op], at, [bit])
            assert bits_of(box.ctx.dot_vecc(*v)) == bits_of(dot0)
            assert box.take() == [(CORRECTED, at, bit | op << 8)], (bit, op)
            flipped = clean[2 + op].copy()
            flipped[at] ^= U(1 << bit)
            assert np.array_equal(box.words(v[op]), flipped) and np.array_equal(box.words(v[1 - op]), clean[3 - op])
        for op in range(4):  # calc_xr_vecc(x, r, p, w): x and r come out repaired, p and w keep the flip
            v = [box.vec(a) for a in clean]
            box.ctx.flip_vector(v[op], at, [bit])
            assert bits_of(box.ctx.calc_xr_vecc(*v, alpha)) == bits_of(rr0)
            assert box.take() == [(CORRECTED, at, bit | op << 8)], (bit, op)
            assert np.array_equal(box.words(v[0]), x0) and np.array_equal(box.words(v[1]), r0)
            for k in (2, 3):
                flipped = clean[k].copy()
                if k == op:
                    flipped[at] ^= U(1 << bit)
                assert np.array_equal(box.words(v[k]), flipped), (bit, op, k)
        for op in range(2):  # calc_p_vecc(p, r): p comes out repaired, r keeps the flip
            p, r = box.vec(clean[2]), box.vec(r0)
            box.ctx.flip_vector((p, r)[op], at, [bit])
            box.ctx.calc_p_vecc(p, r, beta)
            assert box.take() == [(CORRECTED, at, bit | op << 8)], (bit, op)
            assert np.array_equal(box.words(p), p0)
            flipped = r0.copy()
            if op:
                flipped[at] ^= U(1 << bit)
            assert np.array_equal(box.words(r), flipped)
    box.ctx.close()


# ---- 6. the fused product serves its own kind only ----

def test_fused_product_is_not_shared_between_plain_and_protected(amd):
    cols, rows, vals, n = laplace5(40, 40)
    box = Box(amd)
    A = box.matrix(cols, rows, vals, n)
    pw = _vecc.encode(np.random.default_rng(4).standard_normal(n))
    p, w, other = box.vec(pw), box.vec(np.zeros(n, U)), box.vec(np.zeros(1, U))
    # a plain dot after spmv_vecc: the standalone plain dot's bits (it sums the stored words, code bits included)
    box.ctx.spmv_vecc(A, p, w)
    box.ctx.encode_vector(other)  # forgets the fused product
    alone = box.ctx.dot(p, w)
    box.ctx.spmv_vecc(A, p, w)
    assert bits_of(box.ctx.dot(p, w)) == bits_of(alone)
    assert bits_of(alone) != bits_of(box.ctx.dot_vecc(p, w))  # (the two kinds do differ on these vectors)
    assert box.take() == []
    # a protected dot after a plain spmv: w holds no codewords, so the call reports what it sees -- the same
    # reports and the same bits as the standalone protected dot
    box.ctx.spmv(A, p, w)
    box.ctx.encode_vector(other)
    alone = box.ctx.dot_vecc(p, w)
    ev_alone = sorted(box.take())
    box.ctx.spmv(A, p, w)
    assert bits_of(box.ctx.dot_vecc(p, w)) == bits_of(alone)
    assert sorted(box.take()) == ev_alone and ev_alone
    box.ctx.close()


# ---- 7. refusals ----

def test_refusals_leave_every_vector_untouched(amd, monkeypatch):
    cols, rows, vals, n = laplace5(40, 40)
    marks = _vecc.encode(np.arange(1.0, n + 1.0))

    def refused(box, call, vecs, text):
        before = [box.words(v) for v in vecs]
        with pytest.raises(amd.AbftError, match=text):
            call()
        assert all(np.array_equal(box.words(v), b) for v, b in zip(vecs, before))

    box = Box(amd, "secded", "coo")
    A = box.ctx.create_matrix(cols, rows, vals, n, len(vals))
    x, y = box.vec(marks), box.vec(marks)
    refused(box, lambda: box.ctx.spmv_vecc(A, x, y), [x, y], "COO")
    box.ctx.close()
    for layout, name in (("panels", "panel"), ("sweep", "sweep")):
        monkeypatch.setenv("ABFT_HIP_LAYOUT", layout)
        box = Box(amd, "secded")
        A = box.matrix(cols, rows, vals, n, layout=None)
        assert box.ctx.matrix_info(A)[0] == layout
        x, y = box.vec(marks), box.vec(marks)
        refused(box, lambda: box.ctx.spmv_vecc(A, x, y), [x, y], name)
        box.ctx.close()
    monkeypatch.delenv("ABFT_HIP_LAYOUT")
    box = Box(amd, "secded")
    A = box.matrix(cols, rows, vals, n)
    big = box.vec(np.concatenate([marks, marks]))
    a, b, c, d = (box.vec(marks) for _ in range(4))
    short = box.vec(marks[:-1])
    lo, hi = box.ctx.view_vector(big, 0, n), box.ctx.view_vector(big, n - 1, n)  # share one element
    every = [big, a, b, c, d, short]
    refused(box, lambda: box.ctx.spmv_vecc(A, short, a), every, "shorter")
    refused(box, lambda: box.ctx.spmv_vecc(A, a, short), every, "shorter")
    refused(box, lambda: box.ctx.spmv_vecc(A, lo, hi), every, "overlap")
    refused(box, lambda: box.ctx.dot_vecc(a, short), every, "lengths differ")
    for k in range(4):
        v = [a, b, c, d]
        v[k] = short
        refused(box, lambda: box.ctx.calc_xr_vecc(*v, 0.5), every, "lengths differ")
    for v in ([lo, hi, c, d], [lo, b, hi, d], [lo, b, c, hi], [a, lo, hi, d], [a, lo, c, hi]):
        refused(box, lambda: box.ctx.calc_xr_vecc(*v, 0.5), every, "overlap")
    refused(box, lambda: box.ctx.calc_p_vecc(a, short, 0.5), every, "lengths differ")
    refused(box, lambda: box.ctx.calc_p_vecc(lo, hi, 0.5), every, "overlap")
    assert box.take() == []
    box.ctx.close()


# ---- 8, 9. cg_solve(vector_ecc=True) ----

class Solve:
    """one solve of laplace5:40,40 with the reference's b; `flip`: (vector name, index, bits, when) with when
    'start' (b: once it is protected / uploaded), 'dot' (w: behind the 12th p.w, where it is live: written by
    the SpMV, about to be read by calc_xr; abft_hip_vector_flip forgets the fused product, so a flip in front of
    the dot would also turn the served dot into a standalone one) or
    'iteration' (after iteration 10)"""

    def __init__(self, amd, ecc, conv, flip=None, collect=True):
        cols, rows, vals, n = laplace5(40, 40)
        self.b = rhs(n, 1)
        # (collect = False: events are printed and a fatal one raises, as for any caller without a handler)
        ctx = amd.HIPContext("secded", "csr", on_event=(lambda ev, fatal: None) if collect else None)
        A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        v = dict(zip("bxrpw", (ctx.create_vector(n) for _ in range(5))))
        ctx.upload(v["b"], self.b)
        ctx.upload(v["x"], np.zeros(n))
        self.hist = []
        name, index, bits, when = flip or (None, 0, [], None)
        if when == "start":
            if ecc:
                encode = ctx.encode_vector

                def encode_then_flip(vec):
                    encode(vec)
                    if vec is v["b"]:
                        ctx.flip_vector(vec, index, bits)
                ctx.encode_vector = encode_then_flip
            else:
                ctx.flip_vector(v["b"], index, bits)
        if when == "dot":
            attr = "dot_vecc" if ecc else "dot"
            dot, calls = getattr(ctx, attr), [0]

            def dot_then_flip(a, b):
                out = dot(a, b)
                calls[0] += b is v["w"]
                if b is v["w"] and calls[0] == 12:
                    ctx.flip_vector(v[name], index, bits)
                return out
            setattr(ctx, attr, dot_then_flip)

        def on_iteration(itr, rr):
            self.hist.append(rr)
            if when == "iteration" and itr == 10:
                ctx.flip_vector(v[name], index, bits)

        self.itr, self.rr = amd.cg_solve(ctx, A, v["b"], v["x"], v["r"], v["p"], v["w"], 1000, conv,
                                         on_iteration=on_iteration, **({"vector_ecc": True} if ecc else {}))
        self.x = ctx.download(v["x"])
        self.b_after = ctx.download(v["b"])
        self.events = list(ctx.event_log)
        self.A = _vecc.csr_of(cols, rows, vals, n)
        ctx.close()

    def residual(self, x):
        rowptr, cols, vals = self.A
        ax = np.add.reduceat(vals * x[cols], rowptr[:-1])
        return float(np.linalg.norm(self.b - ax))

    def same_as(self, other):
        return self.itr == other.itr and np.array_equal(np.array(self.hist).view(U), np.array(other.hist).view(U)) \
            and np.array_equal(self.x.view(U), other.x.view(U))


@pytest.fixture(scope="module")
def clean_solves(amd):
    return {(ecc, conv): Solve(amd, ecc, conv) for ecc in (False, True) for conv in (1e-3, 1e-10)}


@pytest.mark.parametrize("conv", [1e-3, 1e-10])
def test_clean_protected_solve(amd, clean_solves, conv):
    from abft_sparse_cg_amd.context import threshold_ambiguous, vecc_strip
    plain, prot = clean_solves[False, conv], clean_solves[True, conv]
    print("iterations: plain %d, protected %d" % (plain.itr, prot.itr))
    res_plain, res_prot = plain.residual(plain.x), prot.residual(vecc_strip(prot.x))
    print("residuals: plain %.6e, protected %.6e" % (res_plain, res_prot))
    if not any(threshold_ambiguous(rr, conv) for rr in plain.hist[-1:]):
        assert abs(prot.itr - plain.itr) <= max(1, 0.02 * plain.itr)
    assert res_prot <= 10 * res_plain
    assert prot.events == []
    # what the caller downloads are codewords
    assert not _vecc.decode(prot.x.view(U))[1].any() and not _vecc.decode(prot.b_after.view(U))[1].any()
    assert np.array_equal(_vecc.strip(prot.b_after.view(U)), _vecc.strip(_vecc.encode(prot.b)))


FLIPS = [("p", 777, [55], "iteration"), ("x", 801, [62], "iteration"), ("x", 801, [52], "iteration"),
         ("r", 802, [62], "iteration"), ("r", 802, [52], "iteration"), ("w", 803, [62], "dot"),
         ("w", 803, [52], "dot"), ("b", 804, [40], "start")]
# the events of each flip: (operand of the entry that meets it) per report
REPORTS = {"p": [0, 2, 0], "x": [0], "r": [1], "w": [3], "b": [0, 0]}


@pytest.mark.parametrize("flip", FLIPS, ids=lambda f: "%s%d" % (f[0], f[2][0]))
def test_protected_solve_under_a_flip_is_the_clean_solve(amd, clean_solves, flip):
    name, index, bits, _ = flip
    clean = clean_solves[True, 1e-10]
    hit = Solve(amd, True, 1e-10, flip)
    assert hit.same_as(clean)
    assert np.array_equal(hit.b_after.view(U), clean.b_after.view(U))
    assert hit.events == [(CORRECTED, index, bits[0] | op << 8) for op in REPORTS[name]]
    # without protection the same flip changes the run
    plain = Solve(amd, False, 1e-10, flip)
    assert plain.events == [] and not plain.same_as(clean_solves[False, 1e-10])


def test_double_flip_in_r_is_fatal(amd, capfd):
    with pytest.raises(amd.FatalEvent):
        Solve(amd, True, 1e-10, ("r", 802, [52, 17], "iteration"), collect=False)
    assert "[ECC] double-bit error detected in vector operand 1 at index 802\n" in capfd.readouterr().out


# ---- 10. the command line ----

def cli(args):
    p = subprocess.run([sys.executable, "-m", "abft_sparse_cg_amd.cg", "-t", "hip", "-m", "secded", "-s",
                        "laplace5:40,40", "-i", "300", "-c", "1e-8"] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return re.sub(r"time taken = .*", "time taken", p.stdout)


def test_cli_vector_ecc(amd):
    plain = cli([])
    clean = cli(["--vector-ecc", "secded"])
    hit = cli(["--vector-ecc", "secded", "--flip-vector", "10:p:777:55"])
    assert "vector protection" not in plain and "vector operand" not in plain
    assert clean.count("vector protection: secded (64, 57)\n") == 1 and "[ECC]" not in clean
    assert clean.index("vector protection") < clean.index("iteration     0")
    want = ["[ECC] corrected bit 55 of vector operand %d at index 777" % op for op in (0, 2, 0)]
    assert [ln for ln in hit.split("\n") if ln.startswith("[ECC]")] == want
    assert "*** flipping bit 55 of p[777] ***" in hit
    ran = re.search(r"ran for (\d+) iterations", clean).group(0)
    assert ran in hit
    # apart from the flip and its reports the two transcripts are the same run
    drop = lambda s: [ln for ln in s.split("\n") if not ln.startswith(("[ECC]", "***"))]  # noqa: E731
    assert drop(hit) == drop(clean)
