"""Protected vectors where tests/test_gpu_vector_ecc.py does not reach: the four
protected calls on IEEE special values and on elements crafted to show a wrong truncation, many flips in one
call -- every bit of the word, every way the kernels walk a vector, views at an odd offset, several operands,
double flips --, flips in the SpMV's input beyond one gathered entry, reductions over 66 workgroups, and a
flipped entry of a dense ("hub") column, which more threads gather than the event queue has slots.

Stored words are compared by _vecc.assert_words (bit for bit, NaN payloads aside, every word a codeword), sums
by check_sum below: against the exact sum of the terms the model's stored words give, within the bound of the
kernel's summation tree (_ieee.sum_bound) -- derived, not measured.  tests/test_vector_ecc_edges_host.py checks
the inputs used here and the model on them."""
import math

import numpy as np
import pytest

import _ieee as I
import _vecc
from _oracle import laplace5, rhs
from test_gpu_packed_csr import long_row, packed_stats
from test_gpu_vector_ecc import CORRECTED, DOUBLE, Box, bits_of

pytestmark = pytest.mark.gpu

U = np.uint64
MATRIX_CORRECTED = 2  # ABFT_EV_CORRECTED_BIT
# a fused SpMV partial sums at most a workgroup's rows, each thread a share of them; at most 8192 partials are
# folded by one workgroup: the figures of test_gpu_special_values.py
ROWS_PER_THREAD, NBLK = 1024, 8192
ALIGN = {"aligned": (0, 0, 0, 0), "odd": (1, 1, 1, 1), "p-odd": (0, 0, 1, 0)}  # offsets of x, r, p, w


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def check_sum(got, terms, depth, what=""):
    """The comparison rule for sums.  A NaN term, or +Inf with -Inf: NaN.  Else a +-Inf term: that infinity.
    Else, when sum |terms| < DBL_MAX / 2 (no partial sum can overflow): within sum_bound of the exact sum.
    Else: finite and within the bound, or an infinity."""
    terms = np.asarray(terms, dtype=np.float64)
    want = I.exact_sum(terms)
    if not np.isfinite(terms).all():
        assert I.value_class(got) == I.value_class(want), (what, got, want)
        return
    down = 2.0 ** -64  # sum |terms| itself may overflow: the comparison is made on 2^-64 of everything
    mag = math.fsum(np.abs(terms * down).tolist())
    if mag < I.DBL_MAX / 2 * down:
        assert abs(got - want) <= I.sum_bound(terms, depth), (what, got, want, I.sum_bound(terms, depth))
    elif not math.isinf(got):
        assert math.isfinite(got) and math.isfinite(want), (what, got, want)
        assert abs(got * down - want * down) <= (depth + 1) * I.U * mag + len(terms) * I.TINY, (what, got, want)


def products(aw, bw):
    with np.errstate(all="ignore"):
        return _vecc.strip(aw) * _vecc.strip(bw)


def take(box):
    """-> (events, fatal) of everything queued so far"""
    box.ctx._drain()
    fatal = box.fatal
    return box.take(), fatal


def put(box, vec, stored):
    box.ctx.upload(vec, np.asarray(stored, dtype=U).view(np.float64))


def run_xr(box, vec, stored, alpha, depth, what):
    """one calc_xr_vecc on the given stored words, against the model; -> the words of r it left"""
    for v, a in zip(vec, stored):
        put(box, v, a)
    xs, rs, _ = _vecc.calc_xr(*stored, alpha)
    rr = box.ctx.calc_xr_vecc(*vec, alpha)
    got = [box.words(v) for v in vec]
    _vecc.assert_words(got[0], xs, (what, "x"))
    _vecc.assert_words(got[1], rs, (what, "r"))
    assert np.array_equal(got[2], stored[2]) and np.array_equal(got[3], stored[3]), what  # p and w are only read
    terms = products(rs, rs)
    check_sum(rr, terms, depth, (what, "r.r"))
    alone = box.ctx.dot_vecc(vec[1], vec[1])
    check_sum(alone, terms, depth, (what, "dot(r, r)"))
    print("%s: r.r %r, dot_vecc(r, r) %r, exact %r" % (what, rr, alone, I.exact_sum(terms)))
    assert (rr != rr) == (alone != alone), what
    if rr == rr:
        assert bits_of(rr) == bits_of(alone), what  # r.r is dot_vecc(r, r) of the r it leaves
    return got[0], got[1]


def run_p(box, p, r, pw, rw, beta, what):
    put(box, p, pw)
    put(box, r, rw)
    box.ctx.calc_p_vecc(p, r, beta)
    got = box.words(p)
    _vecc.assert_words(got, _vecc.calc_p(pw, rw, beta), (what, "p"))
    assert np.array_equal(box.words(r), rw), what  # r is only read
    return got


# ---- A1. the arithmetic kernels on special values ----

@pytest.mark.parametrize("align", sorted(ALIGN))
@pytest.mark.parametrize("fam", sorted(_vecc.FAMILIES))
def test_vector_kernels_on_special_values(amd, fam, align):
    box = Box(amd)
    for n in _vecc.EDGE_LENGTHS:
        stored = [_vecc.family(fam, n, _vecc.operand_seed(n, k)) for k in range(4)]
        vec = [box.vec(a, o) for a, o in zip(stored, ALIGN[align])]
        depth = I.dot_depth(n)
        for a, b in ((2, 3), (0, 1), (3, 3)):
            check_sum(box.ctx.dot_vecc(vec[a], vec[b]), products(stored[a], stored[b]), depth, (fam, n, "dot", a, b))
            assert all(np.array_equal(box.words(v), s) for v, s in zip(vec, stored))
        for s in _vecc.SCALARS:
            _, r = run_xr(box, vec, stored, s, depth, (fam, align, n, s))
            run_p(box, vec[2], vec[1], stored[2], r, s, (fam, align, n, s))
    assert take(box) == ([], False)
    box.ctx.close()


def stated(word, want):
    """the stored word holds the value the table states: its codeword (any NaN codeword for a NaN)"""
    if want != want:
        return bool(np.isnan(_vecc.strip(np.array([word], U))[0])) and _vecc.decode(np.array([word], U))[1][0] == 0
    return int(word) == int(_vecc.encode(np.array([want]))[0])


@pytest.mark.parametrize("align", sorted(ALIGN))
def test_crafted_elements(amd, align):
    box = Box(amd)
    for n in _vecc.EDGE_LENGTHS:
        base = [_vecc.family("finite", n, _vecc.operand_seed(n, k)) for k in range(4)]
        vec = [box.vec(a, o) for a, o in zip(base, ALIGN[align])]
        for alpha, rows in _vecc.crafted_calls(n):
            stored = [a.copy() for a in base]
            for i, (x, p, _, _, _) in rows.items():
                stored[0][i] = stored[1][i] = _vecc.encode(np.array([x]))[0]
                stored[2][i] = _vecc.encode(np.array([p]))[0]
                stored[3][i] = _vecc.encode(np.array([-p]))[0]  # r -= alpha w is r += alpha p
            xs, rs = run_xr(box, vec, stored, alpha, I.dot_depth(n), ("crafted", align, n, alpha))
            ps = run_p(box, vec[2], vec[1], stored[2], stored[1], alpha, ("crafted", align, n, alpha))
            for i, (_, _, _, want, what) in rows.items():
                assert stated(xs[i], want) and stated(rs[i], want) and stated(ps[i], want), \
                    (what, n, i, hex(int(xs[i])), hex(int(rs[i])), hex(int(ps[i])))
    assert take(box) == ([], False)
    box.ctx.close()


# ---- A2. spmv_vecc on special values ----

def special_spmv_input(name):
    if name == "special":
        B = I.special_matrix()
        assert B.crafted["empty"]
        return B.csr(), B.x
    if name == "tile-edge":
        B, _ = I.tile_edge_matrix()
        return B.csr(), B.x
    mat = laplace5(40, 40)
    return mat, I.special_vector(mat[3], 5)


@pytest.mark.parametrize("name,mode", [("special", "none"), ("special", "secded"), ("tile-edge", "none"),
                                       ("tile-edge", "secded"), ("laplace-packed", "none")])
def test_spmv_vecc_on_special_values(amd, name, mode):
    (cols, rows, vals, n), xv = special_spmv_input(name)
    box = Box(amd, mode)
    A = box.matrix(cols, rows, vals, n)
    if name == "laplace-packed":
        p, t, _ = packed_stats(box.ctx, A)
        assert p == t > 0  # every block packed
    xw = _vecc.encode(xv)
    assert {I.value_class(v) for v in _vecc.strip(xw)} >= ({"+inf"} if name == "tile-edge" else {"nan", "+inf", "-inf"})
    x, y = box.vec(xw), box.vec(_vecc.encode(np.full(n, 7.0)))
    want, _ = _vecc.spmv(*_vecc.csr_of(cols, rows, vals, n), xw)
    empty = np.bincount(rows, minlength=n) == 0
    assert (want[empty] == 0).all()  # the codeword of +0.0
    box.ctx.spmv_vecc(A, x, y)
    fused = box.ctx.dot_vecc(x, y)  # served from the SpMV's own product
    _vecc.assert_words(box.words(y), want, (name, mode))
    assert np.array_equal(box.words(x), xw)
    terms = products(xw[:n], want)
    print("%s %s: fused %r, exact %r" % (name, mode, fused, I.exact_sum(terms)))
    check_sum(fused, terms, I.fused_depth(ROWS_PER_THREAD, NBLK), (name, mode, "fused"))
    box.ctx.encode_vector(box.vec(np.zeros(1, U)))  # (any write: forgets the fused product)
    check_sum(box.ctx.dot_vecc(x, y), terms, I.dot_depth(n), (name, mode, "alone"))
    assert take(box) == ([], False)
    box.ctx.close()


# ---- A3. flips in the vector kernels: positions, bits, alignments, multiplicity ----

OPERANDS = {"dot": 2, "xr": 4, "p": 2}


class VectorCase:
    """the three vector kernels on one set of clean vectors of n elements, each vector at `offset`: the clean
    calls' results, and the same calls with flips put in first"""

    def __init__(self, amd, n, offset, seed=0):
        self.box, self.n = Box(amd), n
        rng = np.random.default_rng(n + seed)
        self.clean = [_vecc.encode(rng.standard_normal(n)) for _ in range(4)]
        self.alpha, self.beta = 0.71, 0.125
        self.vec = [self.box.vec(a, offset) for a in self.clean]
        out = self.run("dot", [])
        self.dot0 = out[0]
        out = self.run("xr", [])
        self.rr0, (self.x0, self.r0) = out[0], out[1][:2]
        self.p0 = self.run("p", [])[1][0]
        # the clean calls against the model
        xs, rs, _ = _vecc.calc_xr(*self.clean, self.alpha)
        assert np.array_equal(self.x0, xs) and np.array_equal(self.r0, rs)
        assert np.array_equal(self.p0, _vecc.calc_p(self.clean[2], rs, self.beta))
        check_sum(self.dot0, products(self.clean[2], self.clean[3]), I.dot_depth(n), "p.w")
        check_sum(self.rr0, products(rs, rs), I.dot_depth(n), "r.r")

    def inputs(self, kernel):
        """the stored words a call of the kernel starts from, in the order of its operands"""
        if kernel == "dot":
            return [self.clean[2], self.clean[3]]
        if kernel == "xr":
            return list(self.clean)
        return [self.clean[2], self.r0]

    def run(self, kernel, flips):
        """flips: [(operand, index, bits)] -> (the call's scalar, the words of its operands behind it, events, fatal)"""
        ctx = self.box.ctx
        vec = self.vec[:OPERANDS[kernel]]
        for v, a in zip(vec, self.inputs(kernel)):
            put(self.box, v, a)
        for op, i, bits in flips:
            ctx.flip_vector(vec[op], i, bits)
        if kernel == "dot":
            val = ctx.dot_vecc(*vec)
        elif kernel == "xr":
            val = ctx.calc_xr_vecc(*vec, self.alpha)
        else:
            val = ctx.calc_p_vecc(vec[0], vec[1], self.beta)
        ev, fatal = take(self.box)
        return val, [self.box.words(v) for v in vec], ev, fatal

    def check(self, kernel, flips, out, lost=None):
        """outputs and the sum carry the clean call's bits, operands that are only read keep their flips;
        lost: the index of a word with two flipped bits -- what a written vector holds there, and the sum, are
        unspecified"""
        val, got = out[0], out[1]
        want = [a.copy() for a in self.inputs(kernel)]
        for op, i, bits in flips:
            for b in bits:
                want[op][i] ^= U(1 << b)
        if kernel == "xr":
            want[0], want[1] = self.x0.copy(), self.r0.copy()
        if kernel == "p":
            want[0] = self.p0.copy()
        written = {"dot": 0, "xr": 2, "p": 1}[kernel]
        for k in range(OPERANDS[kernel]):
            if lost is not None and k < written:
                got[k][lost] = want[k][lost]
            assert np.array_equal(got[k], want[k]), (kernel, flips, k, np.flatnonzero(got[k] != want[k])[:8])
        if lost is None and kernel != "p":
            assert bits_of(val) == bits_of(self.dot0 if kernel == "dot" else self.rr0), (kernel, flips)

    def close(self):
        self.box.ctx.close()


def events_of(flips):
    return sorted((CORRECTED, i, b | op << 8) for op, i, bits in flips for b in bits)


@pytest.fixture(scope="module", params=[0, 1], ids=["aligned", "odd-view"])
def case(request, amd):
    c = VectorCase(amd, _vecc.FLIP_N, request.param)
    yield c
    c.close()


@pytest.mark.parametrize("pattern", ["sweep", "walk"])
@pytest.mark.parametrize("kernel", sorted(OPERANDS))
def test_many_flips_in_one_operand(case, kernel, pattern):
    """every bit of the word at once, each in an element of its own over the three workgroups; and one flip per
    way the kernels meet an element: both halves of the first pair, three rounds of one thread, the last
    pair, the odd tail.  Indices are indices inside the view."""
    places = _vecc.SWEEP if pattern == "sweep" else _vecc.WALK
    for op in range(OPERANDS[kernel]):
        flips = [(op, i, [b]) for i, b in places]
        out = case.run(kernel, flips)
        assert (sorted(out[2]), out[3]) == (events_of(flips), False), (kernel, op)
        case.check(kernel, flips, out)


def test_flips_in_several_operands(case):
    i = 1536
    for flips in ([(0, i, [9]), (2, i, [50])],  # x[i] and p[i]
                  [(1, i, [0]), (3, i + 1, [63])],  # the partners of one pair in different operands
                  [(0, i, [5]), (1, i, [22]), (2, i, [41]), (3, i, [62])],
                  [(0, i, [33]), (1, i, [33]), (2, i, [33]), (3, i, [33])]):  # the same bit: operands apart in the report
        out = case.run("xr", flips)
        assert (sorted(out[2]), out[3]) == (events_of(flips), False), flips
        case.check("xr", flips, out)


@pytest.mark.parametrize("kernel", sorted(OPERANDS))
def test_double_flips(case, kernel):
    i = 1537  # the second element of a pair (test_vector_ecc_edges_host.py), not the tail
    for op in range(OPERANDS[kernel]):
        flips = [(op, i, [13, 44])]
        out = case.run(kernel, flips)
        assert (out[2], out[3]) == ([(DOUBLE, i, op << 8)], True), (kernel, op, out[2])
        case.check(kernel, flips, out, lost=i)


@pytest.mark.parametrize("kernel", sorted(OPERANDS))
def test_single_flip_below_a_double_flip(case, kernel):
    """the drain hands over the corrected event, then the fatal one, and is cut there"""
    op = OPERANDS[kernel] - 1
    flips = [(op, 100, [9]), (op, 1537, [13, 44]), (op, 3000, [27])]
    out = case.run(kernel, flips)
    assert (out[2], out[3]) == ([(CORRECTED, 100, 9 | op << 8), (DOUBLE, 1537, op << 8)], True), out[2]
    case.check(kernel, flips, out, lost=1537)
    assert take(case.box) == ([], False)  # the cut events are gone, not left for the next drain


# ---- A4. flips in the spmv_vecc input beyond one gathered entry ----

N4, UNREAD, SHARED, EMPTY = 700, 333, 500, 420


def gather_matrix():
    """700 x 700, rows of up to four entries; no element lies in column UNREAD (its row is not empty), column
    SHARED is gathered by several rows, row EMPTY has no element (its column is gathered)"""
    ent = set()
    for r in range(N4):
        if r != EMPTY:
            ent |= {(r, max(r - 1, 0)), (r, r), (r, min(r + 1, N4 - 1)), (r, (7 * r + 3) % N4)}
    ent |= {(r, SHARED) for r in (10, 200, 650)}
    ent = sorted(e for e in ent if e[1] != UNREAD)
    rows = np.array([e[0] for e in ent], np.uint32)
    cols = np.array([e[1] for e in ent], np.uint32)
    assert not (cols == UNREAD).any() and (rows == UNREAD).any() and not (rows == EMPTY).any()
    assert np.count_nonzero(cols == SHARED) >= 5 and np.count_nonzero(cols == EMPTY) >= 2
    return cols, rows, np.random.default_rng(4).standard_normal(len(ent)), N4


class SpmvCase:
    def __init__(self, amd, mode, mat, **kw):
        self.cols, self.rows, self.vals, self.n = mat
        self.box = Box(amd, mode)
        if kw:
            self.A = self.box.ctx.create_matrix(self.cols, self.rows, self.vals, self.n, len(self.vals), **kw)
            assert self.box.ctx.vecc_supported(self.A)
        else:
            self.A = self.box.matrix(*mat)
        self.n_in = kw.get("n_in", self.n)
        self.xw = _vecc.encode(np.random.default_rng(1).standard_normal(self.n_in))
        self.x, self.y = self.box.vec(self.xw), self.box.vec(np.zeros(self.n, U))

    def run(self, flips=(), dot=True):
        """-> (y words, the product behind the SpMV, x words, events, fatal)"""
        ctx = self.box.ctx
        put(self.box, self.x, self.xw)
        put(self.box, self.y, np.zeros(self.n, U))
        for i, bits in flips:
            ctx.flip_vector(self.x, i, bits)
        ctx.spmv_vecc(self.A, self.x, self.y)
        pw = ctx.dot_vecc(self.x, self.y) if dot else None
        ev, fatal = take(self.box)
        return self.box.words(self.y), pw, self.box.words(self.x), ev, fatal

    def flipped(self, flips):
        w = self.xw.copy()
        for i, bits in flips:
            for b in bits:
                w[i] ^= U(1 << b)
        return w


@pytest.mark.parametrize("mode", ["none", "secded"])
def test_flips_in_read_and_unread_entries_of_the_spmv_input(amd, mode):
    c = SpmvCase(amd, mode, gather_matrix())
    y0, pw0, _, ev, _ = c.run()
    assert ev == []
    assert np.array_equal(y0, _vecc.spmv(*_vecc.csr_of(c.cols, c.rows, c.vals, c.n), c.xw)[0])
    flips = [(UNREAD, [7]), (SHARED, [0]), (EMPTY, [63])]
    y, pw, x, ev, fatal = c.run(flips)
    # the fused product reads x[row] of every row: each flipped entry once, however many rows gather it
    assert (ev, fatal) == (sorted((CORRECTED, i, b[0]) for i, b in flips), False)
    assert np.array_equal(y, y0) and bits_of(pw) == bits_of(pw0) and np.array_equal(x, c.flipped(flips))
    flips = [(SHARED, [19, 40])]
    y, _, x, ev, fatal = c.run(flips)
    assert (ev, fatal) == ([(DOUBLE, SHARED, 0)], True)
    assert np.array_equal(x, c.flipped(flips))
    c.box.ctx.close()


@pytest.mark.parametrize("mode", ["none", "secded"])
def test_flip_first_gathered_in_a_later_tile_of_a_long_row(amd, mode):
    mat = long_row()
    at = I.csr_tile() + 100  # row 5 gathers it in its second tile; rows at - 1, at, at + 1 as well
    assert at < 1500 and np.count_nonzero(mat[0] == at) == 4
    c = SpmvCase(amd, mode, mat)
    y0, pw0, _, ev, _ = c.run()
    assert ev == []
    flips = [(at, [30]), (5, [12])]  # (and the long row's own entry: gathered in its first tile, read for its product)
    y, pw, x, ev, fatal = c.run(flips)
    assert (ev, fatal) == ([(CORRECTED, 5, 12), (CORRECTED, at, 30)], False)
    assert np.array_equal(y, y0) and bits_of(pw) == bits_of(pw0) and np.array_equal(x, c.flipped(flips))
    c.box.ctx.close()


@pytest.mark.parametrize("mode", ["none", "secded"])
def test_without_the_fused_product_only_gathered_entries_are_reported(amd, mode, monkeypatch):
    monkeypatch.setenv("ABFT_HIP_FUSE_DOT", "0")
    c = SpmvCase(amd, mode, gather_matrix())
    y0 = c.run(dot=False)[0]
    flips = [(UNREAD, [7]), (SHARED, [0]), (EMPTY, [63])]
    y, _, x, ev, fatal = c.run(flips, dot=False)
    assert (ev, fatal) == ([(CORRECTED, EMPTY, 63), (CORRECTED, SHARED, 0)], False)
    assert np.array_equal(y, y0) and np.array_equal(x, c.flipped(flips))
    # the stand-alone dot behind it reads all of x
    pw0 = c.run()[1]
    y, pw, x, ev, fatal = c.run(flips)
    assert (ev, fatal) == (sorted((CORRECTED, i, b[0]) for i, b in flips), False)
    assert np.array_equal(y, y0) and bits_of(pw) == bits_of(pw0)
    c.box.ctx.close()


def test_flips_in_a_rectangular_shard(amd):
    """rows 15..24 of the grid as a shard: the matrix event carries the re-based element index, the vector
    event the column"""
    cols, rows, vals, n = laplace5(40, 40)
    r0, r1 = 15 * 40, 25 * 40
    m = (rows >= r0) & (rows < r1)
    base = int(np.argmax(m))
    assert base > 0
    c = SpmvCase(amd, "secded", (cols[m], rows[m] - r0, vals[m], r1 - r0), n_in=n, index_base=base)
    y0 = c.run(dot=False)[0]
    want = _vecc.spmv(*_vecc.csr_of(cols[m], rows[m] - r0, vals[m], r1 - r0), c.xw)[0]
    assert np.array_equal(y0, want)
    at = 20 * 40 + 20
    assert np.count_nonzero(cols[m] == at) == 5
    elem = 17
    c.box.ctx.inject_at(c.A, elem, [37])
    flips = [(at, [55])]
    y, _, x, ev, fatal = c.run(flips, dot=False)
    assert (sorted(ev), fatal) == ([(MATRIX_CORRECTED, base + elem, 37), (CORRECTED, at, 55)], False)
    assert np.array_equal(y, y0) and np.array_equal(x, c.flipped(flips))
    c.box.ctx.close()


# ---- A5. many workgroups ----

@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd-view"])
def test_reductions_over_66_workgroups(amd, offset):
    """133121 elements: 66 workgroups, ticket groups of 32, 32 and 2.  The sums against the exact sum: at this
    length the model's serial sum is itself off by a share of the bound (test_vector_ecc_edges_host.py)."""
    c = VectorCase(amd, _vecc.MANY_N, offset)  # (checks the clean calls against the model and the exact sums)
    for kernel in sorted(OPERANDS):
        nop = OPERANDS[kernel]
        flips = [(k % nop, i, [b]) for k, (i, b) in enumerate(_vecc.MANY_FLIPS)]
        out = c.run(kernel, flips)
        assert (sorted(out[2]), out[3]) == (events_of(flips), False), kernel
        c.check(kernel, flips, out)
    c.close()


# ---- A6. a flipped entry of a hub column ----

@pytest.mark.parametrize("mode", ["none", "secded"])
def test_flip_in_an_entry_that_more_rows_gather_than_the_queue_holds(amd, mode):
    from abft_sparse_cg_amd import capi
    cap = capi.load().abft_hip_event_capacity()
    n = cap + 64
    for dense, flips in ((1, [(0, [30])]), (2, [(0, [30]), (1, [30])])):
        mat = _vecc.arrow(n, dense)
        assert all(np.count_nonzero(mat[0] == i) > cap for i, _ in flips)
        c = SpmvCase(amd, mode, mat)
        y0, pw0, _, ev, fatal = c.run()
        assert (ev, fatal) == ([], False)
        want, _ = _vecc.spmv(*_vecc.csr_of(*mat), c.xw)
        assert np.array_equal(y0, want)
        check_sum(pw0, products(c.xw, want), I.fused_depth(ROWS_PER_THREAD, NBLK), "p.w")
        y, pw, x, ev, fatal = c.run(flips)  # (raises AbftError if the drain reports an overflow)
        assert (ev, fatal) == ([(CORRECTED, i, b[0]) for i, b in flips], False)
        assert np.array_equal(y, y0) and bits_of(pw) == bits_of(pw0) and np.array_equal(x, c.flipped(flips))
        if dense == 1:
            y, _, x, ev, fatal = c.run([(0, [30, 31])])
            assert (ev, fatal) == ([(DOUBLE, 0, 0)], True)
            assert np.array_equal(x, c.flipped([(0, [30, 31])]))
        c.box.ctx.close()


class ArrowSolve:
    """cg_solve(vector_ecc=True) on the symmetric arrow, as test_gpu_vector_ecc.py's Solve runs laplace5;
    flip: (vector name, index, bits), put in after iteration 2 -- the second one, on_iteration's 1: the
    matrix has three distinct eigenvalues (4 is one n - 2 times over), so CG is done after its third"""

    def __init__(self, amd, n, flip=None):
        cols, rows, vals, n = _vecc.arrow_spd(n)
        ctx = amd.HIPContext("secded", "csr", on_event=lambda ev, fatal: None)
        A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        v = dict(zip("bxrpw", (ctx.create_vector(n) for _ in range(5))))
        ctx.upload(v["b"], rhs(n, 1))
        ctx.upload(v["x"], np.zeros(n))
        self.hist = []

        def on_iteration(itr, rr):
            self.hist.append(rr)
            if flip and itr == 1:
                ctx.flip_vector(v[flip[0]], flip[1], flip[2])

        self.itr, self.rr = amd.cg_solve(ctx, A, v["b"], v["x"], v["r"], v["p"], v["w"], 1000, 1e-10,
                                         on_iteration=on_iteration, vector_ecc=True)
        self.x = ctx.download(v["x"])
        self.events = list(ctx.event_log)
        ctx.close()


def test_protected_solve_under_a_flip_in_the_hub_entry_is_the_clean_solve(amd):
    from abft_sparse_cg_amd import capi
    n = capi.load().abft_hip_event_capacity() + 64
    clean = ArrowSolve(amd, n)
    assert clean.itr >= 3 and clean.events == []  # an iteration runs on the flipped p
    hit = ArrowSolve(amd, n, ("p", 0, [30]))
    assert hit.itr == clean.itr and np.array_equal(np.array(hit.hist).view(U), np.array(clean.hist).view(U))
    assert np.array_equal(hit.x.view(U), clean.x.view(U))
    # a flip in p: spmv_vecc and calc_p_vecc report operand 0, calc_xr_vecc operand 2
    assert hit.events == [(CORRECTED, 0, 30 | op << 8) for op in (0, 2, 0)]
