"""The fixed-iteration CG loop with alpha and beta kept on the device -- abft_hip_cg_iteration_dev (SpMV + ONE
launch, cg_tail_kernel, in its three template forms), the three calls it stands for (abft_hip_spmv_dot_dev,
abft_hip_calc_xr_ratio_dev, abft_hip_calc_p_ratio_dev), ABFT_HIP_TAIL=0 and a replayed graph pair -- against a model
that shares nothing with the kernels (tests/_devloop.py: the oracle's SpMV, numpy's element-wise arithmetic, exact
sums; compared with the oracle in test_devloop_model.py).

After EVERY iteration x, r, p, w and the six scalars are downloaded:
  vectors   ieee_equal to the model (bit for bit, NaN payloads aside), given the two scalars the device left;
  p.w       the IEEE class of the exact sum of p[off + i] * w[i], and within sum_bound(terms, fused_depth(1024,
            nparts)) of it when finite -- the bound of test_gpu_special_values.py (a fused SpMV partial sums at most
            a workgroup's 1024 rows);
  r.r       likewise with dot_depth(n); on the first iteration also the bits of abft_hip_dot(r, r);
  events    each pair's second word equals what abft_hip_read_pair delivers and abft_hip_pending_events then says;
  the scalar the iteration started from is left alone (the next iteration starts from what this one left).
Every other way of running the same iteration must leave identical bits everywhere, and abft_hip_tail_stats must
name the form the case was built to reach."""
import ctypes as C
import math
import mmap

import numpy as np
import pytest

import _ieee as I
from _devloop import model_iteration
from _ieee import ieee_diff, ieee_equal, value_class
from _oracle import COO, CSR, OracleMatrix, laplace5, random_spd

pytestmark = pytest.mark.gpu

ROWS_PER_THREAD = 1024  # as in test_gpu_special_values.py: 1024 rows bound a fused SpMV partial in every layout
SENTINEL = -7.0e77      # around every view: a store outside the view shows
FMT = {"csr": CSR, "coo": COO}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------ matrices --

def tri(n, seed=7):
    """tridiagonal, symmetric, strictly diagonally dominant (SPD): diagonal in [3.5, 4.5), off-diagonals in
    (-1.5, -1.25] -- beyond 1 in magnitude, so an entry of DBL_MAX overflows in its neighbours' rows too"""
    rng = np.random.default_rng(seed)
    off = -(1.25 + 0.25 * rng.random(max(n - 1, 0)))
    diag = 3.5 + rng.random(n)
    i, j = np.arange(n), np.arange(max(n - 1, 0))
    rows = np.concatenate([i, j, j + 1])
    cols = np.concatenate([i, j + 1, j])
    vals = np.concatenate([diag, off, off])
    order = np.lexsort((cols, rows))
    return cols[order].astype(np.uint32), rows[order].astype(np.uint32), vals[order], n


def pairs2(n, seed=3):
    """two elements per row (n even): 2 x 2 SPD blocks [[d, -0.5], [-0.5, d']] on the diagonal"""
    assert n % 2 == 0
    rows = np.repeat(np.arange(n, dtype=np.int64), 2)
    cols = (rows & ~1) + np.tile(np.array([0, 1]), n)
    diag = 2.0 + np.random.default_rng(seed).random(n)
    vals = np.where(cols == rows, diag[rows], -0.5)
    return cols.astype(np.uint32), rows.astype(np.uint32), vals, n


def skew(n):
    """row 2j = +e(2j+1), row 2j+1 = -e(2j) (an odd n's last row: one stored 0.0): p . (A p) is exactly 0 for
    every p, in any order of summation when p holds small integers"""
    m = n & ~1
    rows = np.arange(n, dtype=np.int64)
    cols = np.where(rows < m, rows ^ 1, rows)
    vals = np.where(rows < m, np.where(rows & 1, -1.0, 1.0), 0.0)
    return cols.astype(np.uint32), rows.astype(np.uint32), vals, n


def start(n, seed=12):
    """the loop's state behind its first copy: p = r = b, an x with every mantissa bit in use, w full of NaN (the
    SpMV rewrites every entry: none may show)"""
    rng = np.random.default_rng(seed)
    b = rng.random(n)
    return {"x": rng.standard_normal(n), "r": b.copy(), "p": b.copy(), "w": np.full(n, I.QNAN), "rr": float(b @ b)}


# ------------------------------------------------------------------- harness --

class Dev:
    """one context: a matrix, x r p w (each its own vector, or a view one entry into a parent), the six scalars
    {rr, ev}, {rr', ev}, {p.w, ev}; window=(n_pad, off): the matrix is a shard reading a gathered vector of n_pad
    entries of which p is the window [off, off + n)"""

    def __init__(self, mat, fmt="csr", mode="none", align="aligned", window=None, layout=None, flip=None, sharers=1,
                 board=None):
        import abft_sparse_cg_amd as amd
        from abft_sparse_cg_amd import capi
        self.capi, self.events = capi, []
        self.ctx = ctx = amd.HIPContext(mode, fmt, on_event=lambda ev, fatal: self.events.extend(ev))
        self.L, self.h = ctx.L, ctx.h
        cols, rows, vals, n = mat
        self.n = n
        if window:
            self.n_pad, self.off = window
            self.A = ctx.create_matrix(cols, rows, vals, n, len(vals), n_in=self.n_pad, index_base=0)
        else:
            self.n_pad, self.off = n, 0
            self.A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout=layout)
        if flip:
            ctx.inject_at(self.A, flip[0], flip[1])
        self.parents = []

        def vec(odd):
            if not odd:
                return ctx.create_vector(n)
            parent = ctx.create_vector(n + 2)
            ctx.upload(parent, np.full(n + 2, SENTINEL))
            self.parents.append(parent)
            return ctx.view_vector(parent, 1, n)

        self.x, self.r = vec(align == "odd"), vec(align == "odd")
        self.w = vec(align in ("odd", "w_odd"))
        # r.r is summed in the order of the call's walk over its operands: by pairs when x, r, p and w are all 16-byte
        # aligned, else entry by entry (include/abft_hip.h, abft_hip_calc_xr_ratio_dev).  abft_hip_dot(r, r) chooses by r
        # alone, so where r is aligned and another operand is not it sums the same values in the other order: there
        # the identity is checked on a copy of r that is unaligned like the call.
        self.r_walk = vec(True) if align == "w_odd" or (window and window[1] & 1) else self.r
        if window:
            self.pfull = ctx.create_vector(self.n_pad)
            self.p = ctx.view_vector(self.pfull, self.off, n)
        else:
            self.pfull = self.p = vec(align == "odd")
        self.sc = ctx.create_vector(6)
        self.base = self.sc.device_ptr
        self.board = None
        if sharers != 1:
            capi.check(self.L.abft_hip_set_sharers(self.h, sharers))
        if board == "host":  # a board of one rank, set up as tools/shard_budget.py does
            self.board = mmap.mmap(-1, self.L.abft_hip_peer_board_bytes())
            capi.check(self.L.abft_hip_peer_board_attach(self.h, C.addressof(C.c_char.from_buffer(self.board)),
                                                         len(self.board), 0, 1, 5.0))
        elif board == "device":
            bp = C.c_void_p()
            capi.check(self.L.abft_hip_peer_board_device_alloc(self.h, C.byref(bp)))
            self.board = bp
            capi.check(self.L.abft_hip_peer_board_attach_device(self.h, (C.c_void_p * 1)(bp.value), 0, 1, 5.0))
        if board:
            capi.check(self.L.abft_hip_peer_board_fuse(self.h, 1))
        self.board_kind = board

    def matrix(self, mat):
        cols, rows, vals, n = mat
        assert n == self.n and self.n_pad == n
        return self.ctx.create_matrix(cols, rows, vals, n, len(vals))

    def nparts(self):
        """partials of the fused product.  The streaming CSR layout has one per row block, which
        abft_hip_matrix_compact_stats counts; the other layouts launch a grid of at most a few thousand workgroups,
        and up to 8192 partials every count gives the same depth (finalize_depth: one pass of the 1024-thread fold)"""
        if self.A.fmt == 0 and self.ctx.matrix_info(self.A)[0] == "stream":
            c, t, m = C.c_uint32(), C.c_uint32(), C.c_uint32()
            self.capi.check(self.L.abft_hip_matrix_compact_stats(self.A.h, C.byref(c), C.byref(t), C.byref(m)))
            return t.value
        return 8192

    def load(self, s):
        ctx = self.ctx
        for v, a in ((self.x, s["x"]), (self.r, s["r"]), (self.w, s["w"])):
            ctx.upload(v, a)
        if "pfull" in s:
            ctx.upload(self.pfull, s["pfull"])
        else:
            ctx.upload(self.p, s["p"])
        ctx.upload(self.sc, np.array([s["rr"], 0.0, 0.0, 0.0, 0.0, 0.0]))

    def snapshot(self):
        d = self.ctx.download
        return {"x": d(self.x), "r": d(self.r), "pfull": d(self.pfull), "w": d(self.w), "sc": d(self.sc)}

    def launch(self, kind, parity, A=None):
        L, h, c = self.L, self.h, self.capi
        A = A or self.A
        cur, nxt, pw = self.base + 16 * parity, self.base + 16 * (1 - parity), self.base + 32
        if kind == "three":
            c.check(L.abft_hip_spmv_dot_dev(h, A.h, self.pfull.h, self.w.h, self.off, pw))
            c.check(L.abft_hip_calc_xr_ratio_dev(h, self.x.h, self.r.h, self.p.h, self.w.h, cur, pw, nxt))
            c.check(L.abft_hip_calc_p_ratio_dev(h, self.p.h, self.r.h, nxt, cur))
        else:
            c.check(L.abft_hip_cg_iteration_dev(h, A.h, self.pfull.h, self.off, c.PART_ALL, self.x.h, self.r.h, self.p.h,
                                                self.w.h, cur, pw, nxt))

    def capture(self, parity):
        self.capi.check(self.L.abft_hip_graph_begin(self.h))
        self.launch("one", parity)
        g = C.c_void_p()
        self.capi.check(self.L.abft_hip_graph_end(self.h, C.byref(g)))
        return g

    def read_pair(self, at):
        """-> (value, events word, abft_hip_pending_events right behind it) of the pair at scalar slot `at`"""
        v, e = C.c_double(), C.c_double()
        self.capi.check(self.L.abft_hip_read_pair(self.h, self.base + 8 * at, C.byref(v), C.byref(e)))
        return v.value, e.value, self.L.abft_hip_pending_events(self.h)

    def close(self):
        """tear everything down first, then say whether anything was stored outside a view"""
        edges = []
        try:
            for parent in self.parents:
                a = self.ctx.download(parent)
                edges.append((a[0], a[-1]))
        finally:
            if self.board_kind:
                self.L.abft_hip_peer_board_fuse(self.h, 0)
                self.L.abft_hip_peer_board_detach(self.h)
                if self.board_kind == "device":
                    self.L.abft_hip_peer_board_device_free(self.h, self.board)
            self.L.abft_hip_set_sharers(self.h, 1)
            self.ctx.close()
        for e in edges:
            assert e == (SENTINEL, SENTINEL), e


def check_scalar(what, d, terms, depth, exact=False):
    want = I.exact_sum(terms)
    print("   %s: device %r exact %r" % (what, d, want), end="")
    assert value_class(d) == value_class(want), (what, d, want)
    if math.isfinite(want):
        bound = I.sum_bound(terms, depth)
        print(" |diff| %.3e bound %.3e" % (abs(d - want), bound), end="")
        assert abs(d - want) <= bound, (what, d, want, bound)
        if exact:  # exactly representable partial sums: the exact value, and an exact zero as +0.0
            assert ieee_equal([d], [want]), (what, d, want)
    print()


def check_model(o, dev, pre, post, parity, nparts, exact=False):
    """one iteration, from the state `pre` to the state `post`, against the model"""
    n, off = dev.n, dev.off
    cur, nxt = 2 * parity, 2 * (1 - parity)
    rr, pw, rr_new = pre["sc"][cur], post["sc"][4], post["sc"][nxt]
    m = model_iteration(o, pre["x"], pre["r"], pre["pfull"], off, pre["w"], rr, pw, rr_new)
    for name, got, want in (("w", post["w"], m.w), ("r", post["r"], m.r), ("x", post["x"], m.x),
                            ("p", post["pfull"][off:off + n], m.p)):
        assert ieee_equal(got, want), (name, ieee_diff(got, want))
    rest = np.ones(dev.n_pad, dtype=bool)
    rest[off:off + n] = False
    assert np.array_equal(bits(post["pfull"][rest]), bits(pre["pfull"][rest]))  # the other ranks' slots and the padding
    assert np.array_equal(bits(post["sc"][cur:cur + 2]), bits(pre["sc"][cur:cur + 2]))  # what it started from: left alone
    check_scalar("p.w", pw, m.pw_terms, I.fused_depth(ROWS_PER_THREAD, nparts), exact)
    check_scalar("r.r", rr_new, m.rr_terms, I.dot_depth(n), exact)
    return m


def run(dev, kind, iters, o=None, nparts=None, path=None, grid=None, flip=False, dot_check=True, exact=False, A=None,
        first_parity=0):
    """`iters` iterations of one kind -- "one": abft_hip_cg_iteration_dev; "three": the three _dev calls; "graph": the
    first two as calls, the rest replayed from a pair of captured graphs -- with the scalar slots swapping parity.
    With an oracle matrix `o` every iteration is held against the model.  path: what abft_hip_tail_stats must say
    after a call of abft_hip_cg_iteration_dev (a tuple: any of these); grid: a predicate on (grid, want).
    -> the downloaded states after every iteration"""
    posts, graphs = [], {}
    for k in range(iters):
        parity = (first_parity + k) & 1
        pre = dev.snapshot()  # (a download also drains the events queued so far)
        n_before = len(dev.events)
        called = True
        if kind == "graph" and k >= 2:
            called = parity not in graphs
            if called:
                graphs[parity] = dev.capture(parity)
            dev.capi.check(dev.L.abft_hip_graph_launch(graphs[parity]))
        else:
            dev.launch(kind, parity, A)
        if kind != "three" and called:
            st = dev.ctx.tail_stats()
            if k == 0:
                print("   %s: path %d grid %d want %d" % (kind, st[0], st[1], st[2]))
            if path is not None:
                assert st[0] in (path if isinstance(path, tuple) else (path,)), (st, path)
            assert (st[1] == 0 and st[2] == 0) if st[0] == 0 else 1 <= st[1] <= st[2], st
            if grid is not None and st[0] != 0:
                assert grid(st[1], st[2]), st
        # the two pairs as the host reads them, before anything drains: value, events word, pending count
        v_pw, e_pw, pend_pw = dev.read_pair(4)
        v_rr, e_rr, pend_rr = dev.read_pair(2 * (1 - parity))
        post = dev.snapshot()
        new_events = len(dev.events) - n_before
        sc = post["sc"]
        assert ieee_equal([v_pw, v_rr], [sc[4], sc[2 * (1 - parity)]])
        assert e_pw == sc[5] == pend_pw and e_rr == sc[2 * (1 - parity) + 1] == pend_rr, (e_pw, sc, pend_pw, e_rr, pend_rr)
        if flip and k == 0:  # the flipped bit was met by this iteration's SpMV, and repaired
            assert e_pw >= 1 and e_pw == e_rr == new_events, (e_pw, e_rr, new_events)
        else:                # nothing pending: drained, or never queued
            assert e_pw == 0 and e_rr == 0 and new_events == 0, (k, e_pw, e_rr, new_events)
        assert dev.L.abft_hip_pending_events(dev.h) == 0
        if o is not None:
            check_model(o, dev, pre, post, parity, nparts, exact)
        if dot_check and k == 0:  # r.r is the bits abft_hip_dot(r, r) gives on the r it left
            if dev.r_walk is not dev.r:
                dev.ctx.copy_vector(dev.r_walk, dev.r)
            assert ieee_equal([dev.ctx.dot(dev.r_walk, dev.r_walk)], [sc[2 * (1 - parity)]])
        posts.append(post)
    for g in graphs.values():
        dev.L.abft_hip_graph_destroy(g)
    return posts


def same_bits(a, b, plus_zero=False):
    """two runs' states, iteration by iteration; plus_zero: a sum of -0.0 may have become +0.0 (a board adds 0.0 + v)"""
    assert len(a) == len(b)
    for k, (pa, pb) in enumerate(zip(a, b)):
        for name in ("x", "r", "pfull", "w"):
            assert np.array_equal(bits(pa[name]), bits(pb[name])), (k, name, ieee_diff(pa[name], pb[name]))
        sa, sb = (pa["sc"] + 0.0, pb["sc"] + 0.0) if plus_zero else (pa["sc"], pb["sc"])
        assert np.array_equal(bits(sa), bits(sb)), (k, pa["sc"], pb["sc"])


def full_case(mat, state, monkeypatch, path, kinds=("three", "tail0", "graph"), iters=5, fmt="csr", mode="none", o=None,
              flip=None, grid=None, **kw):
    """the case as abft_hip_cg_iteration_dev against the model, then every other way of running it: same bits"""
    own = o is None
    if own:
        o = OracleMatrix(FMT[fmt], mode, *mat[:3], mat[3], n_in=kw["window"][0] if kw.get("window") else None)
        if flip:
            o.inject(*flip)
    dev = Dev(mat, fmt, mode, flip=flip, **kw)
    try:
        dev.load(state)
        ref = run(dev, "one", iters, o, dev.nparts(), path=path, grid=grid, flip=bool(flip))
    finally:
        dev.close()
    for kind in kinds:
        if kind == "tail0":
            monkeypatch.setenv("ABFT_HIP_TAIL", "0")
        dev = Dev(mat, fmt, mode, flip=flip, **kw)
        monkeypatch.delenv("ABFT_HIP_TAIL", raising=False)
        try:
            dev.load(state)
            got = run(dev, "one" if kind == "tail0" else kind, iters, path=0 if kind == "tail0" else path, grid=grid,
                      flip=bool(flip))
        finally:
            dev.close()
        same_bits(ref, got)
    if own:
        o.close()
    return ref


# ------------------------------------------------------- a. lengths and tails --

# an odd last element (1, 255, 257, ...), one virtual block of 2048 entries partly filled (2047, 2049, 4097, 6145),
# quarters of a 1024-thread workgroup with no virtual block of their own (every n here below 8192 at Q = 4)
LENGTHS = [1, 2, 255, 256, 257, 511, 513, 2047, 2048, 2049, 4097, 6145]


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_and_tails(n, monkeypatch):
    mat, state = tri(n), start(n)
    ref = full_case(mat, state, monkeypatch, path=3)
    o = OracleMatrix(CSR, "none", *mat)
    for q in ("1", "2"):
        monkeypatch.setenv("ABFT_HIP_TAIL_Q", q)
        dev = Dev(mat)
        try:
            dev.load(state)
            got = run(dev, "one", 5, o, dev.nparts(), path=3, grid=lambda g, w: g == w == -(-I.reduce_blocks(n) // int(q)))
        finally:
            dev.close()
        same_bits(ref, got)


# ------------------------------------------------------ b. unaligned operands --

@pytest.mark.parametrize("n", [257, 2049, 40961])
def test_operands_at_an_odd_offset(n, monkeypatch):
    """x, r, p and w each a view one entry into its parent: cg_tail_kernel<1, false>, the form a shard that starts
    at an odd row takes; the three _ratio_dev calls on the same views; then w alone unaligned"""
    mat, state = tri(n), start(n)
    odd = full_case(mat, state, monkeypatch, path=1, align="odd")
    mix = full_case(mat, state, monkeypatch, path=1, align="w_odd", kinds=("three",))
    same_bits(odd, mix)  # (not the aligned run's bits: that one sums r.r by pairs, another order)


# ------------------------------------------------ c. capped grid, several rounds --

N_CAPPED = 100003  # 49 virtual blocks: 13 / 25 / 49 workgroups of 4 / 2 / 1


@pytest.mark.parametrize("q", ["4", "2", "1"])
def test_capped_grid_walks_the_vector_in_rounds(q, monkeypatch):
    """32 sharers leave each process 1/64 of the resident workgroups (any cap from 256 to 2048 gives 4 to 32): fewer
    than the vector asks for, so the looped form runs with several workgroups and several rounds of
    base += gridDim.x * Q.  Seen on an MI355X: grid 4 of 13 (Q = 4), 12 of 25 (Q = 2), 28 of 49 (Q = 1), for the aligned
    and for the unaligned form alike."""
    n = N_CAPPED
    mat, state = tri(n), start(n)
    monkeypatch.setenv("ABFT_HIP_TAIL_Q", q)
    want = -(-I.reduce_blocks(n) // int(q))
    assert I.reduce_blocks(n) == 49
    capped = lambda g, w: w == want and 2 <= g < w  # noqa: E731
    ref = full_case(mat, state, monkeypatch, path=2, kinds=("three", "graph"), sharers=32, grid=capped)
    full_case(mat, state, monkeypatch, path=1, kinds=("three", "graph"), sharers=32, grid=capped, align="odd")
    # 4096 sharers: the share rounds to no workgroup at all -- the three kernels, the same bits
    none = full_case(mat, state, monkeypatch, path=0, kinds=(), sharers=4096)
    same_bits(ref, none)
    # one process per device again: the register-resident form, the same bits
    alone = full_case(mat, state, monkeypatch, path=3, kinds=(), grid=lambda g, w: g == w == want)
    same_bits(ref, alone)


# ----------------------------------------------------------- d. the 2^22 cut --

@pytest.mark.parametrize("n,merged", [(1 << 22, True), ((1 << 22) + 2, False)])
def test_the_length_cut_of_the_one_launch(n, merged, monkeypatch):
    """2^22 entries still take the one launch (whichever form the resident cap leaves: seen on an MI355X, the looped
    one with 256 workgroups of the 512 the length asks for), two entries more take the three kernels; one iteration"""
    mat, state = pairs2(n), start(n)
    o = OracleMatrix(CSR, "none", *mat)
    dev = Dev(mat)
    try:
        dev.load(state)
        ref = run(dev, "one", 1, o, dev.nparts(), path=(2, 3) if merged else 0)
    finally:
        dev.close()
    o.close()
    dev = Dev(mat)
    try:
        dev.load(state)
        got = run(dev, "three", 1)
    finally:
        dev.close()
    same_bits(ref, got)


# ---------------------------------------------------------- e. many partials --

def test_chunk_fold_loops_when_the_grid_is_capped_below_it(monkeypatch):
    """More than 8192 SpMV partials: the product is folded by chunks (fold_nb of them) and a grid capped below
    fold_nb virtual blocks walks the chunks in rounds.  The matrix is test_gpu_special_values.py's: rows of TILE / 2 + 1
    elements fill one row block each (two do not fit a tile), so 8200 rows give 8200 partials -- read back from
    abft_hip_matrix_compact_stats and asserted.  The resident cap is not known here: the sharers are halved from
    1024 until the share is at least one workgroup, which then is exactly one (Q = 1: 256 threads, five chunks, five
    rounds on that one workgroup); the calls before that take the three kernels and are held against the model all
    the same.  Seen on an MI355X: grid 1 of the 5 the length asks for."""
    tile = I.csr_tile()
    length, n = tile // 2 + 1, 8200
    rows = np.repeat(np.arange(n, dtype=np.uint32), length)
    cols = ((rows.astype(np.int64) + np.tile(np.arange(length) * 13, n)) % n).reshape(n, length)
    cols.sort(axis=1)
    cols = cols.reshape(-1).astype(np.uint32)
    vals = np.random.default_rng(9).standard_normal(len(cols))
    mat = (cols, rows, vals, n)
    o = OracleMatrix(CSR, "none", *mat)
    monkeypatch.setenv("ABFT_HIP_TAIL_Q", "1")
    dev = Dev(mat)
    try:
        nparts = dev.nparts()
        assert nparts > 8192, nparts
        fold_nb = min(64, -(-nparts // 2048))
        dev.load(start(n))
        plain = run(dev, "one", 1, o, nparts, path=3)
        dev.load(start(n))
        s, reached = 1024, None
        while s >= 1 and reached is None:
            dev.capi.check(dev.L.abft_hip_set_sharers(dev.h, s))
            dev.load(start(n))
            got = run(dev, "one", 1, o, nparts)
            same_bits(plain, got)
            st = dev.ctx.tail_stats()
            if st[0] != 0:
                reached = st
            s //= 2
        assert reached is not None and reached[0] == 2 and 1 <= reached[1] < fold_nb, (reached, fold_nb)
        assert reached[3][3] == 1  # (the uncapped call before the search)
    finally:
        dev.close()


# ------------------------------------------------- f. layouts, modes and events --

LAYOUTS = [
    ("csr", "sec8", "sweep", (1000, [37])),
    ("coo", "sec7", "panels", (1000, [70])),
    ("csr", "secded", "stream", (1000, [37])),
]


@pytest.mark.parametrize("fmt,mode,layout,flip", LAYOUTS)
def test_layouts_with_a_repaired_bit(fmt, mode, layout, flip, monkeypatch):
    """one repairable flipped bit: both pairs carry the count of queued events until they are drained (by the
    download behind the iteration) and 0 from then on; vectors and scalars as the oracle's after the same flip"""
    mat = random_spd(30011, 9, seed=5)
    kw = {}
    if layout == "stream":
        kw["layout"] = "stream"
    else:
        monkeypatch.setenv("ABFT_HIP_LAYOUT", layout)
    dev = Dev(mat, fmt, mode, **kw)
    assert dev.ctx.matrix_info(dev.A)[0] == layout
    dev.close()
    # (COO: the fix-up of moved products is part of every COO fold and rewrites entries of w: the looped form)
    full_case(mat, start(mat[3]), monkeypatch, path=2 if fmt == "coo" else 3, fmt=fmt, mode=mode, flip=flip, **kw)


def test_coo_fixup_inside_the_fold(monkeypatch):
    """COO, mode none, a silently corrupted column (test_gpu_tail.py's): the moved product is put where the reference
    puts it inside the fold -- not the register-resident form, which loads w before the fix-up rewrites it"""
    mat = laplace5(61, 47)
    o = OracleMatrix(COO, "none", *mat)
    o.inject(777, [3])
    dev = Dev(mat, "coo", "none", flip=(777, [3]))
    try:
        dev.load(start(mat[3]))
        ref = run(dev, "one", 5, o, dev.nparts(), path=2)
    finally:
        dev.close()
    for kind in ("three", "graph"):
        dev = Dev(mat, "coo", "none", flip=(777, [3]))
        try:
            dev.load(start(mat[3]))
            same_bits(ref, run(dev, kind, 5, path=2))
        finally:
            dev.close()


# ------------------------------------------------- g. a shard, vec_offset != 0 --

@pytest.mark.parametrize("parity", ["even", "odd"])
def test_shard_reads_its_window_of_the_gathered_vector(parity, monkeypatch):
    """rank 1 of 3 of random:8192,6,1 (the generator takes powers of two only, so not 6000 rows), built as
    tools/shard_budget.py builds it: columns re-based to the slot-padded gathered vector, p the window
    [slot, slot + rows) of it.  p.w is the product over the window only; the other ranks' slots and the padding hold
    values a thousand times larger, which the SpMV reads and nothing else may."""
    from abft_sparse_cg_amd import generators
    spec, G, k = "random:8192,6,1", 3, 1
    bounds = generators.partition(spec, G)
    slot = max(bounds[g + 1] - bounds[g] for g in range(G))
    if (slot & 1) != (parity == "odd"):
        slot += 1
    cols, rows, vals, _ = generators.generate(spec, bounds[k], bounds[k + 1])
    b = np.asarray(bounds)
    owner = np.searchsorted(b, cols, side="right") - 1
    pin = (owner * slot + (cols - b[owner])).astype(np.uint32)
    n_loc, n_pad, off = int(bounds[k + 1] - bounds[k]), slot * G, k * slot
    assert off % 2 == (parity == "odd") and (owner != k).any()
    mat = (pin, (rows - bounds[k]).astype(np.uint32), vals, n_loc)
    state = start(n_loc)
    rng = np.random.default_rng(4)
    state["pfull"] = 1e3 * (1.0 + rng.random(n_pad))
    state["pfull"][off:off + n_loc] = state["p"]
    full_case(mat, state, monkeypatch, path=1 if parity == "odd" else 3, window=(n_pad, off))


# ------------------------------------------------------ h. a board of one rank --

@pytest.mark.parametrize("board", ["host", "device"])
@pytest.mark.parametrize("sharers", [1, 32])
def test_board_all_reduces_inside_the_tail(board, sharers, monkeypatch):
    """abft_hip_peer_board_fuse on a board of one rank: both all-reduces run inside the one launch.  The
    host-memory board has workgroup 0 fold and publish p.w behind a flag and the last workgroup to arrive fold r.r;
    the device-memory board has every workgroup fold.  One rank's sum is 0.0 + v: the unfused run's bits, a -0.0 aside."""
    n = N_CAPPED
    mat, state = tri(n), start(n)
    path = 3 if sharers == 1 else 2
    grid = (lambda g, w: g == w) if sharers == 1 else (lambda g, w: 2 <= g < w)
    plain = full_case(mat, state, monkeypatch, path=path, kinds=(), sharers=sharers, grid=grid)
    o = OracleMatrix(CSR, "none", *mat)
    for kind in ("one", "three", "graph"):
        dev = Dev(mat, sharers=sharers, board=board)
        try:
            dev.load(state)
            got = run(dev, kind, 5, o, dev.nparts(), path=path, grid=grid)
            assert dev.L.abft_hip_peer_board_failed(dev.h) == 0
        finally:
            dev.close()
        same_bits(plain, got, plus_zero=True)


# ---------------------------------------------------- i. scalars in edge states --

def edge_states(n):
    """name -> (state, which matrix, exact): states in which the loop has nothing finite to say, each reached by
    arithmetic alone"""
    s = {}
    z = start(n)
    z.update(r=np.zeros(n), p=np.zeros(n), rr=0.0)
    s["converged"] = (z, "tri", False)                     # p.w = 0, alpha = 0 / 0
    a = start(n)
    a["rr"] = 0.0
    s["rr_zero"] = (a, "tri", False)                       # alpha = 0, beta = r.r / 0
    b = start(n)
    b["p"] = 1e160 * (1.0 + 0.01 * b["p"])                 # (nearly constant: every entry of A p is positive)
    s["pw_overflows"] = (b, "tri", False)                  # every product overflows: p.w = +Inf, alpha = 0
    c = start(n)
    ints = I.exact_pair(n, 5, "int")[0]
    c["p"] = np.where(ints == 0.0, 3.0, ints)
    s["pw_cancels"] = (c, "skew", True)                    # p.w = +0.0 exactly with p != 0: alpha = +Inf
    d = start(n)
    d["rr"] = float(I.TINY * 1000)
    s["rr_subnormal"] = (d, "tri", False)
    e = start(n)
    k = n // 2
    e["p"][k - 1], e["p"][k], e["p"][k + 1] = I.DBL_MAX, 1.0, -I.DBL_MAX
    s["nan_in_w"] = (e, "tri", False)                      # w[k] = -Inf + finite + Inf: the one NaN of w
    return s


# what p.w must be after the first iteration of each state (from the state, not from a run)
EXPECT_PW = {"converged": lambda v: v == 0.0, "rr_zero": math.isfinite, "pw_overflows": lambda v: v == I.INF,
             "pw_cancels": lambda v: v == 0.0 and math.copysign(1.0, v) == 1.0, "rr_subnormal": math.isfinite,
             "nan_in_w": math.isnan}


@pytest.mark.parametrize("n,align,sharers,path", [(2049, "aligned", 1, 3), (2049, "odd", 1, 1), (N_CAPPED, "aligned", 32, 2)])
def test_scalars_in_edge_states(n, align, sharers, path, monkeypatch):
    """every state on ONE context, two iterations each (the second starts from the scalars the first left), then a
    clean case on the same context: finite, and the model's -- so no wait inside the launch was given up on the
    way (that would leave every later launch of the context answering NaN)"""
    mats = {"tri": tri(n), "skew": skew(n)}
    oracles = {k: OracleMatrix(CSR, "none", *m) for k, m in mats.items()}
    dev = Dev(mats["tri"], align=align, sharers=sharers)
    try:
        A = {"tri": dev.A, "skew": dev.matrix(mats["skew"])}
        nparts = dev.nparts()
        grid = (lambda g, w: 2 <= g < w) if sharers > 1 else None
        with np.errstate(all="ignore"):
            expect = {"nan_in_w": lambda w: np.isnan(w).sum() == 1}
            for name, (state, which, exact) in edge_states(n).items():
                print(" state %s" % name)
                for kind in ("one", "three"):
                    dev.load(state)
                    posts = run(dev, kind, 2, oracles[which], nparts, path=path, grid=grid, dot_check=False, exact=exact,
                                A=A[which])
                    if kind == "one":
                        ref = posts
                        if name in expect:
                            assert expect[name](posts[0]["w"])
                        assert EXPECT_PW[name](float(posts[0]["sc"][4])), (name, posts[0]["sc"])
                    else:
                        # identical bits wherever the value is no NaN, NaNs in the same places (ieee_equal).  The NaNs' own
                        # bits do differ between the forms: seen in the converged state (alpha = 0 / 0), second iteration,
                        # in x -- IEEE 754 leaves the sign and payload of a NaN that an operation returns open
                        for k, (pa, pb) in enumerate(zip(ref, posts)):
                            for key in ("x", "r", "pfull", "w", "sc"):
                                assert ieee_equal(pa[key], pb[key]), (name, k, key, ieee_diff(pa[key], pb[key]))
        dev.load(start(n))
        clean = run(dev, "one", 2, oracles["tri"], nparts, path=path, grid=grid)
        for post in clean:
            assert all(np.isfinite(post[key]).all() for key in ("x", "r", "pfull", "w", "sc"))
    finally:
        dev.close()


def test_a_refused_call_has_launched_nothing():
    """abft_hip_cg_iteration_dev with an r of 63 entries for a matrix of 64 rows: ABFT_ERR_INVALID, decided on the
    host before the SpMV -- which would overwrite w and hold the fold of p.w back -- so every word of w, x, r, p and of
    the pair dev_pw keeps the bits it had"""
    import abft_sparse_cg_amd as amd
    from abft_sparse_cg_amd import capi
    n = 64
    cols, rows, vals, _ = tri(n)
    ctx = amd.HIPContext("none", "csr")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        vecs = {"x": ctx.create_vector(n), "r": ctx.create_vector(n - 1), "p": ctx.create_vector(n),
                "w": ctx.create_vector(n), "sc": ctx.create_vector(6)}
        for v in vecs.values():
            ctx.upload(v, np.full(v.N, SENTINEL))
        base = vecs["sc"].device_ptr
        rc = ctx.L.abft_hip_cg_iteration_dev(ctx.h, A.h, vecs["p"].h, 0, capi.PART_ALL, vecs["x"].h, vecs["r"].h,
                                             vecs["p"].h, vecs["w"].h, base, base + 32, base + 16)
        assert rc == -1, rc  # ABFT_ERR_INVALID
        assert b"lengths differ" in ctx.L.abft_hip_last_error()
        ctx.synchronize()
        want = bits(np.array([SENTINEL]))[0]
        for name, v in vecs.items():
            got = bits(ctx.download(v))
            assert got.shape == (v.N,) and (got == want).all(), (name, got)
    finally:
        ctx.close()
