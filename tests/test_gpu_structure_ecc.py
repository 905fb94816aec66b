"""The protected CSR row structure on the GPU: a matrix created with structure_ecc=True stores
row extent words and row-block descriptors as SECDED codewords, and every SpMV checks each word it reads.

Every comparison is bit for bit.  The reference of every output is a CLEAN TWIN: the same call on the same matrix
created with layout="stream" alone, in a second context.  The stored words are held against host models
(tests/_structecc.py: the vector code's model on the packed integer, the oracle's COO secded element), the planted
flips against the events drained.  tests/test_struct_ecc_host.py proves without a GPU that the matrices reach every
branch: `rand` reads every row word, `wide5` has uniform blocks (whose row words no SpMV reads) and others, `diag23`
blocks of 1024 rows (four trips of the row loop), `arrow` a long row, `holes` empty rows.  (`lap40`, which the sweep
runs as well, has no uniform block: its rows change length every 40 rows.)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _layout_cases as LC
import _structecc as S
from _oracle import rhs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO = LC.geometry(os.path.join(ROOT, "abft_sparse_cg_amd", "csrc"))
NTHREADS, TILE = GEO[0], GEO[1]
MODES = ["none", "constraints", "sed", "sec7", "sec8", "secded"]
SWEPT = ["rand", "diag23", "arrow", "holes", "lap40", "wide5"]
U = np.uint64
EV_ELEMENT, EV_VEC, EV_FIXED, EV_DOUBLE = 2, 10, 12, 13
SENTINEL = -7.25


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(U)


def same(a, b, tag=None):
    a, b = u64(a), u64(b)
    assert a.shape == b.shape and np.array_equal(a, b), (tag, int(np.count_nonzero(a != b)) if a.shape == b.shape else -1)


class Box:
    """one context and one matrix in the streaming layout, its structure protected or not; events collected"""

    def __init__(self, amd, mode, name, protect, collect=True):
        cols, rows, vals, n = S.matrix(name)
        self.events, self.fatal = [], False
        self.ctx = amd.HIPContext(mode, "csr", on_event=self._on if collect else None)
        self.mode, self.n, self.nnz = mode, n, len(vals)
        self.ptr = S.rowptr_of(rows, n)
        self.A = self.ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream", structure_ecc=protect)
        self.x = rhs(n, 7) - 0.5
        self.vx, self.vy = self.vec(self.x), self.vec(np.full(n, SENTINEL))

    def _on(self, ev, fatal):
        self.events += ev
        self.fatal |= fatal

    def take(self):
        self.ctx._drain()  # (synchronises the stream)
        ev, f = self.events, self.fatal
        self.events, self.fatal = [], False
        return sorted(ev), f

    def vec(self, array):
        v = self.ctx.create_vector(len(array))
        self.ctx.upload(v, array)
        return v

    def spmv(self, sentinel=False):
        if sentinel:
            self.ctx.upload(self.vy, np.full(self.n, SENTINEL))
        self.ctx.spmv(self.A, self.vx, self.vy)
        return self.ctx.download(self.vy)

    def close(self):
        self.ctx.close()


class Pair:
    """the protected box, its clean twin, the clean stored words and the plain descriptors"""

    def __init__(self, amd, mode, name, collect=True):
        self.dam, self.twin = Box(amd, mode, name, True, collect), Box(amd, mode, name, False)
        self.mode, self.n = mode, self.dam.n
        self.want = self.twin.spmv()
        assert self.twin.take() == ([], False)
        self.ext, self.blk = self.dam.ctx.read_structure(self.dam.A)
        self.desc = self.blk.astype(np.int64)
        self.desc[:, 0] &= 0x00FFFFFF
        self.row0, self.row1, self.flag = self.desc[:, 0], self.desc[:, 1] & 0x7FFFFFFF, self.desc[:, 1] >> 31

    def rows_read(self):
        """the rows whose word one SpMV reads: all but those of uniform blocks (constraints mode has none)"""
        read = np.ones(self.n, bool)
        if self.mode != "constraints":
            for t in np.flatnonzero(self.flag):
                read[self.row0[t]:self.row1[t]] = False
        return read

    def close(self):
        self.dam.close()
        self.twin.close()


@pytest.fixture
def pair(amd, request):
    made = []

    def make(mode, name, collect=True):
        made.append(Pair(amd, mode, name, collect))
        return made[-1]
    yield make
    for p in made:
        p.close()


# ---- 1. clean parity ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_clean_parity(pair, mode, name):
    p = pair(mode, name)
    d, t = p.dam, p.twin
    assert d.ctx.structure_protected(d.A) and not t.ctx.structure_protected(t.A)
    assert d.ctx.matrix_info(d.A)[0] == "stream"
    # the stored form: stripped row words are the rows' pointers, every word re-encodes to itself under the host models
    assert np.array_equal(S.strip_rows(p.ext), d.ptr) and np.array_equal(d.ctx.rowptr(d.A).astype(np.int64), d.ptr)
    assert np.array_equal(p.ext, S.row_words(d.ptr)) and not (p.ext >> U(63)).any()
    assert np.array_equal(p.blk, S.blk_words(p.desc))
    # descriptors tile [0, N) with the pointers as element bounds; the flag only where a block's rows have one length
    assert p.row0[0] == 0 and p.row1[-1] == p.n and np.array_equal(p.row0[1:], p.row1[:-1])
    assert np.array_equal(p.desc[:, 2], d.ptr[p.row0]) and np.array_equal(p.desc[:, 3], d.ptr[p.row1])
    for k in np.flatnonzero(p.flag):
        assert len(set(np.diff(d.ptr[p.row0[k]:p.row1[k] + 1]).tolist())) == 1
    # y, and the product through spmv + dot and through spmv_dot_dev
    same(d.spmv(sentinel=True), p.want, "y")
    assert d.ctx.dot(d.vx, d.vy) == t.ctx.dot(t.vx, t.vy)
    pw = []
    for b in (d, t):
        scal = b.vec(np.zeros(4))
        from abft_sparse_cg_amd.capi import check
        check(b.ctx.L.abft_hip_spmv_dot_dev(b.ctx.h, b.A.h, b.vx.h, b.vy.h, 0, scal.device_ptr))
        pw.append(b.ctx.download(scal)[:2])
        same(b.ctx.download(b.vy), p.want, "y of spmv_dot_dev")
    same(pw[0], pw[1], "p.w on the device")
    assert pw[0][1] == 0.0
    # protected vectors
    out = []
    for b in (d, t):
        b.ctx.encode_vector(b.vx)
        b.ctx.spmv_vecc(b.A, b.vx, b.vy)
        out.append(b.ctx.download(b.vy))
    same(out[0], out[1], "spmv_vecc")
    assert d.take() == ([], False) and t.take() == ([], False)
    ext, blk = d.ctx.read_structure(d.A)
    assert np.array_equal(ext, p.ext) and np.array_equal(blk, p.blk)
    assert d.ctx.scrub_structure(d.A) == (0, 0)


# ---- 2. every slot, every bit ---------------------------------------------------------------------------------------

def flipped_rows(ext, s):
    k = np.arange(len(ext), dtype=U)
    return ext ^ (U(1) << ((k + U(s)) % U(64)))


def flipped_blocks(blk, s):
    out = blk.copy()
    for t in range(len(blk)):
        b = (t + s) % 128
        out[t, b >> 5] ^= np.uint32(1 << (b & 31))
    return out


def check_row_launch(p, s, plant):
    d = p.dam
    read = p.rows_read()
    flipped = flipped_rows(p.ext, s)
    plant(flipped)
    same(d.spmv(), p.want, ("rows", s))
    want = sorted((EV_FIXED, int(k), int((k + s) % 64)) for k in np.flatnonzero(read))
    assert d.take() == (want, False), ("rows", s)
    now = d.ctx.read_structure(d.A)[0]
    assert np.array_equal(now[read], p.ext[read]) and np.array_equal(now[~read], flipped[~read]), ("rows", s)
    # the scrub meets exactly the words no SpMV read
    rest = sorted((EV_FIXED, int(k), int((k + s) % 64)) for k in np.flatnonzero(~read))
    assert d.ctx.scrub_structure(d.A) == (len(rest), 0) and d.take() == (rest, False), ("rows", s)
    assert d.ctx.scrub_structure(d.A) == (0, 0) and d.take() == ([], False)
    assert np.array_equal(d.ctx.read_structure(d.A)[0], p.ext)


def check_block_launch(p, s, plant):
    d = p.dam
    plant(flipped_blocks(p.blk, s))
    same(d.spmv(), p.want, ("blocks", s))
    want = sorted((EV_FIXED, t, ((t + s) % 128) | (S.BLOCK << 8)) for t in range(len(p.blk)))
    assert d.take() == (want, False), ("blocks", s)
    assert np.array_equal(d.ctx.read_structure(d.A)[1], p.blk), ("blocks", s)
    assert d.ctx.scrub_structure(d.A) == (0, 0) and d.take() == ([], False)


@pytest.mark.parametrize("name", SWEPT)
@pytest.mark.parametrize("mode", ["none", "secded"])
def test_every_word_every_bit(pair, mode, name):
    p = pair(mode, name)
    d = p.dam
    for s in range(64):
        check_row_launch(p, s, lambda words: d.ctx.write_structure(d.A, rowext=words))
    for s in range(128):
        check_block_launch(p, s, lambda words: d.ctx.write_structure(d.A, blk=words))
    same(d.spmv(), p.want)
    assert d.take() == ([], False)


@pytest.mark.parametrize("name", SWEPT)
@pytest.mark.parametrize("mode", ["constraints", "sed", "sec7", "sec8"])
def test_every_word_one_launch(pair, mode, name):
    """s = 5 in the other four modes, planted word by word through flip_structure"""
    p = pair(mode, name)
    d = p.dam

    def rows(_):
        for k in range(p.n):
            d.ctx.flip_structure(d.A, "row", k, [(k + 5) % 64])

    def blocks(_):
        for t in range(len(p.blk)):
            d.ctx.flip_structure(d.A, S.BLOCK, t, [(t + 5) % 128])
    check_row_launch(p, 5, rows)
    check_block_launch(p, 5, blocks)
    if mode == "constraints":
        assert p.rows_read().all()


def test_long_row_reports_once(pair):
    """arrow's row 0 is read by all 256 threads of its workgroup: one event, one store-back"""
    p = pair("secded", "arrow")
    d = p.dam
    assert p.desc[0][3] - (p.desc[0][2] & ~1) > TILE and p.row1[0] == 1
    d.ctx.flip_structure(d.A, "row", 0, [33])
    same(d.spmv(), p.want)
    assert d.take() == ([(EV_FIXED, 0, 33)], False)
    assert np.array_equal(d.ctx.read_structure(d.A)[0], p.ext)


# ---- 3. double flips --------------------------------------------------------------------------------------------------

def double_sites():
    return [("rand", "row", "first"), ("rand", "row", "last"), ("arrow", "row", "long"), ("diag23", "row", "third_trip"),
            ("rand", "block", "first"), ("rand", "block", "last"), ("wide5", "block", "uniform")]


@pytest.mark.parametrize("name,kind,where", double_sites())
def test_double_flip_is_fatal_and_owned_rows_are_not_written(amd, pair, capsys, name, kind, where):
    p = pair("secded", name, collect=False)
    d = p.dam
    if kind == "row":
        if where == "third_trip":
            t = int(np.flatnonzero((p.row1 - p.row0 > 2 * NTHREADS) & (p.flag == 0))[0])
            index = int(p.row0[t]) + 2 * NTHREADS + 7
        else:
            index = {"first": 0, "last": p.n - 1, "long": 0}[where]
        owned = np.zeros(p.n, bool)
        owned[index] = True
        bits, line = [9, 52], "[ECC] double-bit error detected in row extent %d\n" % index
    else:
        index = {"first": 0, "last": len(p.blk) - 1, "uniform": int(np.flatnonzero(p.flag)[0]) if p.flag.any() else -1}[where]
        assert index >= 0
        owned = np.zeros(p.n, bool)
        owned[p.row0[index]:p.row1[index]] = True
        bits, line = [3, 97], "[ECC] double-bit error detected in row block %d\n" % index
    d.ctx.flip_structure(d.A, kind, index, bits)
    stored = d.ctx.read_structure(d.A)
    d.ctx.upload(d.vy, np.full(p.n, SENTINEL))
    d.ctx.spmv(d.A, d.vx, d.vy)
    capsys.readouterr()
    with pytest.raises(amd.FatalEvent) as e:
        d.ctx._drain()
    assert capsys.readouterr().out == line
    assert e.value.events == [(EV_DOUBLE, index, (S.BLOCK << 8) if kind == "block" else 0)]
    y = d.ctx.download(d.vy)
    same(y[owned], np.full(int(owned.sum()), SENTINEL), "owned rows keep the sentinel")
    same(y[~owned], p.want[~owned], "all other rows")
    after = d.ctx.read_structure(d.A)
    assert np.array_equal(after[0], stored[0]) and np.array_equal(after[1], stored[1])
    # the fused product of such a launch reads no unwritten partial: the flips undone, a clean pass
    d.ctx.flip_structure(d.A, kind, index, bits)
    same(d.spmv(sentinel=True), p.want)
    d.ctx._drain()
    assert capsys.readouterr().out == ""


# ---- 4. everything at once --------------------------------------------------------------------------------------------

def test_element_row_word_descriptor_and_vector_in_one_launch(pair):
    p = pair("secded", "rand")
    d, t = p.dam, p.twin
    out = []
    words = d.ctx.stored_words(d.A)
    for b in (d, t):
        b.ctx.encode_vector(b.vx)
    d.ctx.inject_at(d.A, 1234, [37])
    d.ctx.flip_structure(d.A, "row", 2000, [61])
    d.ctx.flip_structure(d.A, "block", 3, [24])
    d.ctx.flip_vector(d.vx, 100, [44])
    for b in (d, t):
        b.ctx.spmv_vecc(b.A, b.vx, b.vy)
        out.append(b.ctx.download(b.vy))
    same(out[0], out[1])
    want = sorted([(EV_ELEMENT, 1234, 37), (EV_FIXED, 2000, 61), (EV_FIXED, 3, 24 | (S.BLOCK << 8)), (EV_VEC, 100, 44)])
    assert d.take() == (want, False) and t.take() == ([], False)
    ext, blk = d.ctx.read_structure(d.A)
    assert np.array_equal(ext, p.ext) and np.array_equal(blk, p.blk) and np.array_equal(d.ctx.stored_words(d.A), words)


# ---- 5. solvers -------------------------------------------------------------------------------------------------------

VARIANTS = ["plain", "jacobi", "vector_ecc", "check_every"]
SOLVERS = [("host", None), ("device", 3), ("device", 16)]


def solve(amd, box, solver, stride, variant, plant):
    from abft_sparse_cg_amd.context import vecc_strip
    ctx, n = box.ctx, box.n
    b, x, r, pv, w = (box.vec(np.zeros(n)) for _ in range(5))
    ctx.upload(b, rhs(n, 1))
    hist = []
    kw = {}
    dinv = None
    if variant == "jacobi":
        dinv = kw["precond"] = ctx.jacobi(box.A)
    if variant == "vector_ecc":
        kw["vector_ecc"] = True
    if variant == "check_every":
        kw["check_every"] = 5

    def each(itr, rr):
        hist.append((itr, float(rr).hex()))
        if plant:
            plant(itr)
    if solver == "host":
        itr, rr = amd.cg_solve(ctx, box.A, b, x, r, pv, w, 40, 1e-20, on_iteration=each, **kw)
    else:
        itr, rr = amd.cg_solve_device(ctx, box.A, b, x, r, pv, w, 40, 1e-20, on_iteration=each, stride=stride, graph=True, **kw)
    xs = ctx.download(x)
    if variant == "vector_ecc":
        xs = vecc_strip(xs)
    return itr, float(rr).hex(), hist, xs, None if dinv is None else ctx.download(dinv)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["lap40", "rand"])
def test_solvers_repair_the_structure_and_compute_the_twins_solve(amd, pair, name, variant):
    p = pair("secded", name)
    d, t = p.dam, p.twin

    def plant(itr):
        if itr == 1:
            d.ctx.flip_structure(d.A, "row", 17, [40])
        if itr == 3:
            d.ctx.flip_structure(d.A, "block", 1, [70])
    for solver, stride in SOLVERS:
        got = solve(amd, d, solver, stride, variant, plant)
        want = solve(amd, t, solver, stride, variant, None)
        assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2], (solver, stride)
        assert got[0] > 16  # (at stride 16 the callbacks that plant the flips run behind the first batch: another must follow)
        same(got[3], want[3], (solver, stride, "x"))
        if variant == "jacobi":
            same(got[4], want[4], "jacobi(A)")
        assert d.take() == (sorted([(EV_FIXED, 17, 40), (EV_FIXED, 1, 70 | (S.BLOCK << 8))]), False), (solver, stride)
        assert t.take() == ([], False)
        ext, blk = d.ctx.read_structure(d.A)
        assert np.array_equal(ext, p.ext) and np.array_equal(blk, p.blk)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------

def test_refusals(amd, pair):
    from abft_sparse_cg_amd import capi
    p = pair("secded", "lap40")
    d = p.dam
    ctx, A, n, k = d.ctx, d.A, p.n, 2
    blocks = [ctx.create_block(n, k) for _ in range(5)]
    for v in blocks:
        ctx.upload(v, np.arange(n * k, dtype=np.float64).reshape(n, k))
    scal = d.vec(np.zeros(64))
    before = [ctx.download(v).copy() for v in blocks] + [ctx.download(d.vx), ctx.download(d.vy)]
    X, R, P, W, B = blocks

    def refused(call, exc, *needles):
        with pytest.raises(exc) as e:
            call()
        for needle in needles:
            assert needle in str(e.value), (needle, str(e.value))
        if exc is capi.AbftError:
            assert e.value.code == -1  # ABFT_ERR_INVALID
    refused(lambda: capi.check(ctx.L.abft_hip_inject_rowptr(A.h, 3, 1)), capi.AbftError, "abft_hip_inject_structure")
    refused(lambda: ctx.spmm(A, P, W, k), capi.AbftError, "protected")
    refused(lambda: capi.check(ctx.L.abft_hip_spmm(ctx.h, A.h, d.vx.h, d.vy.h, 1)), capi.AbftError, "protected")
    refused(lambda: ctx.spmm_dot(A, P, W, k), capi.AbftError, "protected")
    refused(lambda: ctx.spmm_dot_vecc(A, P, W, k), capi.AbftError, "protected")
    refused(lambda: ctx.block_loop_reserve(A, k), capi.AbftError, "protected")
    refused(lambda: ctx.cg_block_iteration_until_dev(A, X, R, P, W, k, scal, 0, 12, 6, 1e-3), capi.AbftError, "protected")
    refused(lambda: ctx.cg_block_vecc_iteration_until_dev(A, X, R, P, W, k, scal, 0, 12, 6, 1e-3), capi.AbftError, "protected")
    refused(lambda: capi.check(ctx.L.abft_hip_spmv_dot_range_dev(ctx.h, A.h, d.vx.h, d.vy.h, 0, scal.device_ptr, 0, 1)),
            capi.AbftError, "protected")
    refused(lambda: amd.cg_solve_block(ctx, A, B, X, R, P, W, 10, 1e-3), ValueError, "structure_ecc")
    from abft_sparse_cg_amd.context import cg_solve_block_device
    refused(lambda: cg_solve_block_device(ctx, A, B, X, R, P, W, 10, 1e-3), ValueError, "structure_ecc")
    assert ctx.drain_events() == ([], False)
    after = [ctx.download(v) for v in blocks] + [ctx.download(d.vx), ctx.download(d.vy)]
    for a, b in zip(after, before):
        same(a, b)
    # the keyword
    cols, rows, vals, n = S.matrix("lap3")
    refused(lambda: ctx.create_matrix(cols, rows, vals, n, len(vals), structure_ecc=True), ValueError, "layout='stream'")
    refused(lambda: ctx.create_matrix(cols, rows, vals, n, len(vals), n_in=n + 1, layout="stream", structure_ecc=True), ValueError)
    coo = amd.HIPContext("secded", "coo")
    try:
        refused(lambda: coo.create_matrix(cols, rows, vals, n, len(vals), layout="stream", structure_ecc=True), ValueError)
        refused(lambda: coo.create_matrix(cols, rows, vals, n, len(vals), structure_ecc=True), ValueError)
    finally:
        coo.close()
    # the limits, checked before an array is read or anything is uploaded: nnz < 2^28, N <= 2^24
    import ctypes as C
    one_u, one_d, h = np.zeros(4, np.uint32), np.zeros(4), C.c_void_p()
    for big_n, big_nnz, needle in ((4, 1 << 28, "2^28"), ((1 << 24) + 1, 0, "2^24")):
        with pytest.raises(capi.AbftError) as e:
            capi.check(ctx.L.abft_hip_matrix_create_csr_protected(ctx.h, ctx.mode_id, one_u.ctypes.data_as(capi.u32p),
                                                                   one_u.ctypes.data_as(capi.u32p), one_d.ctypes.data_as(capi.f64p),
                                                                   big_n, big_nnz, C.byref(h)))
        assert e.value.code == capi.ERR_RANGE and needle in str(e.value) and not h.value
    # the entries of the protected form refuse a plain matrix
    t = p.twin
    refused(lambda: t.ctx.read_structure(t.A) if t.ctx.structure_protected(t.A) else capi.check(
        t.ctx.L.abft_hip_matrix_read_structure(t.A.h, None, None)), capi.AbftError, "not protected")
    refused(lambda: t.ctx.flip_structure(t.A, "row", 0, [1]), capi.AbftError, "not protected")
    refused(lambda: t.ctx.scrub_structure(t.A), capi.AbftError, "not protected")
    refused(lambda: ctx.flip_structure(A, "row", n + 5000, [1]), capi.AbftError, "outside")
    refused(lambda: ctx.flip_structure(A, "row", 0, [64]), capi.AbftError, "outside")
    refused(lambda: ctx.flip_structure(A, "block", 0, [128]), capi.AbftError, "outside")


# ---- 7. the command line ----------------------------------------------------------------------------------------------

def cli(args):
    return subprocess.run([sys.executable, "-m", "abft_sparse_cg_amd.cg", "-t", "hip", "-s", "laplace5:40,40", "-m", "secded",
                           "-i", "30", "-c", "0"] + args, capture_output=True, text=True, timeout=300, cwd=ROOT)


@pytest.mark.parametrize("extra", [[], ["--vector-ecc", "secded"], ["--device-loop", "4"]])
def test_cli(extra):
    flags = ["--structure-ecc", "secded", "--flip-structure", "3:row:17:40", "--flip-structure", "5:block:1:70"]
    plain, got = cli(extra), cli(extra + flags)
    assert plain.returncode == 0 and got.returncode == 0, got.stdout + got.stderr
    rr = lambda text: re.findall(r"^iteration +\d+ : +rr = .*$", text, re.M)  # noqa: E731
    assert len(rr(plain.stdout)) == 30 and rr(got.stdout) == rr(plain.stdout)
    out = got.stdout
    line = "structure protection: secded (row extents (64, 57), row blocks (128, 120))\n"
    assert out.count(line) == 1 and out.index(line) < out.index("iteration     0")
    assert out.count("[ECC] corrected bit 40 of row extent 17\n") == 1
    assert out.count("[ECC] corrected bit 70 of row block 1\n") == 1
    assert out.count("[ECC]") == 2
    assert out.count("structure scrub: 0 corrected\n") == 1
    assert "structure" not in plain.stdout


def test_cli_refuses_block_right_hand_sides():
    p = cli(["--structure-ecc", "secded", "--rhs", "2"])
    assert p.returncode == 1 and "--structure-ecc" in p.stdout and "--rhs" in p.stdout
    p = cli(["--flip-structure", "3:row:17:40"])
    assert p.returncode == 1 and "--structure-ecc" in p.stdout
