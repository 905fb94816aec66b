"""Matrix-fault repair at every tile slot of every SpMV and SpMM path.

Every kernel that reads the matrix has a cold path of its own that rebuilds a failed element's index from the lane's
slot number, re-reads the element, writes it back and restages the product.  The sweeps here put one bit flip into
EVERY stored element (tests/_fault_slots.py: the bit walks all 96 / 128 positions; 4096 elements per pass, the
oracle wrapper's buffer) and make the call once.  Asserted, all bit for bit: the drained events are the oracle's for
the same flips (tuples and printed lines, in the drain's order: by element index); nothing is fatal; every output
equals that of a CLEAN TWIN -- the same call on an undamaged matrix in a second context --; the stored words are the
clean words again; the call repeated drains nothing.  test_fault_slots_host.py shows on the oracle alone that these
inputs leave nothing out.

Detecting outcomes (sed: one flip; secded: two flips in one element) go one flip per run: exactly the oracle's one
fatal event and its line, and after the flip is undone a silent pass with the clean twin's output.

Every call starts from uploaded inputs, so a twin's output is computed once per case.  Not swept, because the
library documents them as refused: protected vectors and block vectors outside streaming CSR (the parameter lists
below name CSR alone for those paths); `constraints` is no ECC mode and has its own tests.

The x-in-SpMV kernels: abft_hip_inject applies every queued x update before it flips anything (it is not one of
the loop's four calls), so through the C ABI the SpMV that reads freshly planted flips takes ONE update along -- it
applies it (ABFT_HIP_LAZY_X=1) or queues it (2, 4) -- and the launch that applies 2 or 4 comes later in the same
call, on elements already repaired; the counters prove both.  Flips that are only detected stay, so the launches
that apply 2 and 4 updates do meet those: the count of queued events shows that each of them reported one."""
import numpy as np
import pytest

from _fault_slots import (CORRECTING, FNAME, SEEDS, TwinOracle, chunks, fatal_sites, flip_plan, second_bit,
                          sweep_matrix)
from _loop_scripts import SWITCHES
from _oracle import COO, CSR, EV_DOUBLE, EV_SED, event_lines, rhs
from _x_in_spmv import loop

pytestmark = pytest.mark.gpu

SWEPT = ["arrow1300", "holes"]  # every path; the plain spmv sweeps also run "rand" and "diag23" (the 1024-row cap)
DETECTING = ["sed", "secded"]
VEC_CORRECTED = 10  # ABFT_EV_VEC_CORRECTED: (kind, index in the vector, bit)
VEC_BIT = 44
STRIDE = 5  # fatal_sites of every path but plain spmv


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want, tag=None):
    assert len(got) == len(want), tag
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = u64(a), u64(b)
        assert a.shape == b.shape and np.array_equal(a, b), (tag, k, int(np.count_nonzero(a != b)) if a.shape == b.shape else -1)


class Box:
    """one context and one matrix, events collected instead of printed"""

    def __init__(self, amd, fmt, mode, mat, stream=False):
        cols, rows, vals, n = mat
        self.events, self.fatal = [], False
        self.ctx = amd.HIPContext(mode, FNAME[fmt], on_event=self._on)
        self.fmt, self.mode, self.n, self.nnz, self.cols = fmt, mode, n, len(vals), cols
        self.A = self.ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream" if stream else None)

    def _on(self, ev, fatal):
        self.events += ev
        self.fatal |= fatal

    def take(self):
        self.ctx._drain()  # (synchronises the stream)
        ev, f = self.events, self.fatal
        self.events, self.fatal = [], False
        return ev, f

    def vec(self, array):
        v = self.ctx.create_vector(len(array))
        self.ctx.upload(v, array)
        return v

    def block(self, array):
        v = self.ctx.create_block(*array.shape)
        self.ctx.upload(v, array)
        return v

    def inject(self, i, bits):
        self.ctx.inject_at(self.A, int(i), [int(b) for b in bits])

    def words(self):
        return self.ctx.stored_words(self.A)


class Case:
    """the damaged box, its clean twin and the oracle of one (format, mode, matrix); `make(box)` returns the path's call
    on that box: call(plant=None) -> list of arrays, `plant` a function the call runs where the flips belong (for
    most paths: first)"""

    def __init__(self, amd, fmt, mode, name, make, stream=False, layout=None):
        mat = sweep_matrix(name)
        self.fmt, self.mode, self.n = fmt, mode, mat[3]
        self.x = rhs(self.n, 7) - 0.5
        self.co = TwinOracle(fmt, mode, mat)
        self.dam, self.twin = Box(amd, fmt, mode, mat, stream), Box(amd, fmt, mode, mat, stream)
        try:
            if layout is not None:
                for b in (self.dam, self.twin):
                    assert b.ctx.matrix_info(b.A)[0] == layout, (b.ctx.matrix_info(b.A), layout)
            assert np.array_equal(self.dam.words(), self.co.words)
            self.call, self.twin_call = make(self.dam, self.x), make(self.twin, self.x)
            self.want = self.twin_call()
            assert self.twin.take() == ([], False)
            same(self.call(), self.want, "clean")  # the damaged box before any damage
            assert self.dam.take() == ([], False)
        except BaseException:
            self.close()
            raise

    def close(self):
        self.dam.ctx.close()
        self.twin.ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def sweep(case, oracle_y=False, vector_flip=None):
    """a flip in every element, chunk by chunk and seed by seed -> events compared.  vector_flip(box, chunk) ->
    (flip, undo, event): one more flip, in a vector word that a flipped element gathers"""
    dam, co, fmt = case.dam, case.co, case.fmt
    compared = 0
    for seed in SEEDS:
        plan = flip_plan(fmt, co.mode, co.nnz, seed)
        for ch in chunks(co.nnz):
            tag = (FNAME[fmt], co.mode, seed, ch)
            extra = []
            if vector_flip is not None:
                flip, undo, event = vector_flip(dam, ch)
                flip()
                extra = [event]

            def plant():
                for i in ch:
                    dam.inject(i, [plan[i]])

            co.plant(ch, plan)
            got = case.call(plant)
            ev, fatal = dam.take()
            oy, oev, ofatal = co.run(case.x)
            assert len(oev) == len(ch) and not ofatal, tag
            assert not fatal, tag
            if extra:
                assert sorted(ev) == sorted(oev + extra), tag
                ev = [e for e in ev if e[0] != VEC_CORRECTED]
                undo()
            assert ev == oev, (tag, ev[:3], oev[:3], len(ev))
            assert event_lines(ev, fmt) == event_lines(oev, fmt), tag
            same(got, case.want, tag)
            if oracle_y:
                same(got[:1], [oy], tag)
            assert np.array_equal(dam.words(), co.words), tag
            same(case.call(), case.want, tag)
            assert dam.take() == ([], False), tag
            compared += len(ev)
    assert compared == len(SEEDS) * co.nnz
    return compared


def detect(case, stride):
    """one flip per run (sed) or two in one element (secded): the oracle's one fatal event, then undone and silent"""
    dam, co, fmt = case.dam, case.co, case.fmt
    kind = EV_SED if co.mode == "sed" else EV_DOUBLE
    plan = flip_plan(fmt, co.mode, co.nnz, 1)
    sites = fatal_sites(co.nnz, stride)
    assert sites[:2] == [0, 1] and sites[-2:] == [co.nnz - 2, co.nnz - 1]
    for i in sites:
        bits = [int(plan[i])] + ([second_bit(fmt, int(plan[i]))] if co.mode == "secded" else [])
        co.o.inject(i, bits)
        case.call(lambda: dam.inject(i, bits))
        ev, fatal = dam.take()
        _, oev, ofatal = co.run(case.x)
        assert ofatal and oev == [(kind, i, 0)], (i, oev)
        assert fatal and ev == oev, (i, bits, ev, oev)
        assert event_lines(ev, fmt) == event_lines(oev, fmt), i
        co.o.inject(i, bits)
        dam.inject(i, bits)
        same(case.call(), case.want, i)
        assert dam.take() == ([], False), i
    assert np.array_equal(dam.words(), co.words)
    return len(sites)


# ------------------------------------------------------------------------------------------------ the paths --

def make_spmv(box, x):
    ctx, A, nan = box.ctx, box.A, np.full(box.n, np.nan)
    vx, vy = box.vec(x), box.vec(nan)

    def call(plant=None):
        if plant:
            plant()
        ctx.upload(vy, nan)
        ctx.spmv(A, vx, vy)
        return [ctx.download(vy)]
    return call


def make_spmv_dot_dev(box, x):
    """FUSE: y and the fused x . y in one launch, both on the device (word 1 of the pair counts queued events)"""
    from abft_sparse_cg_amd import capi
    ctx, A, nan = box.ctx, box.A, np.full(box.n, np.nan)
    vx, vy, sc = box.vec(x), box.vec(nan), box.vec(np.zeros(2))

    def call(plant=None):
        if plant:
            plant()
        ctx.upload(vy, nan)
        ctx.upload(sc, np.zeros(2))
        capi.check(ctx.L.abft_hip_spmv_dot_dev(ctx.h, A.h, vx.h, vy.h, 0, sc.device_ptr))
        return [ctx.download(vy), ctx.download(sc)[:1]]
    return call


def make_spmv_part(asked, blocks):
    """the interior rows, then the boundary rows: what one launch leaves.  asked: the range handed to set_interior;
    blocks: the rows of the whole row blocks inside it, which is what the interior launch multiplies.  Before anything
    is planted each part runs alone on a NaN y: the interior writes exactly `blocks`, the boundary exactly the rest --
    so both launches of every later call do work, the boundary one on spans on both sides of the interior"""
    def make(box, x):
        from abft_sparse_cg_amd import capi
        ctx, A, nan = box.ctx, box.A, np.full(box.n, np.nan)
        vx, vy = box.vec(x), box.vec(nan)
        ctx.set_interior(A, *asked)
        inside = np.zeros(box.n, bool)
        inside[blocks[0]:blocks[1]] = True
        assert asked[0] < blocks[0] < blocks[1] < asked[1] and 0 < blocks[0] and blocks[1] < box.n
        for part, rows in ((capi.PART_INTERIOR, inside), (capi.PART_BOUNDARY, ~inside)):
            ctx.upload(vy, nan)
            ctx.spmv(A, vx, vy, part)
            assert np.array_equal(~np.isnan(ctx.download(vy)), rows), part

        def call(plant=None):
            if plant:
                plant()
            ctx.upload(vy, nan)
            ctx.spmv(A, vx, vy, capi.PART_INTERIOR)  # (no download in between: one drain, one order of events)
            ctx.spmv(A, vx, vy, capi.PART_BOUNDARY)
            return [ctx.download(vy)]
        return call
    return make


def make_spmv_vecc(box, x):
    """VECC: x and y codewords; the fused product comes back through dot_vecc"""
    ctx, A = box.ctx, box.A
    vx, vy = box.vec(x), box.vec(np.zeros(box.n))
    ctx.encode_vector(vx)
    box.gathered, box.width = vx, 1

    def call(plant=None):
        if plant:
            plant()
        ctx.upload(vy, np.zeros(box.n))
        ctx.spmv_vecc(A, vx, vy)
        pw = ctx.dot_vecc(vx, vy)
        return [ctx.download(vy), [pw]]
    return call


def block_of(x, k):
    return np.stack([np.roll(x, 17 * j) * (1.0 + 0.25 * j) for j in range(k)], axis=1)


def make_spmm(entry, k):
    def make(box, x):
        ctx, A = box.ctx, box.A
        X = block_of(x, k)
        vX, vY = box.block(X), box.block(np.zeros((box.n, k)))
        if entry == "spmm_dot_vecc":
            ctx.encode_vector(vX)
            box.gathered, box.width = vX, k

        def call(plant=None):
            if plant:
                plant()
            ctx.upload(vY, np.full((box.n, k), 0.0 if entry == "spmm_dot_vecc" else np.nan))
            if entry == "spmm":
                ctx.spmm(A, vX, vY, k)
                return [ctx.download(vY)]
            pw = getattr(ctx, entry)(A, vX, vY, k)
            return [ctx.download(vY), pw]
        call.X = X
        return call
    return make


def gathered_word_flip(box, ch):
    """one flip in the word of the gathered vector that the chunk's middle element reads (block vectors: its column
    k - 1); read-only operands are not written back, so the flip is undone by hand"""
    col = int(box.cols[ch[len(ch) // 2]])
    index = col * box.width + box.width - 1
    flip = lambda: box.ctx.flip_vector(box.gathered, index, [VEC_BIT])  # noqa: E731
    return flip, flip, (VEC_CORRECTED, index, VEC_BIT)


def make_x_in_spmv(depth):
    """The host-scalar loop with the x updates riding in the SpMV (ABFT_HIP_X_IN_SPMV=1, ABFT_HIP_LAZY_X=depth; the
    environment is set by the test).  Three warm iterations arm the prediction, SpMV 3 runs, the flips go in right
    behind it (where the prediction stays armed; queued updates are applied by the inject), and `depth` more
    iterations follow: their first SpMV reads the flips and takes the pending update along, their last applies
    `depth` of them in one launch.  Events stay queued on the device until the call's downloads: a drain in between
    would apply the queue on its own.  alpha and beta are chosen (tests/_x_in_spmv.py), nothing has to converge."""
    def make(box, x):
        import ctypes as C
        from abft_sparse_cg_amd import capi
        ctx, A, n = box.ctx, box.A, box.n
        out = C.c_double()
        rng = np.random.default_rng(11)
        start = [rng.random(n) - 0.5 for _ in range(3)] + [np.zeros(n)]
        vs = [box.vec(a) for a in start]
        vx, vr, vp, vw = vs
        steps = loop(4 + depth)
        box.counters, box.pending = [], []

        def call(plant=None):
            for v, a in zip(vs, start):
                ctx.upload(v, a)
            scalars, spmvs, pend = [], 0, []
            for step in steps:
                if step[0] == "spmv":
                    ctx.spmv(A, vp, vw)
                    spmvs += 1
                    if spmvs == 4:
                        if plant:
                            plant()
                        mid = ctx.x_in_spmv_stats() + ctx.lazy_x_stats()
                elif step[0] == "dot":  # (the C entries: HIPContext.dot and .calc_xr drain pending events first)
                    capi.check(ctx.L.abft_hip_dot(ctx.h, vp.h, vw.h, C.byref(out)))
                    scalars.append(out.value)
                    if spmvs >= 4:  # events queued so far, as this dot's result says
                        pend.append(ctx.L.abft_hip_pending_events(ctx.h))
                elif step[0] == "calc_xr":
                    capi.check(ctx.L.abft_hip_calc_xr(ctx.h, vx.h, vr.h, vp.h, vw.h, step[1], C.byref(out)))
                    scalars.append(out.value)
                else:
                    ctx.calc_p(vp, vr, step[1])
            end = ctx.x_in_spmv_stats() + ctx.lazy_x_stats()  # (before the downloads apply what is left)
            box.counters.append(tuple(e - m for e, m in zip(end, mid)))
            box.pending.append(tuple(pend))
            return [np.array(scalars)] + [ctx.download(v) for v in vs]
        return call
    return make


def make_guarded_iteration(frozen):
    """cg_iteration_until_dev from uploaded x, r, p and r.r: live (threshold 0), or frozen (threshold above r.r: the
    SpMV still runs, x, r and p keep every bit).  Words 1, 3 and 5 of the scalars count queued events: not compared"""
    def make(box, x):
        ctx, A, n = box.ctx, box.A, box.n
        rng = np.random.default_rng(13)
        x0, r0 = rng.random(n) - 0.5, rng.random(n) - 0.5
        start = [x0, r0, r0.copy(), np.zeros(n)]
        vs = [box.vec(a) for a in start]
        vx, vr, vp, vw = vs
        sc = box.vec(np.zeros(6))
        rr = ctx.dot(vr, vr)
        assert rr > 0.0

        def call(plant=None):
            if plant:
                plant()
            for v, a in zip(vs, start):
                ctx.upload(v, a)
            ctx.upload(sc, np.array([rr, 0.0, 0.0, 0.0, 0.0, 0.0]))
            ctx.cg_iteration_until_dev(A, vp, vx, vr, vp, vw, sc, 0, 2, 4, 2.0 * rr if frozen else 0.0)
            s = ctx.download(sc)
            out = [ctx.download(v) for v in vs]
            if frozen:
                same(out[:3], start[:3], "frozen")
                assert u64(s[4:5]) == u64(np.array([rr]))  # the pair handed on
            else:
                assert not np.array_equal(u64(out[0]), u64(x0)) and 0.0 < s[4] != rr
            assert not np.array_equal(u64(out[3]), u64(start[3]))  # the SpMV ran
            return out + [s[0::2]]
        return call
    return make


# --------------------------------------------------------------- 1. plain spmv: the streaming / grouped layouts --

@pytest.mark.parametrize("fmt", [CSR, COO], ids=FNAME.get)
@pytest.mark.parametrize("mode", CORRECTING)
@pytest.mark.parametrize("name", SWEPT + ["rand", "diag23"])
def test_spmv_repairs_a_flip_in_every_element(amd, name, mode, fmt, monkeypatch):
    monkeypatch.delenv("ABFT_HIP_LAYOUT", raising=False)
    with Case(amd, fmt, mode, name, make_spmv, layout="stream") as case:
        sweep(case, oracle_y=True)


@pytest.mark.parametrize("fmt", [CSR, COO], ids=FNAME.get)
@pytest.mark.parametrize("mode", DETECTING)
@pytest.mark.parametrize("name", SWEPT)
def test_spmv_detects_a_flip_in_any_element(amd, name, mode, fmt, monkeypatch):
    monkeypatch.delenv("ABFT_HIP_LAYOUT", raising=False)
    with Case(amd, fmt, mode, name, make_spmv, layout="stream") as case:
        detect(case, 1)


# ------------------------------------------------------------------------------------ 2. the forced layouts --

WIDTH = "64"  # arrow1300: 21 panels, holes: 32
LAYOUTS = {
    "csr-panels": (CSR, "panels", dict(ABFT_HIP_LAYOUT="panels", ABFT_HIP_PANEL_CHUNK="3")),
    "csr-sweep2": (CSR, "sweep", dict(ABFT_HIP_LAYOUT="sweep", ABFT_HIP_SWEEP_RPT="2", ABFT_HIP_SWEEP_LAG="1")),
    "csr-sweep4": (CSR, "sweep", dict(ABFT_HIP_LAYOUT="sweep", ABFT_HIP_SWEEP_RPT="4", ABFT_HIP_SWEEP_LAG="1")),
    "csr-sweep8": (CSR, "sweep", dict(ABFT_HIP_LAYOUT="sweep", ABFT_HIP_SWEEP_RPT="8", ABFT_HIP_SWEEP_LAG="2")),
    "csr-sweep16": (CSR, "sweep", dict(ABFT_HIP_LAYOUT="sweep", ABFT_HIP_SWEEP_RPT="16", ABFT_HIP_SWEEP_LAG="0")),
    "csr-slice": (CSR, "slice", dict(ABFT_HIP_LAYOUT="slice", ABFT_HIP_SLICE_ROWS="64", ABFT_HIP_SLICE_LAG="2")),
    "coo-panels": (COO, "panels", dict(ABFT_HIP_LAYOUT="panels", ABFT_HIP_PANEL_CHUNK="3")),
    "coo-panels-lean": (COO, "panels", dict(ABFT_HIP_LAYOUT="panels", ABFT_HIP_PANEL_CHUNK="3", ABFT_HIP_COO_LEAN="1")),
    "coo-panels-pc": (COO, "panels", dict(ABFT_HIP_LAYOUT="panels", ABFT_HIP_PANEL_CHUNK="3", ABFT_HIP_COO_PC="1")),
}
LAYOUT_KNOBS = ["ABFT_HIP_LAYOUT", "ABFT_HIP_PANEL_WIDTH", "ABFT_HIP_PANEL_CHUNK", "ABFT_HIP_SWEEP_RPT", "ABFT_HIP_SWEEP_LAG",
                "ABFT_HIP_SLICE_ROWS", "ABFT_HIP_SLICE_LAG", "ABFT_HIP_COO_LEAN", "ABFT_HIP_COO_PC"]


def forced(monkeypatch, which):
    fmt, layout, env = LAYOUTS[which]
    for k in LAYOUT_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ABFT_HIP_PANEL_WIDTH", WIDTH)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return fmt, layout


@pytest.mark.parametrize("mode", CORRECTING)
@pytest.mark.parametrize("name", SWEPT)
@pytest.mark.parametrize("which", sorted(LAYOUTS))
def test_forced_layout_repairs_a_flip_in_every_element(amd, which, name, mode, monkeypatch):
    fmt, layout = forced(monkeypatch, which)
    with Case(amd, fmt, mode, name, make_spmv, layout=layout) as case:
        sweep(case, oracle_y=True)


@pytest.mark.parametrize("mode", DETECTING)
@pytest.mark.parametrize("name", SWEPT)
@pytest.mark.parametrize("which", sorted(LAYOUTS))
def test_forced_layout_detects_a_flip(amd, which, name, mode, monkeypatch):
    fmt, layout = forced(monkeypatch, which)
    with Case(amd, fmt, mode, name, make_spmv, layout=layout) as case:
        detect(case, STRIDE)


# ------------------------------------------------- 3. the fused product, the two parts, the protected vectors --

# Interior ranges that start and end inside row blocks.  set_interior keeps the whole row blocks inside the range:
# arrow1300 is cut (1024-element tile) into rows [0, 1) [1, 513) [513, 1025) [1025, 1300), holes into [0, 768)
# [768, 1536) [1536, 2000) -- so each interior is one block, with blocks of the boundary part on both sides, and
# make_spmv_part holds the two parts against exactly these rows
INTERIOR = {"arrow1300": ((300, 1100), (513, 1025)), "holes": ((500, 1700), (768, 1536))}
SINGLE = {
    "spmv_dot_dev-csr": (CSR, lambda name: make_spmv_dot_dev, False, None),
    "spmv_dot_dev-coo": (COO, lambda name: make_spmv_dot_dev, False, None),
    "spmv_part": (CSR, lambda name: make_spmv_part(*INTERIOR[name]), False, None),
    "spmv_vecc": (CSR, lambda name: make_spmv_vecc, True, None),
    "spmv_vecc+x-flip": (CSR, lambda name: make_spmv_vecc, True, gathered_word_flip),
    "spmm_dot_vecc-k2": (CSR, lambda name: make_spmm("spmm_dot_vecc", 2), True, None),
    "spmm_dot_vecc-k3": (CSR, lambda name: make_spmm("spmm_dot_vecc", 3), True, None),
    "spmm_dot_vecc-k3+p-flip": (CSR, lambda name: make_spmm("spmm_dot_vecc", 3), True, gathered_word_flip),
    "guarded-live": (CSR, lambda name: make_guarded_iteration(False), False, None),
    "guarded-frozen": (CSR, lambda name: make_guarded_iteration(True), False, None),
}


def single_case(amd, which, name, mode, monkeypatch):
    monkeypatch.delenv("ABFT_HIP_LAYOUT", raising=False)
    fmt, maker, stream, vflip = SINGLE[which]
    case = Case(amd, fmt, mode, name, maker(name), stream=stream, layout="stream")
    if which == "spmv_part":  # two launches leave what one leaves
        try:
            one = Box(amd, fmt, mode, sweep_matrix(name))
            same(make_spmv(one, case.x)(), case.want, "one launch")
            one.ctx.close()
        except BaseException:
            case.close()
            raise
    return case, vflip


@pytest.mark.parametrize("mode", CORRECTING)
@pytest.mark.parametrize("name", SWEPT)
@pytest.mark.parametrize("which", sorted(SINGLE))
def test_path_repairs_a_flip_in_every_element(amd, which, name, mode, monkeypatch):
    case, vflip = single_case(amd, which, name, mode, monkeypatch)
    with case:
        sweep(case, vector_flip=vflip)


@pytest.mark.parametrize("mode", DETECTING)
@pytest.mark.parametrize("name", SWEPT)
@pytest.mark.parametrize("which", sorted(k for k in SINGLE if "flip" not in k))
def test_path_detects_a_flip(amd, which, name, mode, monkeypatch):
    case, _ = single_case(amd, which, name, mode, monkeypatch)
    with case:
        detect(case, STRIDE)


# --------------------------------------------------------------------------------- 4. spmm and spmm_dot --

KS = [2, 3, 4, 5, 8]  # K <= 4 and K > 4 unroll the row sum differently


def block_case(amd, entry, k, name, mode):
    case = Case(amd, CSR, mode, name, make_spmm(entry, k), stream=True, layout="stream")
    try:  # column j is plain spmv of column j
        box = Box(amd, CSR, mode, sweep_matrix(name), stream=True)
        X = case.twin_call.X
        for j in range(k):
            y = make_spmv(box, np.ascontiguousarray(X[:, j]))()[0]
            same([np.ascontiguousarray(case.want[0][:, j])], [y], ("column", j))
        box.ctx.close()
    except BaseException:
        case.close()
        raise
    return case


@pytest.mark.parametrize("mode", CORRECTING)
@pytest.mark.parametrize("name", SWEPT)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("entry", ["spmm", "spmm_dot"])
def test_spmm_repairs_a_flip_in_every_element(amd, entry, k, name, mode, monkeypatch):
    monkeypatch.delenv("ABFT_HIP_LAYOUT", raising=False)
    with block_case(amd, entry, k, name, mode) as case:
        sweep(case)


@pytest.mark.parametrize("mode", DETECTING)
@pytest.mark.parametrize("name", SWEPT)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("entry", ["spmm", "spmm_dot"])
def test_spmm_detects_a_flip(amd, entry, k, name, mode, monkeypatch):
    monkeypatch.delenv("ABFT_HIP_LAYOUT", raising=False)
    with block_case(amd, entry, k, name, mode) as case:
        detect(case, STRIDE)


# --------------------------------------------------------------------------- 5. the x updates inside the SpMV --

def x_in_spmv_case(amd, depth, name, mode, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.delenv("ABFT_HIP_LAYOUT", raising=False)
    monkeypatch.setenv("ABFT_HIP_X_IN_SPMV", "1")  # (the library reads both when a context is made)
    monkeypatch.setenv("ABFT_HIP_LAZY_X", str(depth))
    return Case(amd, CSR, mode, name, make_x_in_spmv(depth), layout="stream")


def rode_along(counters, depth, planted):
    """(absorbed, flushed, bursts, applied_in_bursts, applied_by_flush) between the planting point and the end of the
    call: `depth` SpMVs took a pending update over; with depth > 1 the last of them applied `depth` in one launch,
    and nothing was applied on its own -- except, in a planted run, what the inject found queued"""
    for absorbed, flushed, bursts, in_bursts, by_flush in counters:
        assert absorbed == depth and flushed == 0, counters
        assert (bursts, in_bursts) == ((1, depth) if depth > 1 else (0, 0)), counters
        assert by_flush == 0 or planted, counters


@pytest.mark.parametrize("mode", CORRECTING)
@pytest.mark.parametrize("name", SWEPT)
@pytest.mark.parametrize("depth", [1, 2, 4])
def test_x_in_spmv_repairs_a_flip_in_every_element(amd, depth, name, mode, monkeypatch):
    with x_in_spmv_case(amd, depth, name, mode, monkeypatch) as case:
        sweep(case)
        print("x-in-SpMV counters behind the flips, depth %d: %s" % (depth, sorted(set(case.dam.counters))))
        rode_along(case.dam.counters, depth, True)
        rode_along(case.twin.counters, depth, False)
        nnz = case.co.nnz  # one chunk: every flip is queued by the first SpMV behind it, none again
        assert set(case.dam.pending) == {(0,) + (nnz,) * depth, (0,) * (depth + 1)}, set(case.dam.pending)


@pytest.mark.parametrize("mode", DETECTING)
@pytest.mark.parametrize("name", SWEPT)
@pytest.mark.parametrize("depth", [1, 2, 4])
def test_x_in_spmv_detects_a_flip(amd, depth, name, mode, monkeypatch):
    """the flip stays, so each of the `depth` SpMVs behind it queues its event -- the one that applies `depth` updates
    too: the count of queued events grows by one with every dot behind the flip.  The one drain at the end of the call
    hands over the first fatal event, as the reference stops at its first fatal line"""
    with x_in_spmv_case(amd, depth, name, mode, monkeypatch) as case:
        detect(case, STRIDE)
        rode_along(case.dam.counters, depth, True)
        assert set(case.dam.pending) == {tuple(range(depth + 1)), (0,) * (depth + 1)}, set(case.dam.pending)


# ----------------------------------------------------------------------------------------- 6. the solvers --

K_SOLVE = 3
CONV, MAX_ITRS, BATCH = 1e-18, 40, 4  # arrow1300: 12 iterations (the oracle's count); 4 to a batch of the device loops
# Jacobi solves arrow1300 to 1e-18 in 3 iterations, before on_iteration(3): those two run to an iteration limit instead
STOP_AT_LIMIT = dict(conv_threshold=0.0, max_itrs=2 * BATCH)
SOLVERS = {
    "cg_solve": ("cg_solve", {}),
    "cg_solve-precond": ("cg_solve", dict(precond=True, **STOP_AT_LIMIT)),
    "cg_solve-vecc": ("cg_solve", dict(vector_ecc=True)),
    "cg_solve_device": ("cg_solve_device", dict(stride=BATCH)),
    "cg_solve_device-precond": ("cg_solve_device", dict(stride=BATCH, precond=True, **STOP_AT_LIMIT)),
    "cg_solve_device-vecc": ("cg_solve_device", dict(stride=BATCH, vector_ecc=True)),
    "cg_solve_device-check5": ("cg_solve_device", dict(stride=BATCH, check_every=5)),
    "cg_solve_block": ("cg_solve_block", dict(fused=False)),
    "cg_solve_block-fused": ("cg_solve_block", dict(fused=True)),
    "cg_solve_block-vecc": ("cg_solve_block", dict(vector_ecc=True)),
    "cg_solve_block_device": ("cg_solve_block_device", dict(stride=BATCH)),
    "cg_solve_block_device-vecc": ("cg_solve_block_device", dict(stride=BATCH, vector_ecc=True)),
}


def solve(amd, box, which, plant):
    """-> (iterations, rr history, x, index into box.events where the second planting went in)"""
    fn, kw = SOLVERS[which]
    kw = dict(kw)
    ctx, A, n = box.ctx, box.A, box.n
    block = "block" in fn
    b = rhs(n, 1)
    if block:
        vs = [box.block(block_of(b, K_SOLVE))] + [box.block(np.zeros((n, K_SOLVE))) for _ in range(4)]
    else:
        vs = [box.vec(b)] + [box.vec(np.zeros(n)) for _ in range(4)]
    if kw.get("precond"):
        kw["precond"] = ctx.jacobi(A)  # (reads the matrix: before anything is planted)
    hist, mark = [], []

    def on_iteration(itr, rr, *active):
        hist.append(np.array(rr, dtype=np.float64).copy().reshape(-1))
        if itr == 3:  # (the twin makes the same calls, the planting apart)
            ctx._drain()
            mark.append(len(box.events))
            if plant:
                plant()

    if plant:
        plant()
    kw.setdefault("max_itrs", MAX_ITRS)
    kw.setdefault("conv_threshold", CONV)
    its, rr = getattr(amd, fn)(ctx, A, *vs, on_iteration=on_iteration, **kw)
    x = ctx.download(vs[1])
    return np.array(its).reshape(-1), np.concatenate(hist), x, (mark[0] if mark else None)


@pytest.mark.parametrize("which", sorted(SOLVERS))
def test_solver_repairs_every_element_twice_and_keeps_every_bit(amd, which, monkeypatch):
    monkeypatch.delenv("ABFT_HIP_LAYOUT", raising=False)
    mat = sweep_matrix("arrow1300")
    co = TwinOracle(CSR, "secded", mat)
    ch = chunks(co.nnz)[0]
    plan = flip_plan(CSR, "secded", co.nnz, 2)
    co.plant(ch, plan)
    _, oev, ofatal = co.run(rhs(co.n, 1))
    assert len(oev) == len(ch) and not ofatal
    dam, twin = Box(amd, CSR, "secded", mat, stream=True), Box(amd, CSR, "secded", mat, stream=True)
    try:
        def plant():
            for i in ch:
                dam.inject(i, [plan[i]])

        its, hist, x, mark = solve(amd, dam, which, plant)
        ev, fatal = dam.take()
        want_its, want_hist, want_x, _ = solve(amd, twin, which, None)
        assert twin.take() == ([], False)
        assert want_its.max() > 4  # the second planting was read by an SpMV: iteration 4's, the second batch's first
        assert np.array_equal(its, want_its), (its, want_its)
        same([hist], [want_hist], "rr history")
        same([x], [want_x], "x")
        assert not fatal and mark is not None
        assert ev[:mark] == oev and ev[mark:] == oev, (mark, len(ev), ev[:2], ev[mark:mark + 2])
        assert np.array_equal(dam.words(), co.words)
    finally:
        dam.ctx.close()
        twin.ctx.close()
