"""The device-resident block loop on a protected scalar trail: the two
abft_hip_cg_block[_vecc]_trail_iteration_until_dev entries, abft_hip_block_trail_inject_at, and
cg_solve_block_device(trail_ecc=True, on_batch=...).  Every comparison is bit for bit; the yardstick is the same loop
without the keyword, or a clean twin.

Slots: r.r of column j has ordinal j, its r.z K + j, the events word 2K, the trailing word 2K + 1; in the SpMM's tail
P.W of column j has ordinal j, the events word K.  Events are (kind, ordinal, bit | record << 8): kind 14 a repaired
slot, 15 two flips (fatal); record 0 the record the iteration starts from, 1 the P.W tail, 2 the record it leaves."""
import ctypes as C
import mmap

import numpy as np
import pytest

import _ieee
import _structecc as S
import _vecc
import _vecc_precond as P
from _oracle import rhs
from test_gpu_trail_ecc import SAMPLE, planned_blocks

pytestmark = pytest.mark.gpu

U = np.uint64
FIXED, DOUBLE = 14, 15
VEC_FIXED = 10
START, TAIL, NEXT = 0, 1, 2
LOOPS = ["plain", "jacobi", "vecc"]
# thresholds at which the columns stop at different iterations (lap40: the counts test_gpu_device_loop_block_vecc.py
# pins, 59, 60, 63, 64 for the first four columns; the Jacobi system: 81 and 80 for the first two on a CPU, the
# residuals a few per cent off the threshold on either side)
THRESHOLD = dict(plain=1e-3, vecc=1e-3, jacobi=1e-4)
NAN, NEG0 = float(np.array([0x7FF8000000ABCDEF], U).view(np.float64)[0]), -0.0
_mats = {}


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def matrix(name):
    if name not in _mats:
        _mats[name] = P.scaled_laplace(32, 32, 6) if name == "scaled" else S.matrix(name)
    return _mats[name]


def matrix_of(loop, name="lap40"):
    return matrix("scaled" if loop == "jacobi" else name)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(U).copy()


def rhs_block(n, k):
    return np.stack([rhs(n, 1 + j) for j in range(k)], axis=1)


class Solve:
    """one context, one matrix, K right-hand sides (column j drawn with seed 1 + j): cg_solve_block_device of one of
    the three loops, with or without the keyword"""

    def __init__(self, amd, loop, mode, mat, k, capture=True):
        self.amd, self.loop, self.k = amd, loop, k
        self.events = []
        self.ctx = amd.HIPContext(mode, "csr", device=0,
                                  on_event=(lambda ev, fatal: self.events.extend(ev)) if capture else None)
        cols, rows, vals, n = mat
        self.n = n
        self.A = self.ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        self.v = [self.ctx.create_block(n, k) for _ in range(5)]  # B X R P W
        self.B0 = rhs_block(n, k)
        self.dinv = self.ctx.jacobi(self.A) if loop == "jacobi" else None

    def run(self, **kw):
        ctx = self.ctx
        ctx.upload(self.v[0], self.B0)
        ctx.upload(self.v[1], np.zeros((self.n, self.k)))
        hist, masks = [], []
        self.events.clear()

        def cb(i, rr, active):
            hist.append(rr)
            masks.append(active)
        itrs, rr = self.amd.cg_solve_block_device(ctx, self.A, *self.v, precond=self.dinv, vector_ecc=self.loop == "vecc",
                                                  on_iteration=cb, **kw)
        return list(itrs), bits(np.array(hist)), bits(ctx.download(self.v[1])), list(self.events), masks

    def vectors(self):
        return [bits(self.ctx.download(v)) for v in self.v[1:4]]  # X R P

    def close(self):
        self.ctx.close()


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[4] == b[4]


# ---- 1. clean parity ----

@pytest.mark.parametrize("mode", ["none", "secded"])
@pytest.mark.parametrize("loop", LOOPS)
def test_clean_parity_for_every_k(amd, mode, loop):
    for k in range(1, 9):
        s = Solve(amd, loop, mode, matrix_of(loop), k)
        kw = dict(max_itrs=200, conv_threshold=THRESHOLD[loop], stride=3, graph=True)
        plain, prot = s.run(**kw), s.run(trail_ecc=True, **kw)
        assert same(plain, prot), (k, plain[0], prot[0])
        assert plain[3] == prot[3] == []
        assert min(plain[0]) > 3 and (k == 1 or len(set(plain[0])) > 1), (k, plain[0])  # columns stop apart
        s.close()


@pytest.mark.parametrize("mode", ["none", "secded"])
@pytest.mark.parametrize("loop,name", [("plain", "lap40"), ("plain", "wide5"), ("jacobi", "scaled"), ("vecc", "lap40"),
                                       ("vecc", "wide5")])
def test_clean_parity_at_every_stride(amd, mode, loop, name):
    s = Solve(amd, loop, mode, matrix(name), 4)
    for stride in (1, 16):
        for graph in (True, False):
            kw = dict(max_itrs=200, conv_threshold=THRESHOLD[loop], stride=stride, graph=graph)
            plain, prot = s.run(**kw), s.run(trail_ecc=True, **kw)
            assert same(plain, prot), (stride, graph, plain[0], prot[0])
            assert plain[3] == prot[3] == [] and len(set(plain[0])) > 1, (stride, graph, plain[0])
    s.close()


# ---- 2. every bit of every value slot of the start record, between batches ----

@pytest.mark.parametrize("ordinal", range(6))
def test_every_bit_of_the_start_record_between_batches(amd, ordinal):
    k, rec = 3, 8  # slots per record; stride 1: record 1 starts the next batch
    s = Solve(amd, "plain", "secded", matrix("lap40"), k)
    kw = dict(max_itrs=4, conv_threshold=0.0, stride=1, graph=False, trail_ecc=True)
    clean = s.run(**kw)
    assert clean[0] == [4] * k and clean[3] == []
    for bit in range(128):
        def on_batch(done, trail):
            if done == 2:
                s.ctx.flip_trail(trail, rec + ordinal, [bit])
        hit = s.run(on_batch=on_batch, **kw)
        assert same(hit, clean), bit
        assert hit[3] == [(FIXED, ordinal, bit | START << 8)], (bit, hit[3])
    s.close()


# ---- the C entries, one iteration at a time ----

class Iter:
    """X, R, P, W (dinv) and the slots {start record | P.W tail | next record} of one guarded block iteration"""

    def __init__(self, amd, loop, k=3, mode="secded", mat=None):
        self.loop, self.k, self.vecc = loop, k, loop == "vecc"
        self.rec, self.tail = 2 * k + 2, k + 1  # slots
        self.IN, self.PW, self.OUT = 0, 2 * self.rec, 2 * self.rec + 2 * self.tail  # doubles
        self.size = 4 * self.rec + 2 * self.tail + 8  # (eight doubles to spare: the refusal test's layouts)
        self.events = []
        self.ctx = amd.HIPContext(mode, "csr", device=0, on_event=lambda ev, fatal: self.events.extend(ev))
        cols, rows, vals, n = mat or matrix_of(loop)
        self.n = n
        self.A = self.ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        rng = np.random.default_rng(1)
        vals0 = [rng.standard_normal(n * k) for _ in range(3)] + [np.full(n * k, 7.5)]
        self.start = [bits(_vecc.encode(v).view(np.float64)) if self.vecc else bits(v) for v in vals0]
        self.v = [self.ctx.create_block(n, k) for _ in range(4)]  # X R P W
        self.dinv = self.ctx.jacobi(self.A) if loop == "jacobi" else None
        self.sc = self.ctx.create_vector(self.size)

    def reset(self, rr, rz, out=None):
        for v, a in zip(self.v, self.start):
            self.ctx.upload(v, a.view(np.float64))
        start = np.zeros(self.size)
        start[:2 * self.rec] = self.ctx.encode_trail(list(rr) + list(rz) + [0.0, 0.0])
        start[self.PW:self.OUT] = self.ctx.encode_trail(np.zeros(self.tail))
        start[self.OUT:self.OUT + 2 * self.rec] = self.ctx.encode_trail(np.zeros(self.rec) if out is None else out)
        self.ctx.upload(self.sc, start)
        self.events.clear()

    def until(self, thr, at=None):
        IN, PW, OUT = at or (self.IN, self.PW, self.OUT)
        if self.vecc:
            self.ctx.cg_block_vecc_trail_iteration_until_dev(self.A, *self.v, self.k, self.sc, IN, PW, OUT, thr)
        else:
            self.ctx.cg_block_trail_iteration_until_dev(self.A, *self.v, self.k, self.sc, IN, PW, OUT, thr, dinv=self.dinv)

    def state(self):
        """-> (words of X, R, P, W, the raw slots); the download drains the events"""
        vecs = [bits(self.ctx.download(v)).ravel() for v in self.v]
        return vecs, bits(self.ctx.download(self.sc))

    def values(self, sc):
        """the decoded slots of the three records -> (values, status)"""
        v, st, _ = self.ctx.decode_trail(sc[:self.size - 8].view(np.float64))
        return v, st

    def event_words(self):
        return [2 * self.k, self.rec + self.k, self.rec + self.tail + 2 * self.k]

    def close(self):
        self.ctx.close()


RR, RZ, THR = (3.25, 0.5, 2.5), (2.75, 0.25, 1.75), 1.0  # K = 3, the mask 0b101: column 1 is frozen


@pytest.mark.parametrize("loop", LOOPS)
def test_slots_that_live_inside_an_iteration(amd, loop):
    """block_trail_inject_at, stage 1 (behind the fold) and stage 2 (behind the r half): the outputs of a clean twin,
    and one event each, from the launch that met the flip"""
    it, twin = Iter(amd, loop), Iter(amd, loop)
    k = it.k
    twin.reset(RR, RZ)
    twin.until(THR)
    want_v, want_sc = twin.state()
    assert twin.events == []
    want, st = twin.values(want_sc)
    assert not st.any()
    out = it.rec + it.tail
    # the mask was 0b101: the frozen column's words were handed on, the live ones are new
    assert bits(want[out + 1:out + 2])[0] == bits([RR[1]])[0] and bits(want[out + k + 1:out + k + 2])[0] == bits([RZ[1]])[0]
    assert want[out] != RR[0] and want[out + 2] != RR[2]
    places = [(1, TAIL, 0), (2, TAIL, 2), (2, NEXT, k + 0), (2, NEXT, k + 2)]
    places += [(stage, START, o) for stage in (1, 2) for o in (0, 1, k + 0, k + 1)]  # r.r, r.z of a live, a frozen column
    for stage, record, ordinal in places:
        for bit in SAMPLE:
            it.reset(RR, RZ)
            it.ctx.block_trail_inject_at(stage, record, ordinal, [bit])
            it.until(THR)
            got_v, got_sc = it.state()
            for name, g, w in zip("XRPW", got_v, want_v):
                assert np.array_equal(g, w), (stage, record, ordinal, bit, name)
            # every slot read was stored back clean, every slot written is a fresh encode: the twin's slots, but for
            # the events words, which count the one queued event from the launch that met it on
            v, st = it.values(got_sc)
            assert not st.any(), (stage, record, ordinal, bit)
            keep = [i for i in range(len(v)) if i not in it.event_words()]
            assert np.array_equal(bits(v)[keep], bits(want)[keep]), (stage, record, ordinal, bit)
            assert it.events == [(FIXED, ordinal, bit | record << 8)], (stage, record, ordinal, bit, it.events)
    # the injection is one shot: the next call is clean
    it.reset(RR, RZ)
    it.until(THR)
    assert np.array_equal(it.state()[1], want_sc) and it.events == []
    # the frozen column's P.W slot is not read: two flips there stop nothing and are reported by nobody (the next
    # fold overwrites the slot); neither are two in the next record's r.z of the frozen column, which the r half's
    # publication has just written over anyway when the flip comes at stage 1
    for stage in (1, 2):
        it.reset(RR, RZ)
        it.ctx.block_trail_inject_at(stage, TAIL, 1, [3, 99])
        it.until(THR)
        got_v, got_sc = it.state()
        assert all(np.array_equal(g, w) for g, w in zip(got_v, want_v)) and it.events == []
        damaged = 2 * (it.rec + 1)  # the slot's two doubles
        keep = [i for i in range(len(got_sc)) if i not in (damaged, damaged + 1)]
        assert np.array_equal(got_sc[keep], want_sc[keep]) and not np.array_equal(got_sc, want_sc)
    it.close()
    twin.close()


# ---- 4. a frozen launch ----

@pytest.mark.parametrize("loop", LOOPS)
def test_frozen_launch_hands_on_the_repaired_record_reencoded(amd, loop):
    it = Iter(amd, loop)
    k = it.k
    for rr, rz, thr, slots in (((3.25, 0.5, 2.5), (2.75, 0.25, 1.75), 3.25, ((0, 127), (k + 2, 24))),
                               ((3.25, 0.5, 2.5), (2.75, 0.25, 1.75), np.inf, ((1, 24), (k + 0, 0))),
                               ((NAN, NEG0, 0.0), (NEG0, NAN, 1e300), 0.0, ((0, 70), (k + 1, 66))),
                               ((NEG0, -1.0, NAN), (NAN, NEG0, -np.inf), 0.0, ((2, 64), (k + 0, 126)))):
        it.reset(rr, rz)
        for slot, bit in slots:
            it.ctx.flip_trail(it.sc, slot, [bit])
        it.until(thr)
        got_v, sc = it.state()
        for name, g, w in zip("XRP", got_v, it.start):  # (W is the SpMM's, which always runs)
            assert np.array_equal(g, w), (rr, thr, name)
        v, st = it.values(sc)
        assert not st.any()  # the start record stored back clean, the next one freshly encoded
        out = it.rec + it.tail
        words = bits(list(rr) + list(rz))
        assert np.array_equal(bits(v[:2 * k]), words)  # repaired in place
        assert np.array_equal(bits(v[out:out + 2 * k]), words)  # moved as integers: payloads, -0.0
        assert v[out + 2 * k] == 2.0 and bits(v[out + 2 * k + 1:out + 2 * k + 2])[0] == 0  # this launch's own two events
        assert sorted(it.events) == sorted((FIXED, slot, bit | START << 8) for slot, bit in slots), it.events
    # a mixed launch: the frozen column's words (a payload NaN, -0.0) go on bit for bit, its vectors keep every bit
    it.reset((3.25, NAN, 2.5), (2.75, NEG0, 1.75))
    it.ctx.flip_trail(it.sc, 1, [60])
    it.ctx.flip_trail(it.sc, k + 1, [127])
    it.until(THR)
    got_v, sc = it.state()
    v, st = it.values(sc)
    out = it.rec + it.tail
    assert not st.any() and bits(v[out + 1:out + 2])[0] == bits([NAN])[0] and bits(v[out + k + 1:out + k + 2])[0] == bits([NEG0])[0]
    assert v[out] != 3.25 and v[out + 2 * k] == 2.0
    for name, g, w in zip("XRP", got_v, it.start):
        col = lambda a: a.reshape(-1, k)[:, 1]
        if it.vecc:  # (a frozen column of a live protected launch is stored back as it decodes: the same words here)
            assert np.array_equal(col(g), col(w)), name
        else:
            assert np.array_equal(col(g), col(w)) and not np.array_equal(g, w), name
    assert sorted(it.events) == [(FIXED, 1, 60 | START << 8), (FIXED, k + 1, 127 | START << 8)]
    it.close()


# ---- 5. double flips ----

def plant(s, trail, what, frozen, live, rec, k, copy=False):
    """-> the (ordinal, record) of the slot damaged for the batch that follows"""
    ordinal, record = dict(rr=(frozen, START), rz=(k + live, START), pw=(live, TAIL), next=(k + live, NEXT))[what]
    if copy:  # a clean codeword in the wrong place: the neighbour's slot, word for word
        t = s.ctx.download(trail)
        src = rec + (ordinal + 1) % (2 * k)
        t[2 * (rec + ordinal):2 * (rec + ordinal) + 2] = t[2 * src:2 * src + 2]
        s.ctx.upload(trail, t)
    elif record == START:
        s.ctx.flip_trail(trail, rec + ordinal, [3, 99])  # stride 1: record 1 starts the next batch
    else:
        s.ctx.block_trail_inject_at(1 if what == "pw" else 2, record, ordinal, [3, 99])
    return ordinal, record


@pytest.mark.parametrize("loop", ["plain", "jacobi"])
@pytest.mark.parametrize("what", ["rr", "rz", "pw", "next", "copy"])
def test_double_flips_are_fatal_at_that_batchs_download(amd, loop, what):
    k, rec = 4, 10
    mat = matrix_of(loop)
    kw = dict(conv_threshold=THRESHOLD[loop], stride=1, graph=False, trail_ecc=True)
    twin = Solve(amd, loop, "secded", mat, k)
    masks = twin.run(max_itrs=200, **kw)[4]
    full = (1 << k) - 1
    # a batch in front of an iteration with a frozen and a live column
    m = next(i for i, a in enumerate(masks) if a != full)
    frozen = next(j for j in range(k) if not (masks[m] >> j) & 1)
    live = next(j for j in range(k) if (masks[m] >> j) & 1)
    assert 3 < m < len(masks)
    twin.run(max_itrs=m, **kw)
    want = twin.vectors()
    twin.close()
    s = Solve(amd, loop, "secded", mat, k, capture=False)
    called, seen, where = [], [], []

    def on_batch(done, trail):
        called.append(done)
        if done == m:
            where.append(plant(s, trail, "rr" if what == "copy" else what, frozen, live, rec, k, copy=what == "copy"))

    with pytest.raises(amd.FatalEvent) as e:
        s.ctx.upload(s.v[0], s.B0)
        s.ctx.upload(s.v[1], np.zeros((s.n, k)))
        amd.cg_solve_block_device(s.ctx, s.A, *s.v, max_itrs=200, precond=s.dinv, on_batch=on_batch,
                                  on_iteration=lambda i, rr, a: seen.append(i), **kw)
    ordinal, record = where[0]
    assert e.value.events[-1] == (DOUBLE, ordinal, record << 8), e.value.events
    assert set(e.value.events) == {(DOUBLE, ordinal, record << 8)}
    assert called == list(range(1, m + 1)) and seen == list(range(m))  # raised before any callback of that batch
    got = s.vectors()
    for name, g, w in zip("XRP", got, want):  # X, R and P keep every bit from that r half on
        if what == "next" and name == "R":
            assert not np.array_equal(g, w)  # (the r half had run: R has moved, X and P have not)
        else:
            assert np.array_equal(g, w), (what, name)
    s.close()


# ---- 6. more than one workgroup in the fold, more than 32 in the r half ----

def test_multi_workgroup_fold_and_r_half(amd, tmp_path):
    n, k = 2048 * 1024 + 1, 2
    assert planned_blocks(tmp_path, n) > 2048  # fold_grid: more than one workgroup folds the partials
    assert _ieee.reduce_blocks(n) > 32  # the r half's own partials: more than 32 workgroups
    idx = np.arange(n, dtype=np.uint32)
    vals = np.where(idx % 2 == 1, -1.0, 4.0)  # the matrix that was planned
    events = []
    ctx = amd.HIPContext("none", "csr", device=0, on_event=lambda ev, fatal: events.extend(ev))
    A = ctx.create_matrix(idx, idx, vals, n, n, layout="stream")
    v = [ctx.create_block(n, k) for _ in range(5)]
    B0 = np.stack([1.0 + (idx % 5), 2.0 - (idx % 3) * 0.25], axis=1).astype(np.float64)
    out = []
    for trail in (False, True):
        ctx.upload(v[0], B0)
        ctx.upload(v[1], np.zeros((n, k)))
        hist = []
        if trail:
            ctx.block_trail_inject_at(1, TAIL, 1, [77])
        it, rr = amd.cg_solve_block_device(ctx, A, *v, max_itrs=3, conv_threshold=0.0, stride=3, graph=False,
                                           on_iteration=lambda i, r, a: hist.append(r), trail_ecc=trail)
        out.append((list(it), bits(np.array(hist)), bits(ctx.download(v[1]))))
    assert out[0][0] == out[1][0] == [3, 3]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert events == [(FIXED, 1, 77 | TAIL << 8)], events
    ctx.close()


# ---- 7. protected vectors and the protected trail together ----

def test_a_vector_flip_and_a_trail_flip_in_one_batch(amd):
    k, rec = 4, 10
    s = Solve(amd, "vecc", "secded", matrix("lap40"), k)
    kw = dict(max_itrs=200, conv_threshold=THRESHOLD["vecc"], stride=5, graph=True, trail_ecc=True)
    clean = s.run(**kw)
    assert clean[3] == [] and len(set(clean[0])) > 1
    index, vbit, ordinal, tbit = 200 * k + 3, 62, k + 2, 41

    def on_batch(done, trail):
        if done == 10:
            s.ctx.flip_vector(s.v[1], index, [vbit])  # X: operand 1 of the guarded entries
            s.ctx.flip_trail(trail, rec * 5 + ordinal, [tbit])  # r.z[2] of record `stride`
    hit = s.run(on_batch=on_batch, **kw)
    assert same(hit, clean)
    assert sorted(hit[3]) == sorted([(VEC_FIXED, index, vbit | 1 << 8), (FIXED, ordinal, tbit | START << 8)]), hit[3]
    s.close()


# ---- 8. refusals ----

def test_refusals(amd):
    from abft_sparse_cg_amd import capi
    it = Iter(amd, "plain", mode="none")
    k = it.k
    it.reset(RR, RZ)
    before = it.state()
    with pytest.raises(capi.AbftError, match="overlap"):  # the tail inside the next record
        it.until(THR, at=(it.IN, it.OUT + 4, it.OUT))
    with pytest.raises(capi.AbftError, match="overlap"):  # records apart as plain ones would be, not as slots
        it.until(THR, at=(it.IN, it.PW, it.IN + it.rec))
    with pytest.raises(capi.AbftError, match="16-byte"):
        it.until(THR, at=(it.IN, it.PW + 1, it.OUT + 2))
    with pytest.raises(capi.AbftError, match="16-byte"):
        it.until(THR, at=(it.IN, it.PW, it.OUT + 1))
    it.ctx.graph_begin()  # a fresh context: nothing reserved yet
    try:
        with pytest.raises(capi.AbftError, match="block_loop_reserve"):
            it.until(THR)
    finally:
        g = it.ctx.graph_end()
    it.ctx.graph_destroy(g)
    it.ctx.block_loop_reserve(it.A, k)
    it.ctx.block_trail_inject_at(1, TAIL, 0, [5])
    it.ctx.graph_begin()
    try:
        with pytest.raises(capi.AbftError, match="injection armed"):
            it.until(THR)
    finally:
        g = it.ctx.graph_end()
    it.ctx.graph_destroy(g)
    it.ctx.block_trail_inject_at(1, TAIL, 0, [])  # disarmed
    # a slot the records of this k do not have: refused with the other refusals, nothing enqueued, nothing written
    for record, ordinal, length in ((TAIL, k + 1, k + 1), (TAIL, 2 * k, k + 1), (START, 2 * k + 2, 2 * k + 2), (NEXT, 17, 2 * k + 2)):
        it.ctx.block_trail_inject_at(2, record, ordinal, [5])
        with pytest.raises(capi.AbftError, match="names word %d of a record of %d words" % (ordinal, length)):
            it.until(THR)
    it.ctx.block_trail_inject_at(1, TAIL, 0, [])
    with pytest.raises(capi.AbftError, match="ordinal 18"):
        it.ctx.block_trail_inject_at(1, START, 18, [5])
    with pytest.raises(capi.AbftError, match="ordinal 4"):  # the single entry's own bound stands
        it.ctx.trail_inject_at(1, START, 4, [5])
    # an armed single injection does not fire in a block call (and stays armed for a single one)
    it.ctx.trail_inject_at(1, START, 0, [5])
    it.until(THR)
    clean = it.state()
    assert it.events == [] and not it.values(clean[1])[1].any()
    it.ctx.trail_inject_at(1, START, 0, [])
    it.reset(RR, RZ)
    assert all(np.array_equal(a, b) for a, b in zip(before[0], it.state()[0]))
    board = mmap.mmap(-1, it.ctx.L.abft_hip_peer_board_bytes())
    capi.check(it.ctx.L.abft_hip_peer_board_attach(it.ctx.h, C.addressof(C.c_char.from_buffer(board)), len(board), 0, 1, 5.0))
    try:
        with pytest.raises(capi.AbftError, match="peer board"):
            it.until(THR)
    finally:
        capi.check(it.ctx.L.abft_hip_peer_board_detach(it.ctx.h))
    after = it.state()
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and np.array_equal(before[1], after[1])
    assert it.events == []
    # the solver's own refusals, before anything runs
    cols, rows, vals, n = matrix("lap40")
    structured = it.ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream", structure_ecc=True)
    with pytest.raises(capi.AbftError):  # a structure_ecc matrix: the entry refuses it ...
        it.ctx.cg_block_trail_iteration_until_dev(structured, *it.v, k, it.sc, it.IN, it.PW, it.OUT, THR)
    with pytest.raises(ValueError, match="structure_ecc"):  # ... and so does the solver
        amd.cg_solve_block_device(it.ctx, structured, it.v[0], *it.v, trail_ecc=True)
    dinv = it.ctx.jacobi(it.A)
    with pytest.raises(ValueError, match="precond"):
        amd.cg_solve_block_device(it.ctx, it.A, it.v[0], *it.v, precond=dinv, vector_ecc=True, trail_ecc=True)
    after = it.state()
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and np.array_equal(before[1], after[1])
    assert it.events == []
    it.until(THR)  # and the entry still works
    assert not it.values(it.state()[1])[1].any() and it.events == []
    it.close()
