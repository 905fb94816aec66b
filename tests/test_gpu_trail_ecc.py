"""The device-resident CG loop on a protected scalar trail: the four
abft_hip_*_trail_iteration_until_dev entries, abft_hip_trail_flip / abft_hip_trail_inject_at, and
cg_solve_device(trail_ecc=True, on_batch=...).  Every comparison is bit for bit; the yardstick is the same loop
without the keyword, or a clean twin context.

Events are (kind, ordinal, bit | record << 8): kind 14 a repaired slot, 15 two flips (fatal); record 0 the record the
iteration starts from, 1 the p.w pair, 2 the record it leaves."""
import ctypes as C
import mmap
import os

import numpy as np
import pytest

import _layout_cases as LC
import _structecc as S
import _vecc
import _vecc_precond as P
from _oracle import rhs

pytestmark = pytest.mark.gpu

U = np.uint64
FIXED, DOUBLE = 14, 15
START, PAIR, NEXT = 0, 1, 2
LOOPS = ["cg", "pcg", "vecc", "pvecc"]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "abft_sparse_cg_amd", "csrc")
# the check byte (24 the parity bit), the ordinal field, word 1, the value's low bits and its three highest
SAMPLE = [24, 25, 28, 31, 0, 1, 23, 40, 64, 90, 125, 126, 127]
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
    return matrix("scaled" if loop.startswith("p") else name)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(U).copy()


class Solve:
    """one context, one matrix, b = rhs: cg_solve_device of one of the four loops, with or without the keyword"""

    def __init__(self, amd, loop, mode, mat, structure_ecc=False, capture=True):
        self.amd, self.loop = amd, loop
        self.events = []
        self.ctx = amd.HIPContext(mode, "csr", device=0,
                                  on_event=(lambda ev, fatal: self.events.extend(ev)) if capture else None)
        cols, rows, vals, n = mat
        self.n = n
        stream = structure_ecc or "vecc" in loop
        self.A = self.ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream" if stream else None,
                                        structure_ecc=structure_ecc)
        self.b, self.x, self.r, self.p, self.w = (self.ctx.create_vector(n) for _ in range(5))
        self.rhs = rhs(n, 1)
        self.dinv = None

    def run(self, **kw):
        ctx = self.ctx
        ctx.upload(self.b, self.rhs)
        ctx.upload(self.x, np.zeros(self.n))
        if self.loop.startswith("p"):
            if self.dinv is not None:
                ctx.destroy_vector(self.dinv)
            self.dinv = ctx.jacobi(self.A, protected="vecc" in self.loop)
        hist = []
        self.events.clear()
        it, rr = self.amd.cg_solve_device(ctx, self.A, self.b, self.x, self.r, self.p, self.w, precond=self.dinv,
                                          vector_ecc="vecc" in self.loop, on_iteration=lambda i, v: hist.append(v), **kw)
        return it, bits(hist), bits(ctx.download(self.x)), list(self.events)

    def close(self):
        self.ctx.close()


# ---- 1. clean parity ----

@pytest.mark.parametrize("mode", ["none", "secded"])
@pytest.mark.parametrize("loop,name", [("cg", "lap40"), ("cg", "wide5"), ("pcg", "scaled"), ("vecc", "lap40"),
                                       ("vecc", "wide5"), ("pvecc", "scaled")])
def test_clean_parity(amd, mode, loop, name):
    s = Solve(amd, loop, mode, matrix(name))
    for stride in (1, 3, 16):
        for graph in (True, False):
            kw = dict(max_itrs=35, conv_threshold=1e-9, stride=stride, graph=graph)
            it0, h0, x0, ev0 = s.run(**kw)
            it, h, x, ev = s.run(trail_ecc=True, **kw)
            assert it == it0 and it > 3, (stride, graph, it, it0)
            assert np.array_equal(h, h0) and np.array_equal(x, x0), (stride, graph)
            assert ev == ev0 == []
    s.close()


@pytest.mark.parametrize("loop", ["vecc", "pvecc"])
def test_clean_parity_with_every_protection_on(amd, loop):
    """a secded matrix, its structure, the vectors and the trail under their codes, all at once"""
    mat = matrix_of(loop)
    ref, s = Solve(amd, loop, "secded", mat), Solve(amd, loop, "secded", mat, structure_ecc=True)
    for stride, graph in ((3, True), (16, False)):
        kw = dict(max_itrs=35, conv_threshold=1e-9, stride=stride, graph=graph)
        it0, h0, x0, _ = ref.run(**kw)
        it, h, x, ev = s.run(trail_ecc=True, **kw)
        assert it == it0 and np.array_equal(h, h0) and np.array_equal(x, x0) and ev == []
    ref.close()
    s.close()


# ---- 2. every bit of every slot the device reads, between batches ----

@pytest.mark.parametrize("loop", ["cg", "pcg"])
def test_every_bit_of_the_start_record_between_batches(amd, loop):
    quad = loop == "pcg"
    rec = 4 if quad else 2  # slots per record; stride 1: record 1 starts the next batch
    s = Solve(amd, loop, "secded", matrix_of(loop))
    kw = dict(max_itrs=33, conv_threshold=0.0, stride=1, graph=True)
    it0, h0, x0, _ = s.run(trail_ecc=True, **kw)
    assert it0 == 33
    for first in range(0, 128, 32):
        state = dict(prev=None, want=[], checked=0)

        def on_batch(done, trail):
            t = s.ctx.download(trail)
            if state["prev"] is not None:  # record 0: the flipped record, its slots stored back clean
                assert np.array_equal(bits(t[:2 * rec])[[0, 1] + ([4, 5] if quad else [])], state["prev"]), done
                state["checked"] += 1
            state["prev"] = bits(t[2 * rec:4 * rec])[[0, 1] + ([4, 5] if quad else [])]
            if done <= 32:
                bit = first + done - 1
                s.ctx.flip_trail(trail, rec + 0, [bit])
                state["want"].append((FIXED, 0, bit | START << 8))
                if quad:
                    s.ctx.flip_trail(trail, rec + 2, [127 - bit])
                    state["want"].append((FIXED, 2, (127 - bit) | START << 8))

        it, h, x, ev = s.run(trail_ecc=True, on_batch=on_batch, **kw)
        assert it == it0 and np.array_equal(h, h0) and np.array_equal(x, x0), first
        assert ev == state["want"] and len(ev) == (64 if quad else 32), (first, ev, state["want"])
        assert state["checked"] == 32
    s.close()


@pytest.mark.parametrize("loop", ["cg", "pcg"])
def test_words_the_device_does_not_read_are_reported_by_the_host_decode(amd, loop):
    quad = loop == "pcg"
    rec = 4 if quad else 2
    s = Solve(amd, loop, "secded", matrix_of(loop))
    kw = dict(max_itrs=12, conv_threshold=0.0, stride=3, graph=True)
    it0, h0, x0, _ = s.run(trail_ecc=True, **kw)
    want = []

    def on_batch(done, trail):
        if done in (3, 6):  # record `stride`: its events word, and the trailing word of a quad
            bit = 24 if done == 3 else 101
            s.ctx.flip_trail(trail, rec * 3 + 1, [bit])
            want.append((FIXED, 1, bit | START << 8))
            if quad:
                s.ctx.flip_trail(trail, rec * 3 + 3, [bit + 1])
                want.append((FIXED, 3, (bit + 1) | START << 8))

    it, h, x, ev = s.run(trail_ecc=True, on_batch=on_batch, **kw)
    assert it == it0 and np.array_equal(h, h0) and np.array_equal(x, x0)
    assert ev == want and len(ev) == (4 if quad else 2), (ev, want)  # each exactly once
    s.close()


# ---- the C entries, one iteration at a time ----

class Iter:
    """x, r, p, w (dinv) and the slots {start record | p.w pair | next record} of one guarded iteration"""

    def __init__(self, amd, loop, mode="secded", mat=None, seed=1):
        self.loop, self.quad, self.vecc = loop, loop.startswith("p"), "vecc" in loop
        self.rec = 4 if self.quad else 2
        self.IN, self.PW, self.OUT = 0, 2 * self.rec, 2 * self.rec + 4  # in doubles
        self.events = []
        self.ctx = amd.HIPContext(mode, "csr", device=0, on_event=lambda ev, fatal: self.events.extend(ev))
        cols, rows, vals, n = mat or matrix_of(loop)
        self.n = n
        self.A = self.ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        rng = np.random.default_rng(seed)
        vals0 = [rng.standard_normal(n) for _ in range(3)] + [np.full(n, 7.5)]
        self.start = [bits(_vecc.encode(v).view(np.float64)) if self.vecc else bits(v) for v in vals0]
        self.x, self.r, self.p, self.w = (self.ctx.create_vector(n) for _ in range(4))
        self.dinv = self.ctx.jacobi(self.A, protected=self.vecc) if self.quad else None
        self.sc = self.ctx.create_vector(4 * self.rec + 8)  # (four doubles to spare: the refusal test's layouts)
        fn = dict(cg=self.ctx.cg_trail_iteration_until_dev, pcg=self.ctx.pcg_trail_iteration_until_dev,
                  vecc=self.ctx.cg_vecc_trail_iteration_until_dev, pvecc=self.ctx.pcg_vecc_trail_iteration_until_dev)[loop]
        self.fn = fn

    def reset(self, rr, rz=None):
        for v, a in zip((self.x, self.r, self.p, self.w), self.start):
            self.ctx.upload(v, a.view(np.float64))
        record = [rr, 0.0] + ([rz, 0.0] if self.quad else [])
        start = np.zeros(4 * self.rec + 8)
        start[:2 * self.rec] = self.ctx.encode_trail(record)
        self.ctx.upload(self.sc, start)
        self.events.clear()

    def until(self, thr, at=None):
        IN, PW, OUT = at or (self.IN, self.PW, self.OUT)
        args = [self.A, self.p, self.x, self.r, self.p, self.w] + ([self.dinv] if self.quad else []) + [self.sc, IN, PW, OUT, thr]
        self.fn(*args)

    def state(self):
        """-> (words of x, r, p, w, the raw slots); the download drains the events"""
        vecs = [bits(self.ctx.download(v)) for v in (self.x, self.r, self.p, self.w)]
        return vecs, bits(self.ctx.download(self.sc))

    def close(self):
        self.ctx.close()


def seeds(quad):
    return (3.25, 2.75) if quad else (3.25,)


@pytest.mark.parametrize("loop", LOOPS)
def test_slots_that_live_inside_an_iteration(amd, loop):
    """trail_inject_at, stage 1 (behind the fold) and stage 2 (behind the r half): the outputs of a clean twin, and
    one event each, from the launch that met the flip"""
    it, twin = Iter(amd, loop), Iter(amd, loop)
    twin.reset(*seeds(twin.quad))
    twin.until(0.0)
    want_v, want_sc = twin.state()
    assert twin.events == []
    values = twin.ctx.decode_trail(want_sc.view(np.float64))
    assert not values[1].any()
    rz = 2 if it.quad else 0
    places = [(1, PAIR, 0), (1, START, 0), (2, START, 0), (2, PAIR, 0), (2, NEXT, rz)] + ([(1, START, 2), (2, START, 2)] if it.quad else [])
    for stage, record, ordinal in places:
        for bit in SAMPLE:
            it.reset(*seeds(it.quad))
            it.ctx.trail_inject_at(stage, record, ordinal, [bit])
            it.until(0.0)
            got_v, got_sc = it.state()
            for name, g, w in zip("xrpw", got_v, want_v):
                assert np.array_equal(g, w), (stage, record, ordinal, bit, name)
            # every slot read was stored back clean, every slot written is a fresh encode: the twin's slots, but for
            # the events words, which count the one queued event from the launch that met it on
            v, st, _ = it.ctx.decode_trail(got_sc.view(np.float64))
            assert not st.any(), (stage, record, ordinal, bit)
            ev_words = [1, it.rec + 1, it.rec + 2 + 1]
            keep = [k for k in range(len(v)) if k not in ev_words]
            assert np.array_equal(bits(v)[keep], bits(values[0])[keep]), (stage, record, ordinal, bit)
            assert it.events == [(FIXED, ordinal, bit | record << 8)], (stage, record, ordinal, bit, it.events)
    # the injection is one shot: the next call is clean
    it.reset(*seeds(it.quad))
    it.until(0.0)
    assert np.array_equal(it.state()[1], want_sc) and it.events == []
    it.close()
    twin.close()


# ---- 4. a frozen launch ----

@pytest.mark.parametrize("loop", LOOPS)
def test_frozen_launch_hands_on_the_repaired_value_reencoded(amd, loop):
    it = Iter(amd, loop)
    nan, neg0 = float(np.array([0x7FF8000000ABCDEF], U).view(np.float64)[0]), -0.0
    for rr, rz, thr, slot, bit in ((3.25, 2.75, 3.25, 0, 127), (3.25, 2.75, np.inf, 0, 24), (nan, neg0, 0.0, 0, 70),
                                   (neg0, nan, 0.0, 2 if it.quad else 0, 66)):
        it.reset(rr, rz)
        it.ctx.flip_trail(it.sc, slot, [bit])
        it.until(thr)
        got_v, sc = it.state()
        for name, g, w in zip("xrp", got_v, it.start):  # (w is the SpMV's, which always runs)
            assert np.array_equal(g, w), (rr, thr, name)
        v, st, _ = it.ctx.decode_trail(sc.view(np.float64))
        assert not st.any()  # the start record stored back clean, the next one freshly encoded
        out = it.rec + 2
        assert bits([v[out]])[0] == bits([rr])[0] and bits([v[0]])[0] == bits([rr])[0]  # moved as integers: payload, -0.0
        if it.quad:
            assert bits([v[out + 2]])[0] == bits([rz])[0] and bits([v[out + 3]])[0] == 0
        assert v[out + 1] == 1.0  # the queued-event count, this launch's own event included
        assert it.events == [(FIXED, slot, bit | START << 8)], it.events
    it.close()


# ---- 5. double flips ----

def vectors(s):
    return [bits(s.ctx.download(v)) for v in (s.x, s.r, s.p)]


@pytest.mark.parametrize("loop,what", [("cg", "rr"), ("pcg", "rr"), ("pcg", "rz"), ("cg", "pw"), ("pcg", "pw"),
                                       ("cg", "next"), ("pcg", "next")])
def test_double_flips_are_fatal_at_that_batchs_download(amd, loop, what):
    quad = loop == "pcg"
    rec = 4 if quad else 2
    mat = matrix_of(loop)
    twin = Solve(amd, loop, "secded", mat)
    twin.run(trail_ecc=True, max_itrs=4, conv_threshold=0.0, stride=1, graph=False)
    want = vectors(twin)
    twin.close()
    s = Solve(amd, loop, "secded", mat, capture=False)
    called = []
    ordinal = dict(rr=0, rz=2, pw=0, next=2 if quad else 0)[what]
    record = dict(rr=START, rz=START, pw=PAIR, next=NEXT)[what]

    def on_batch(done, trail):
        called.append(done)
        if done == 4:
            if what in ("rr", "rz"):
                s.ctx.flip_trail(trail, rec + ordinal, [3, 99])
            else:
                s.ctx.trail_inject_at(1 if what == "pw" else 2, record, ordinal, [3, 99])

    live = []
    with pytest.raises(amd.FatalEvent) as e:
        s.ctx.upload(s.b, s.rhs)
        s.ctx.upload(s.x, np.zeros(s.n))
        if quad:
            s.dinv = s.ctx.jacobi(s.A)
        amd.cg_solve_device(s.ctx, s.A, s.b, s.x, s.r, s.p, s.w, max_itrs=20, conv_threshold=0.0, stride=1, graph=False,
                            precond=s.dinv, trail_ecc=True, on_batch=on_batch, on_iteration=lambda i, v: live.append(i))
    assert (DOUBLE, ordinal, record << 8) in e.value.events, e.value.events
    assert e.value.events[-1][0] == DOUBLE  # nothing is handed over behind the fatal line
    assert called == [1, 2, 3, 4] and live == [0, 1, 2, 3]  # raised before any callback of that batch
    if what != "next":  # x, r and p keep every bit from that r half on
        for name, g, w in zip("xrp", vectors(s), want):
            assert np.array_equal(g, w), (what, name)
    s.close()


# ---- 6. the multi-workgroup fold ----

def planned_blocks(tmp, n):
    """the row blocks the planner (csrc/layout_plan.h) cuts the diagonal matrix of n rows into, in mode none, streaming:
    tests/host/layout_plan_play.cpp run on the host, on its `uniform N 1 0` matrix (element r of row r: 4.0 on an even
    column, -1.0 on an odd one)"""
    import re
    import subprocess

    def define(name, where="abft_internal.h"):
        with open(os.path.join(CSRC, where)) as f:
            return "-D%s=%s" % (name, re.search(r"#define\s+%s\s+(\w+)" % name, f.read()).group(1))
    exe = os.path.join(str(tmp), "layout_plan_play")
    subprocess.run(["g++", "-std=c++17", "-O1", define("ABFT_PAL_ENTRIES"), define("ABFT_CBASE_WIDE"),
                    define("ABFT_PAL_SPARE", "abft_hip.hip"), "-I", CSRC,
                    os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "layout_plan_play.cpp"), "-o", exe], check=True)
    case = LC.case("diag", "uniform %d 1 0" % n, mode=LC.NONE, stream=True)
    p = subprocess.run([exe], input=LC.text_of([case], LC.geometry(CSRC)), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    name, fields = LC.parse(p.stdout.splitlines()[0])
    assert name == "diag" and fields["layout"] == "0"  # the streaming layout
    return int(fields["blk"].split(":")[0])


def test_multi_workgroup_fold_publishes_slots(amd, tmp_path):
    """more than 8192 partials: a diagonal matrix of 8192 * 1024 + 1 rows, whose block count the planner itself gives on
    the host.  Three iterations at stride 3 against the unprotected twin, one p.w flip repaired on the way"""
    n = 8192 * 1024 + 1
    assert planned_blocks(tmp_path, n) > 8192  # fuse_finalize_folds: the multi-workgroup fold
    idx = np.arange(n, dtype=np.uint32)
    vals = np.where(idx % 2 == 1, -1.0, 4.0)  # the matrix that was planned
    ctx = amd.HIPContext("none", "csr", device=0, on_event=lambda ev, fatal: events.extend(ev))
    events = []
    A = ctx.create_matrix(idx, idx, vals, n, n, layout="stream")
    b, x, r, p, w = (ctx.create_vector(n) for _ in range(5))
    rhs_ = 1.0 + (idx % 5).astype(np.float64)
    out = []
    for trail in (False, True):
        ctx.upload(b, rhs_)
        ctx.upload(x, np.zeros(n))
        hist = []
        if trail:
            ctx.trail_inject_at(1, PAIR, 0, [77])
        it, rr = amd.cg_solve_device(ctx, A, b, x, r, p, w, max_itrs=3, conv_threshold=0.0, stride=3, graph=False,
                                     on_iteration=lambda i, v: hist.append(v), trail_ecc=trail)
        out.append((it, bits(hist), bits(ctx.download(x))))
    assert out[0][0] == out[1][0] == 3
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert events == [(FIXED, 0, 77 | PAIR << 8)], events
    ctx.close()


# ---- 7. refusals ----

def test_refusals(amd):
    from abft_sparse_cg_amd import capi
    s = Solve(amd, "cg", "none", matrix("lap40"))
    with pytest.raises(ValueError, match="check_every"):
        s.run(trail_ecc=True, check_every=5)
    s.close()
    it = Iter(amd, "cg", "none")
    it.reset(3.25)
    before = it.state()
    with pytest.raises(capi.AbftError, match="overlap"):  # records that overlap: the pair inside the next record
        it.until(0.0, at=(0, 6, 4))
    with pytest.raises(capi.AbftError, match="16-byte"):
        it.until(0.0, at=(0, 5, 10))
    it.ctx.trail_inject_at(1, PAIR, 0, [5])
    it.ctx.graph_begin()
    try:
        with pytest.raises(capi.AbftError, match="injection armed"):
            it.until(0.0)
    finally:
        g = it.ctx.graph_end()
    it.ctx.graph_destroy(g)
    it.ctx.trail_inject_at(1, PAIR, 0, [])  # disarmed
    # a slot the entry's records do not have: refused with the other refusals, nothing enqueued, nothing written
    for record, ordinal in ((PAIR, 2), (PAIR, 3), (START, 2), (NEXT, 3)):
        it.ctx.trail_inject_at(2, record, ordinal, [5])
        with pytest.raises(capi.AbftError, match="armed trail injection names word %d" % ordinal):
            it.until(0.0)
    it.ctx.trail_inject_at(1, PAIR, 0, [])
    with pytest.raises(capi.AbftError, match="ordinal 4"):
        it.ctx.trail_inject_at(1, START, 4, [5])
    quad = Iter(amd, "pcg", "none")
    quad.reset(3.25, 2.75)
    clean = quad.state()
    quad.ctx.trail_inject_at(1, PAIR, 2, [5])
    with pytest.raises(capi.AbftError, match="names word 2 of a record of 2 words"):
        quad.until(0.0)
    quad.ctx.trail_inject_at(1, START, 3, [5])  # a record of four words has it
    quad.until(0.0)
    got = quad.state()
    assert quad.events == []  # (the trailing word: no launch reads it)
    assert np.array_equal(got[1][-4:], clean[1][-4:])  # the doubles behind the next record: untouched
    quad.close()
    board = mmap.mmap(-1, it.ctx.L.abft_hip_peer_board_bytes())
    capi.check(it.ctx.L.abft_hip_peer_board_attach(it.ctx.h, C.addressof(C.c_char.from_buffer(board)), len(board), 0, 1, 5.0))
    try:
        with pytest.raises(capi.AbftError, match="peer board"):
            it.until(0.0)
    finally:
        capi.check(it.ctx.L.abft_hip_peer_board_detach(it.ctx.h))
    after = it.state()
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and np.array_equal(before[1], after[1])
    assert it.events == []
    it.until(0.0)  # and the entry still works
    assert not it.ctx.decode_trail(it.state()[1].view(np.float64))[1].any()
    it.close()


# ---- 7. the command line ----

def cli(args):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mtx = os.path.join(root, "tests", "golden", "lap64.mtx")
    return subprocess.run([sys.executable, "-m", "abft_sparse_cg_amd.cg", "-t", "hip", "-f", mtx, "-b", "1"] + args,
                          capture_output=True, text=True, timeout=300, cwd=root)


def test_cli_protects_the_trail_and_flips_it():
    base = cli(["--device-loop", "4", "-i", "12", "-c", "0"])
    assert base.returncode == 0 and "scalar trail" not in base.stdout and "trail word" not in base.stdout
    refused = cli(["--trail-ecc", "secded"])
    assert refused.returncode == 1 and "--trail-ecc" in refused.stdout and "--device-loop" in refused.stdout
    on = cli(["--device-loop", "4", "--trail-ecc", "secded", "-i", "12", "-c", "0"])
    assert on.returncode == 0, on.stderr
    lines = on.stdout.splitlines()
    at = lines.index("iteration loop: device scalars, stride 4")
    assert lines[at + 1] == "scalar trail: secded (128, 120)"
    rr = lambda out: [l for l in out.splitlines() if l.startswith("iteration ") and "rr =" in l]
    assert rr(on.stdout) == rr(base.stdout) and len(rr(on.stdout)) == 12
    # without the flags the output is unchanged but for the one line; with a flip, the rr lines are the clean run's
    strip = lambda out: [l for l in out.splitlines() if not l.startswith(("scalar trail", "time taken"))]
    assert strip(on.stdout) == strip(base.stdout)
    hit = cli(["--device-loop", "4", "--trail-ecc", "secded", "-i", "12", "-c", "0", "--flip-trail", "3:0:77",
               "--flip-trail", "7:1:24"])
    assert hit.returncode == 0, hit.stderr
    assert rr(hit.stdout) == rr(base.stdout)
    assert hit.stdout.count("[ECC] corrected bit 77 of trail word 0 (start record)") == 1
    assert hit.stdout.count("[ECC] corrected bit 24 of trail word 1 (start record)") == 1
    assert hit.stdout.count("trail word") == 2


def test_a_codeword_in_the_wrong_place_is_as_two_flips(amd):
    """the ordinal is under the code and compared with the place: r.r's slot holding a clean codeword of ordinal 1 is
    fatal on the device, x, r and p untouched; the host's decode says the same of a downloaded trail"""
    it = Iter(amd, "cg")
    it.reset(3.25)
    sc = it.ctx.download(it.sc)
    sc[0:2] = it.ctx.encode_trail([3.25], 1)
    it.ctx.upload(it.sc, sc)
    it.until(0.0)
    got_v, got_sc = it.state()
    for name, g, w in zip("xrp", got_v, it.start):
        assert np.array_equal(g, w), name
    assert it.events and set(it.events) == {(DOUBLE, 0, START << 8)}, it.events
    assert np.array_equal(got_sc[it.OUT:it.OUT + 4], got_sc[0:4])  # handed on word for word
    good = np.concatenate([it.ctx.encode_trail([1.0, 0.0])] * 2 + [it.ctx.encode_trail([2.0, 0.0])])
    assert np.array_equal(it.ctx.report_trail(good, 2, 1), [1.0, 0.0, 1.0, 0.0, 2.0, 0.0])
    bad = good.copy()
    bad[6:8] = it.ctx.encode_trail([0.0], 0)  # record 1's events word under ordinal 0
    del it.events[:]
    with pytest.raises(amd.FatalEvent):
        it.ctx.report_trail(bad, 2, 1)
    assert it.events == [(DOUBLE, 1, START << 8)]
    it.close()
