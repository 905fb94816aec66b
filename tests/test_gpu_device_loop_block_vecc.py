"""The device-resident block loop on protected vectors: abft_hip_cg_block_vecc_iteration_until_dev (the guarded block
iteration on codewords) and cg_solve_block_device(vector_ecc=True) on top of it.

The yardstick of a launch with a live column is the sequence of host-scalar protected calls it stands for, run on
copies -- abft_hip_spmm_dot_vecc, alpha = r.z / P.W in numpy float64, abft_hip_calc_r_block_vecc, beta = r.r' / r.z,
abft_hip_calc_px_block_vecc, all with the mask the device forms --: the same words in X, R, P, W, P.W and the record.
A frozen column is held against its definition: its column keeps every bit (repaired where a word was flipped and
another column is live), its record words are handed on.  cg_solve_block_device(vector_ecc=True) is held against
itself over every stride and graph setting (bit for bit) and against cg_solve_block(vector_ecc=True) (the same counts,
histories within the README's 1e-10).

A flip in W cannot be planted through the entry: the SpMM of the same call rewrites every word of W before the r half
reads it.  The ordinal the r half reports W under (4) is a constant at its one call site; the walk that takes it is
the one test_gpu_block_vecc.py flips W under (there as operand 1)."""
import math

import numpy as np
import pytest

import _vecc
import _vecc_block as B
import _devloop_block_vecc as D
from _oracle import laplace5, rhs
from test_gpu_block_vecc import CASES, FK, FN
from test_gpu_device_loop_block import SCALES
from test_gpu_devloop import tri
from test_gpu_vector_ecc import Box

pytestmark = pytest.mark.gpu

U = np.uint64
CORRECTED, DOUBLE = 10, 11
ERR_INVALID = -1
PAYLOAD = np.array([0x7FF8000000ABCDEF, 0xFFF0000000000123, 0x7FF4000000000001], dtype=U).view(np.float64)
NAMES = ("X", "R", "P", "W")


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def quot(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


class VDev:
    """one context (a Box: its events are collected): a matrix, the block vectors X R P W holding codewords, and the
    scalars: record A at 0, record B at 2k + 2, {P.W[k], events} at 2 (2k + 2)"""

    def __init__(self, amd, mat, k, mode="none", fmt="csr", layout="stream"):
        self.amd, self.box = amd, Box(amd, mode, fmt)
        self.ctx = ctx = self.box.ctx
        cols, rows, vals, n = mat
        self.n, self.k, self.rec = n, k, 2 * k + 2
        self.A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout=layout)
        self.v = {name: ctx.create_block(n, k) for name in NAMES}
        self.pw_at = 2 * self.rec
        self.sc = ctx.create_vector(self.pw_at + k + 1)

    def load(self, blocks, rec):
        """the words of `blocks` (name -> (N, k) uint64); record A = the 2k doubles of `rec` and {0, 0}, the rest 9.0"""
        for name in NAMES:
            self.ctx.upload(self.v[name], B.flat(blocks[name]).view(np.float64))
        sc = np.full(self.pw_at + self.k + 1, 9.0)
        sc[0:2 * self.k] = rec
        sc[2 * self.k:self.rec] = 0.0
        self.ctx.upload(self.sc, sc)

    def words(self):
        out = {name: B.block(self.ctx.download(self.v[name]).view(U), self.k) for name in NAMES}
        out["sc"] = self.ctx.download(self.sc).view(U).copy()
        return out

    def vecs(self):
        return [self.v[name] for name in NAMES]

    def until(self, thr, at=None):
        at = at or (0, self.pw_at, self.rec)
        self.ctx.cg_block_vecc_iteration_until_dev(self.A, *self.vecs(), self.k, self.sc, at[0], at[1], at[2], thr)

    def raw(self, thr, vecs=None, k=None, at=None, A="own"):
        """the C entry itself, addresses in doubles from the scalars' start (None: a null pointer) -> the return code"""
        base = self.sc.device_ptr
        at = at or (0, self.pw_at, self.rec)
        ptrs = [None if a is None else base + 8 * a for a in at]
        h = lambda v: v.h if v is not None else None
        X, R, P, W = vecs or self.vecs()
        return self.ctx.L.abft_hip_cg_block_vecc_iteration_until_dev(
            self.ctx.h, h(self.A if A == "own" else A), h(X), h(R), h(P), h(W), self.k if k is None else k, *ptrs, thr)

    def host(self, rec, active):
        """the iteration as the three host-scalar protected calls with the mask `active` -> (pw[k], rr_new[k])"""
        ctx, k, v = self.ctx, self.k, self.v
        on = [(active >> j) & 1 for j in range(k)]
        pw = ctx.spmm_dot_vecc(self.A, v["P"], v["W"], k)
        alpha = [quot(rec[k + j], pw[j]) if on[j] else 0.0 for j in range(k)]
        rr_new = ctx.calc_r_block_vecc(v["R"], v["W"], k, alpha, active)
        beta = [quot(rr_new[j], rec[k + j]) if on[j] else 0.0 for j in range(k)]
        ctx.calc_px_block_vecc(v["X"], v["P"], v["R"], k, alpha, beta, active)
        return np.array(pw), np.array(rr_new)

    def close(self):
        self.ctx.close()


def record_of(k):
    """r.r spread over magnitudes, r.z another number: the quotients take r.z, the mask r.r"""
    rr = np.array([SCALES[(j + 1) % 4] * (1.0 + j / 16.0) for j in range(k)])
    return np.concatenate([rr, 0.75 * rr + 0.03125])


def check_launch(dev, blocks, rec, thr, what):
    """one launch against the host-scalar calls on the same start: every word equal"""
    k, r = dev.k, dev.rec
    mask = D.live_mask(rec[:k], thr)
    assert mask, what
    dev.load(blocks, rec)
    pw, rr_new = dev.host(rec, mask)
    want = dev.words()
    assert dev.box.take() == [], what
    dev.load(blocks, rec)
    dev.until(thr)
    got = dev.words()
    for name in NAMES:
        assert np.array_equal(got[name], want[name]), (what, name)
    sc = got["sc"]
    assert np.array_equal(sc[0:r], want["sc"][0:r]), what  # what it read: left alone
    assert np.array_equal(sc[dev.pw_at:dev.pw_at + k], D.bits(pw)), (what, sc[dev.pw_at:], pw)
    for j in range(k):
        if (mask >> j) & 1:
            assert sc[r + j] == sc[r + k + j] == D.bits(rr_new[j:j + 1])[0], (what, j)
        else:
            assert sc[r + j] == D.bits(rec)[j] and sc[r + k + j] == D.bits(rec)[k + j], (what, j)
            for name in ("X", "R", "P"):  # clean words: every bit kept
                assert np.array_equal(got[name][:, j], blocks[name][:, j]), (what, name, j)
    assert np.array_equal(sc[r + 2 * k:2 * r], D.bits([0.0, 0.0])) and sc[dev.pw_at + k] == 0, what
    assert dev.box.take() == [], what
    return mask


def live_case(amd, n, k, mode="none"):
    dev = VDev(amd, tri(n), k, mode)
    try:
        rec = record_of(k)
        salted = {name: B.block(_vecc.family("finite", n * k, _vecc.operand_seed(n * k, c)), k)
                  for c, name in enumerate(NAMES)}
        rng = np.random.default_rng(1000 * n + k)
        plain = {name: B.block(_vecc.encode(rng.standard_normal(n * k)), k) for name in NAMES}
        full = (1 << k) - 1
        mixed = check_launch(dev, salted, rec, 2.0 if k > 1 else 0.5, (n, k, mode, "salted"))
        assert check_launch(dev, plain, rec, 0.0, (n, k, mode, "all live")) == full
        assert check_launch(dev, plain, rec, 2.0 if k > 1 else 0.5, (n, k, mode, "mixed")) == mixed
        assert k == 1 or mixed != full
    finally:
        dev.close()


# -------------------------------------------------- 1. a live launch == the three host-scalar protected calls --

@pytest.mark.parametrize("mode", ["none", "secded"])
@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("n", [1, 2, 255, 257, 2049, 6145])
def test_live_launch_is_the_three_host_scalar_protected_calls(amd, n, k, mode):
    live_case(amd, n, k, mode)


@pytest.mark.parametrize("k", [1, 2, 4, 5, 6, 7])
def test_every_k(amd, k):
    live_case(amd, 257, k)


def test_more_than_32_workgroups(amd):
    live_case(amd, _vecc.MANY_N, 2)


# ------------------------------------------------------------------- 2. every mask --
THR = 0.1 + 0.2


def mask_record(mask, k=3):
    """exactly the columns of `mask` above THR; the others hold NaN, a payload NaN and the threshold itself"""
    cold_rr, cold_rz = [math.nan, PAYLOAD[0], THR], [PAYLOAD[1], PAYLOAD[2], -0.0]
    rr = np.array([2.0 + j if (mask >> j) & 1 else cold_rr[j] for j in range(k)])
    rz = np.array([1.5 + j if (mask >> j) & 1 else cold_rz[j] for j in range(k)])
    return np.concatenate([rr, rz])


@pytest.mark.parametrize("mode", ["none", "secded"])
@pytest.mark.parametrize("mask", range(1, 8))
def test_every_mask_with_a_live_column(amd, mask, mode):
    n, k = 257, 3
    dev = VDev(amd, tri(n), k, mode)
    try:
        rng = np.random.default_rng(mask)
        blocks = {name: B.block(_vecc.encode(rng.standard_normal(n * k)), k) for name in NAMES}
        rec = mask_record(mask)
        assert check_launch(dev, blocks, rec, THR, (mask, mode)) == mask
        got = dev.words()
        for j in range(k):
            if (mask >> j) & 1:
                assert not np.array_equal(got["X"][:, j], blocks["X"][:, j]), j  # it ran
    finally:
        dev.close()


def test_no_column_live_keeps_every_word_and_hands_the_record_on(amd):
    n, k = 257, 3
    dev = VDev(amd, tri(n), k, "secded")
    try:
        rng = np.random.default_rng(8)
        blocks = {name: B.block(_vecc.encode(rng.standard_normal(n * k)), k) for name in NAMES}
        rec = mask_record(0)
        dev.load(blocks, rec)
        flips = {"X": (100 * k + 1, 12), "R": (7 * k + 0, 0), "P": (128 * k + 2, 55)}  # one flipped word in each
        for name, (index, bit) in flips.items():
            dev.ctx.flip_vector(dev.v[name], index, [bit])
        pre = dev.words()
        assert all(not np.array_equal(pre[name], blocks[name]) for name in "XRP")
        r = dev.rec
        for launch in range(2):  # a second launch changes nothing
            dev.until(THR)
            got = dev.words()
            for name in "XRP":
                assert np.array_equal(got[name], pre[name]), (launch, name)  # the flipped words included
            sc = got["sc"]
            assert np.array_equal(sc[0:r], pre["sc"][0:r])
            assert np.array_equal(sc[r:r + 2 * k], D.bits(rec)), launch  # NaN payloads intact
            # the SpMM ran: its gather met the flip in P and reported it (operand 0); the two vector kernels report
            # nothing, and the record's event word counts that one queued event
            assert sc[r + 2 * k:2 * r].view(np.float64).tolist() == [1.0, 0.0], (launch, sc)
            assert dev.box.take() == [(CORRECTED, flips["P"][0], flips["P"][1])], launch
    finally:
        dev.close()


def test_infinite_rr_above_a_finite_threshold_is_live_and_a_nan_is_frozen(amd):
    n, k, thr = 257, 3, 1e300
    dev = VDev(amd, tri(n), k)
    try:
        rng = np.random.default_rng(9)
        blocks = {name: B.block(_vecc.encode(rng.standard_normal(n * k)), k) for name in NAMES}
        rec = np.concatenate([[PAYLOAD[0], math.inf, 5.0], [PAYLOAD[1], 4.0, 3.0]])
        assert check_launch(dev, blocks, rec, thr, "inf") == 0b010
        got = dev.words()
        assert not np.array_equal(got["X"][:, 1], blocks["X"][:, 1])  # it ran
    finally:
        dev.close()


# ------------------------------------------------------------------------ 3. flips --
# the flip fixture of test_gpu_block_vecc.py: 4099 rows, K = 3, columns 0 and 2 live, column 1 frozen
FMASK, FTHR = 0b101, 0.5
FREC = np.array([2.0, 0.25, 3.0, 1.5, 0.125, 2.5])
# operand -> the ordinals a flipped word of it is reported under, in the order of the kernels: the gather of the SpMM
# (P only: 0), the r half (R: 2), the x / p half (X: 1, P: 3; R is clean again by then)
ORDINALS = {"X": [1], "R": [2], "P": [0, 3]}


@pytest.fixture(scope="module")
def flip_clean(amd):
    rng = np.random.default_rng(FN)
    blocks = {name: B.block(_vecc.encode(rng.standard_normal(FN * FK)), FK) for name in NAMES}
    dev = VDev(amd, tri(FN), FK)
    try:
        assert D.live_mask(FREC[:FK], FTHR) == FMASK
        dev.load(blocks, FREC)
        dev.until(FTHR)
        clean = dev.words()
        assert dev.box.take() == []
    finally:
        dev.close()
    return blocks, clean


@pytest.mark.parametrize("op", ["X", "R", "P"])
def test_flips_in_a_live_and_in_a_frozen_column_leave_the_clean_launchs_words(amd, flip_clean, op):
    blocks, clean = flip_clean
    dev = VDev(amd, tri(FN), FK)
    try:
        for flips in CASES:
            dev.load(blocks, FREC)
            events = []
            for i, j, bits in flips:
                dev.ctx.flip_vector(dev.v[op], i * FK + j, bits)
                events += [(CORRECTED, i * FK + j, b | o << 8) for b in bits for o in ORDINALS[op]]
            dev.until(FTHR)
            got = dev.words()
            for name in NAMES:  # the frozen column's word is repaired in memory: X, R and P are all written
                assert np.array_equal(got[name], clean[name]), (op, flips, name)
            r = dev.rec
            assert np.array_equal(got["sc"][r:r + 2 * FK], clean["sc"][r:r + 2 * FK]), (op, flips)
            assert np.array_equal(got["sc"][dev.pw_at:dev.pw_at + FK], clean["sc"][dev.pw_at:dev.pw_at + FK])
            assert sorted(dev.box.take()) == sorted(events), (op, flips)
    finally:
        dev.close()


def test_no_column_live_and_a_flipped_word_in_r_no_event_and_the_word_stays(amd, flip_clean):
    blocks, _ = flip_clean
    dev = VDev(amd, tri(FN), FK)
    try:
        dev.load(blocks, FREC)
        dev.ctx.flip_vector(dev.v["R"], 1536 * FK + 2, [52])
        pre = dev.words()
        dev.until(5.0)  # above every r.r
        got = dev.words()
        for name in "XRP":
            assert np.array_equal(got[name], pre[name]), name
        assert got["R"][1536, 2] == blocks["R"][1536, 2] ^ U(1 << 52)
        assert dev.box.take() == []
    finally:
        dev.close()


# ------------------------------------------------------------------------ 5. the solver --
SK, ROW = 4, 200
COUNTS = {1e-3: [59, 60, 63, 64], 1e-10: [107, 108, 108, 108]}


class Solver:
    """laplace5:40,40, column j with rhs(n, 1 + j), on one context; every run starts from X = 0 and a fresh B"""

    def __init__(self, amd, collect=True):
        self.amd = amd
        cols, rows, vals, n = laplace5(40, 40)
        self.n, self.events = n, []
        self.B0 = np.stack([rhs(n, 1 + j) for j in range(SK)], axis=1)
        self.ctx = ctx = amd.HIPContext("secded", "csr",
                                        on_event=(lambda ev, fatal: self.events.extend(ev)) if collect else None)
        self.A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        self.v = dict(zip("BXRPW", (ctx.create_block(n, SK) for _ in range(5))))

    def run(self, thr, stride=None, graph=True, flip=None, on_iteration=None):
        """stride None: cg_solve_block(vector_ecc=True); else cg_solve_block_device(vector_ecc=True).  flip: (block name,
        index, bits, iteration): planted from the callback of that iteration -- between batches
        -> (itrs, rr, history, masks, X as downloaded, events)"""
        ctx, v = self.ctx, self.v
        ctx.upload(v["B"], self.B0)
        ctx.upload(v["X"], np.zeros((self.n, SK)))
        hist, masks, self.events = [], [], []

        def cb(i, rr, active):
            assert i == len(hist)
            hist.append(rr)
            masks.append(active)
            if flip and i == flip[3]:
                ctx.flip_vector(v[flip[0]], flip[1], flip[2])
            if on_iteration:
                on_iteration(i)
        vecs = [v[name] for name in "BXRPW"]
        if stride is None:
            itrs, rr = self.amd.cg_solve_block(ctx, self.A, *vecs, 1000, thr, on_iteration=cb, vector_ecc=True)
        else:
            itrs, rr = self.amd.cg_solve_block_device(ctx, self.A, *vecs, 1000, thr, on_iteration=cb, stride=stride,
                                                      graph=graph, vector_ecc=True)
        return list(itrs), rr, hist, masks, ctx.download(v["X"]), list(self.events)

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def solver(amd):
    s = Solver(amd)
    yield s
    s.close()


@pytest.fixture(scope="module")
def host_solves(solver):
    return {thr: solver.run(thr) for thr in COUNTS}


def same_run(a, b):
    return a[0] == b[0] and np.array_equal(D.bits(np.array(a[2])), D.bits(np.array(b[2]))) and a[3] == b[3] and \
        np.array_equal(a[4].view(U), b[4].view(U)) and np.array_equal(D.bits(a[1]), D.bits(b[1]))


@pytest.mark.parametrize("thr", sorted(COUNTS))
def test_protected_block_device_solve_agrees_with_itself_and_the_protected_host_loop(solver, host_solves, thr):
    from abft_sparse_cg_amd.context import vecc_strip
    itrs_h, rr_h, hist_h, masks_h, x_h, ev_h = host_solves[thr]
    assert itrs_h == COUNTS[thr] and ev_h == []
    runs = [solver.run(thr, stride, graph) for stride in (1, 3, 16) for graph in (True, False)]
    for run in runs:
        itrs, rr, hist, masks, x, events = run
        assert itrs == itrs_h and len(hist) == len(hist_h) == max(itrs_h), (itrs, itrs_h)
        assert masks == masks_h and events == []
        assert same_run(run, runs[0])  # itrs, rr history and the downloaded X words, bit for bit
        err = float(np.max(np.abs(np.array(hist) - np.array(hist_h)) / np.abs(np.array(hist_h))))
        assert err <= 1e-10, err
        assert np.array_equal(D.bits(rr), D.bits(hist[-1]))
        assert not _vecc.decode(x.view(U))[1].any()  # what the caller downloads are codewords
    same = np.array_equal(D.bits(np.array(runs[0][2])), D.bits(np.array(hist_h))) and \
        np.array_equal(vecc_strip(runs[0][4]).view(U), vecc_strip(x_h).view(U))
    print("   thr %g: counts %s; device loop %s cg_solve_block(vector_ecc=True) bit for bit" %
          (thr, itrs_h, "==" if same else "!="))
    if thr == 1e-3:
        # columns stop at different iterations inside one replayed graph: the batch of iterations 48 .. 63 at stride 16
        assert len(set(masks_h[48:64])) >= 3 and all(47 < c <= 64 for c in itrs_h), (itrs_h, masks_h[48:64])


FLIP_AT = 9  # the last iteration of the second batch of five: the third batch meets the flip
AT = ROW * SK + 3  # column 3 runs longest
# (block, index, bit, the callback that plants it, threshold) -> the ordinals it is reported under
SOLVER_FLIPS = [("P", AT, 55, FLIP_AT, 1e-10, [0, 3]), ("X", AT, 62, FLIP_AT, 1e-10, [1]),
                ("R", AT, 52, FLIP_AT, 1e-10, [2]),
                ("X", ROW * SK + 0, 62, 59, 1e-3, [1])]  # column 0 has stopped (59 iterations), columns 2 and 3 still run


@pytest.mark.parametrize("flip", SOLVER_FLIPS, ids=lambda f: "%s%d@%d" % (f[0], f[2], f[3]))
def test_protected_block_device_solve_under_a_flip_is_the_clean_solve(solver, flip):
    from abft_sparse_cg_amd.context import vecc_strip
    name, index, bit, when, thr, ops = flip
    clean = solver.run(thr, 5, True)
    assert clean[5] == [] and clean[0] == COUNTS[thr]
    if when == 59:
        assert not (clean[3][60] >> 0) & 1 and (clean[3][60] >> 3) & 1
    hit = solver.run(thr, 5, True, flip=(name, index, [bit], when))
    assert hit[0] == clean[0] and np.array_equal(D.bits(np.array(hit[2])), D.bits(np.array(clean[2])))
    assert np.array_equal(vecc_strip(hit[4]).view(U), vecc_strip(clean[4]).view(U))
    assert np.array_equal(hit[4].view(U), clean[4].view(U))
    assert hit[5] == [(CORRECTED, index, bit | op << 8) for op in ops], hit[5]


# ------------------------------------------------------------------------ 4. two flips in one word --

def test_double_flip_in_r_is_fatal_at_the_batchs_download(amd, capfd):
    s = Solver(amd, collect=False)  # events are printed and a fatal one raises, as for any caller without a handler
    try:
        seen = []
        ctx, v = s.ctx, s.v
        ctx.upload(v["B"], s.B0)
        ctx.upload(v["X"], np.zeros((s.n, SK)))

        def cb(i, rr, active):
            seen.append(i)
            if i == FLIP_AT:
                ctx.flip_vector(v["R"], AT, [52, 17])
        with pytest.raises(amd.FatalEvent):
            amd.cg_solve_block_device(ctx, s.A, *[v[name] for name in "BXRPW"], 1000, 1e-10, on_iteration=cb, stride=5,
                                      vector_ecc=True)
        assert seen == list(range(FLIP_AT + 1))  # raised before any callback of the batch that met it
        assert "[ECC] double-bit error detected in vector operand 2 at index %d\n" % AT in capfd.readouterr().out
    finally:
        s.close()


# ------------------------------------------------------------------------ 6. capture and refusals --

def test_capture_on_a_fresh_context_is_refused_until_the_loop_is_reserved(amd):
    n, k = 257, 3
    rng = np.random.default_rng(6)
    blocks = {name: B.block(_vecc.encode(rng.standard_normal(n * k)), k) for name in NAMES}
    rec = record_of(k)
    ref = VDev(amd, tri(n), k)
    try:
        ref.load(blocks, rec)
        ref.until(0.0)
        want = ref.words()
    finally:
        ref.close()
    dev = VDev(amd, tri(n), k)
    ctx = dev.ctx
    try:
        dev.load(blocks, rec)
        before = dev.words()
        spare, other = ctx.create_vector(4), ctx.create_vector(4)
        ctx.graph_begin()
        ctx.copy_vector(spare, other)  # (a node of its own: the graph is not empty)
        rc = dev.raw(0.0)
        msg = (ctx.L.abft_hip_last_error() or b"").decode()
        g = ctx.graph_end()
        ctx.graph_destroy(g)
        assert rc == ERR_INVALID and "abft_hip_block_loop_reserve" in msg, (rc, msg)
        after = dev.words()
        assert all(np.array_equal(after[key], before[key]) for key in before)
        assert dev.box.take() == []
        ctx.block_loop_reserve(dev.A, k)
        ctx.graph_begin()
        try:
            dev.until(0.0)
        finally:
            g = ctx.graph_end()
        ctx.graph_launch(g)
        got = dev.words()
        ctx.graph_destroy(g)
        assert all(np.array_equal(got[key], want[key]) for key in want)
        assert not np.array_equal(got["X"], before["X"])
    finally:
        dev.close()


def test_refusals_leave_vectors_records_and_the_event_queue_untouched(amd, monkeypatch):
    from abft_sparse_cg_amd import generators
    n, k = 257, 3
    rng = np.random.default_rng(7)
    blocks = {name: B.block(_vecc.encode(rng.standard_normal(n * k)), k) for name in NAMES}
    rec = record_of(k)

    def refused(d, call, text, extra=()):
        pre = d.words()
        more = [d.box.words(v) for v in extra]
        rc = call()
        assert rc == ERR_INVALID, text
        with pytest.raises(amd.AbftError, match=text):
            amd.capi.check(rc)
        post = d.words()
        assert all(np.array_equal(post[key], pre[key]) for key in pre), text
        assert all(np.array_equal(d.box.words(v), m) for v, m in zip(extra, more)), text
        assert d.ctx.L.abft_hip_pending_events(d.ctx.h) == 0 and d.box.take() == [], text

    # what abft_hip_spmm_dot_vecc refuses about the matrix: the message names COO, or the layout
    coo = VDev(amd, tri(n), k, "secded", fmt="coo", layout=None)
    try:
        coo.load(blocks, rec)
        refused(coo, lambda: coo.raw(0.0), "cg_block_vecc_iteration_until: .*COO")
    finally:
        coo.close()
    monkeypatch.setenv("ABFT_HIP_LAYOUT", "panels")
    monkeypatch.setenv("ABFT_HIP_PANEL_WIDTH", "256")
    rnd = generators.generate("random:1024,8,1")
    pan = VDev(amd, rnd, k, "secded", layout=None)
    try:
        assert pan.ctx.matrix_info(pan.A)[0] == "panels"
        m = rnd[3]
        pb = {name: B.block(_vecc.encode(rng.standard_normal(m * k)), k) for name in NAMES}
        pan.load(pb, rec)
        refused(pan, lambda: pan.raw(0.0), "cg_block_vecc_iteration_until: .*panel")
        # ... and cg_solve_block_device(vector_ecc=True) refuses it before anything runs, with cg_solve_block's message
        b5 = pan.ctx.create_block(m, k)
        pre = pan.words()
        with pytest.raises(ValueError, match=r"vector_ecc needs a CSR matrix in the streaming layout \(this one: panels\)"):
            amd.cg_solve_block_device(pan.ctx, pan.A, b5, *pan.vecs(), 10, 1e-3, vector_ecc=True)
        post = pan.words()
        assert all(np.array_equal(post[key], pre[key]) for key in pre) and pan.box.take() == []
    finally:
        pan.close()
    monkeypatch.delenv("ABFT_HIP_LAYOUT")
    monkeypatch.delenv("ABFT_HIP_PANEL_WIDTH")

    dev = VDev(amd, tri(n), k)
    ctx = dev.ctx
    try:
        dev.load(blocks, rec)
        marks = _vecc.encode(np.arange(1.0, n * k + 1.0))
        short, longer = dev.box.vec(marks[:-1]), dev.box.vec(np.concatenate([marks, marks[:k]]))
        four = ctx.create_block(n, 4)
        both = dev.box.vec(np.concatenate([marks, marks]))
        xa, rb = ctx.view_vector(both, 0, n * k), ctx.view_vector(both, n * k - 1, n * k)  # one entry shared
        extra = [short, longer, both]
        X, R, P, W = dev.vecs()
        r, pw = dev.rec, dev.pw_at
        name = "cg_block_vecc_iteration_until: "
        bad = [(dict(vecs=(short, R, P, W)), name), (dict(vecs=(X, longer, P, W)), name),        # lengths
               (dict(vecs=(X, R, P, four)), name),
               (dict(k=0), "outside"), (dict(k=9), "outside"), (dict(k=-1), "outside"), (dict(k=2), name),
               (dict(k=4), name),
               (dict(at=(0, pw, 0)), "records overlap"), (dict(at=(0, pw, r - 1)), "records overlap"),
               (dict(at=(0, r - 1, r)), "records overlap"), (dict(at=(0, r + 1, r)), "records overlap"),  # P.W inside one
               (dict(at=(0, pw - k, r)), "records overlap"),
               (dict(at=(None, pw, r)), "null device scalar"), (dict(at=(0, None, r)), "null device scalar"),
               (dict(at=(0, pw, None)), "null device scalar"),
               (dict(vecs=(None, R, P, W)), "null argument"), (dict(vecs=(X, R, P, None)), "null argument"),
               (dict(A=None), "null argument"),
               (dict(vecs=(X, R, P, X)), "overlap"), (dict(vecs=(X, R, W, W)), "overlap"),
               (dict(vecs=(xa, rb, P, W)), "overlap")]
        for kw, text in bad:
            refused(dev, lambda: dev.raw(0.0, **kw), text, extra)
        # cg_solve_block_device(vector_ecc=True) with a precond: refused before anything runs
        b5 = ctx.create_block(n, k)
        ctx.upload(b5, rng.standard_normal((n, k)))
        b5_pre = ctx.download(b5).view(U).copy()
        pre = dev.words()
        for dinv in (ctx.jacobi(dev.A), ctx.jacobi(dev.A, protected=True)):
            with pytest.raises(ValueError, match="vector_ecc with a precond: the protected block loop has no Jacobi form"):
                amd.cg_solve_block_device(ctx, dev.A, b5, X, R, P, W, 10, 1e-3, precond=dinv, vector_ecc=True)
        post = dev.words()
        assert all(np.array_equal(post[key], pre[key]) for key in pre) and dev.box.take() == []
        assert np.array_equal(ctx.download(b5).view(U), b5_pre)
        assert dev.raw(0.0) == 0  # and the call itself is fine
        assert not np.array_equal(dev.words()["X"], pre["X"])
    finally:
        dev.close()
