"""Matrix digests on the GPU: every stored array of a matrix that kernels only read, or only
repair, is a segment with the digest D = sum w[i] (2 i + 1) mod 2^64; a matrix is armed once and verified now and then.

The digests are held bit for bit against the numpy model of tests/_digest.py on what read_segment returns.  The set of
segments a case must have is written here BY HAND from csrc/abft_internal.h (CsrDev, CsrCompact, CsrPacked,
CsrPackedFast, CsrStruct, CsrPanels, SweepLayout, SliceLayout, CooDev), not read from the library.  The matrices are
those of tests/_structecc.py and the 1 x 1 matrix; the layouts other than the default are forced with ABFT_HIP_LAYOUT.
The solvers' keyword is held against the run without it, bit for bit, and against the gap it closes: a flipped palette
word (mode none) or sweep-table word (secded) that the run without the keyword never notices."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _digest as D
import _structecc as S
from _oracle import rhs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EV_DIGEST = 16
NAMES = ["lap40", "wide5", "rand", "diag23", "arrow", "holes", "one"]

CSR_PLAIN = {"cols", "vals", "rowptr", "blk"}
CSR_PERMUTED = CSR_PLAIN | {"orig_index", "pos_of_orig"}
COO = {"elems", "grp_ptr", "coo_blk", "coo_orig_index", "coo_pos_of_orig"}
COMPACT = {"cols16", "cbase"}
PACKED = {"code16", "pdesc", "pal", "fast"}
# name -> (format, mode, create_matrix keywords, environment, layout matrix_info must report, segments)
CASES = {
    "csr-stream-none": ("csr", "none", dict(layout="stream"), {}, "stream", CSR_PLAIN),  # + COMPACT / PACKED by matrix: below
    "csr-stream-secded": ("csr", "secded", dict(layout="stream"), {}, "stream", CSR_PLAIN),
    "csr-stream-sec7": ("csr", "sec7", dict(layout="stream"), {}, "stream", CSR_PLAIN),
    "csr-stream-struct": ("csr", "secded", dict(layout="stream", structure_ecc=True), {}, "stream", {"cols", "vals", "rowext", "sblk"}),
    "csr-sweep": ("csr", "secded", {}, dict(ABFT_HIP_LAYOUT="sweep", ABFT_HIP_PANEL_WIDTH="16"), "sweep",
                  CSR_PERMUTED | {"wbase", "counts"}),
    "csr-panels": ("csr", "sec7", {}, dict(ABFT_HIP_LAYOUT="panels", ABFT_HIP_PANEL_WIDTH="16"), "panels",
                   CSR_PERMUTED | {"seg_base", "seg_ptr"}),
    "csr-slice": ("csr", "none", {}, dict(ABFT_HIP_LAYOUT="slice", ABFT_HIP_PANEL_WIDTH="16"), "slice", CSR_PERMUTED | {"sub", "rid"}),
    "coo-grouped": ("coo", "secded", {}, dict(ABFT_HIP_LAYOUT="stream"), "stream", COO),
    "coo-panels": ("coo", "sec7", {}, dict(ABFT_HIP_LAYOUT="panels", ABFT_HIP_PANEL_WIDTH="16"), "panels", COO | {"seg_base", "seg_ptr"}),
    "coo-constraints": ("coo", "constraints", {}, dict(ABFT_HIP_LAYOUT="stream"), "stream", COO | {"as_created"}),
}
# mode none on the streaming layout: every block of these matrices is one tile of columns within 65536 (compact); the
# blocks of lap40 and wide5 hold {-1, 4} (packed), holes at most 12 values (packed), the others too many or a long row
NONE_EXTRA = {"lap40": COMPACT | PACKED, "wide5": COMPACT | PACKED, "holes": COMPACT | PACKED, "rand": COMPACT,
              "diag23": COMPACT, "arrow": COMPACT, "one": COMPACT | PACKED}
LAYOUT_KNOBS = ["ABFT_HIP_LAYOUT", "ABFT_HIP_PANEL_WIDTH"]


@pytest.fixture(scope="module")
def amd():
    import abft_sparse_cg_amd as a
    return a


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Box:
    """one context and one matrix of a case; events collected, or printed and raised (collect=False)"""

    def __init__(self, amd, monkeypatch, case, name, collect=True):
        fmt, mode, kw, env, self.layout, _ = CASES[case]
        for k in LAYOUT_KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        cols, rows, vals, n = S.matrix(name)
        self.events, self.fatal = [], False
        self.ctx = amd.HIPContext(mode, fmt, on_event=self._on if collect else None)
        self.case, self.name, self.n, self.nnz = case, name, n, len(vals)
        self.A = self.ctx.create_matrix(cols, rows, vals, n, len(vals), **kw)
        for k in LAYOUT_KNOBS:
            monkeypatch.delenv(k, raising=False)

    def _on(self, ev, fatal):
        self.events += ev
        self.fatal |= fatal

    def take(self):
        self.ctx._drain()  # (synchronises the stream)
        ev, f = self.events, self.fatal
        self.events, self.fatal = [], False
        return sorted(ev), f

    def vec(self, array, k=None):
        v = self.ctx.create_vector(len(array)) if k is None else self.ctx.create_block(len(array), k)
        self.ctx.upload(v, array)
        return v

    def expected(self):
        want = set(CASES[self.case][5])
        if self.case == "csr-stream-none":
            want |= NONE_EXTRA[self.name]
        return want

    def close(self):
        self.ctx.close()


def model_digests(box):
    return {s: D.digest(box.ctx.read_segment(box.A, s)) for s, _ in box.ctx.matrix_segments(box.A)}


# ---- 1. the registry and the digest -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_segments_are_the_expected_set_and_digests_equal_the_model(amd, monkeypatch, case):
    tails = set()
    for name in NAMES:
        box = Box(amd, monkeypatch, case, name)
        try:
            assert box.ctx.matrix_info(box.A)[0] == box.layout, (case, name)
            segs = box.ctx.matrix_segments(box.A)
            names = [s for s, _ in segs]
            assert len(set(names)) == len(names) and set(names) == box.expected(), (case, name, names)
            if case == "csr-stream-none":
                packed = box.ctx.packed_stats(box.A)[0]
                assert (packed > 0) == ("code16" in names), (name, packed)
                if name in ("lap40", "wide5"):
                    assert {"code16", "pdesc", "pal", "cols16", "cbase"} <= set(names)
            got = box.ctx.matrix_digest(box.A)
            assert list(got) == names
            for s, size in segs:
                data = box.ctx.read_segment(box.A, s)
                assert len(data) == size and size > 0
                assert got[s] == D.digest(data), (case, name, s, size)
                tails.add((size % 16 != 0, size % 4 != 0))
            # the digest reads and changes nothing: a second one is the same, and so is an armed verification
            assert box.ctx.matrix_digest(box.A) == got
            box.ctx.arm_matrix(box.A)
            assert box.ctx.verify_matrix(box.A) == [] and box.take() == ([], False)
        finally:
            box.close()
    assert (True, False) in tails or (True, True) in tails  # a tail behind the last 16-byte group was walked
    if case in ("csr-panels", "coo-panels"):
        assert (True, True) in tails  # `one`: seg_ptr is 2049 16-bit offsets, a last word of two bytes


# ---- 2. every flip is found, in exactly its segment ----------------------------------------------------------------

def flip_positions(box, rng):
    """per segment: (word, bits) for the first word, the last, a padding word where the array has one, three seeded;
    bits 0, the word's highest stored bit, one seeded"""
    out = []
    pad_word = {"cols": box.nnz, "vals": 2 * box.nnz, "elems": 4 * box.nnz}  # behind the nnz stored elements
    for s, size in box.ctx.matrix_segments(box.A):
        nwords = (size + 3) // 4
        words = [0, nwords - 1] + [int(w) for w in rng.integers(0, nwords, 3)]
        if s in pad_word and pad_word[s] < nwords:
            words.append(pad_word[s])
        if s == "pal":
            words.append(nwords - 2)  # the pool's spare palettes
        for w in words:
            top = 8 * min(4, size - 4 * w) - 1
            out.append((s, w, sorted({0, top, int(rng.integers(0, top + 1))})))
    return out


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_every_flip_names_exactly_its_segment(amd, monkeypatch, case, seed):
    rng = np.random.default_rng(1000 + seed)
    box = Box(amd, monkeypatch, case, "lap40" if seed == 0 else "rand")
    ctx, A = box.ctx, box.A
    try:
        ctx.arm_matrix(A)
        clean = ctx.matrix_digest(A)
        spots = flip_positions(box, rng)
        for s, w, bits in spots:
            for b in bits:
                ctx.flip_segment(A, s, w, [b])
                assert ctx.verify_matrix(A) == [s], (case, s, w, b)
                ctx.flip_segment(A, s, w, [b])
                assert ctx.verify_matrix(A) == [], (case, s, w, b)
            if len(bits) > 1:  # two flips in one word
                ctx.flip_segment(A, s, w, bits[:2])
                assert ctx.verify_matrix(A) == [s], (case, s, w, bits)
                ctx.flip_segment(A, s, w, bits[:2])
        # two flips in two words of one segment, and two segments at once (named in segment order)
        order = [s for s, _ in ctx.matrix_segments(A)]
        by_seg = {}
        for s, w, bits in spots:
            by_seg.setdefault(s, []).append((w, bits[0]))
        for s, picks in by_seg.items():
            (w0, b0), (w1, b1) = picks[0], picks[1]  # the first and the last word
            if w0 == w1:
                continue
            ctx.flip_segment(A, s, w0, [b0])
            ctx.flip_segment(A, s, w1, [b1])
            assert ctx.verify_matrix(A) == [s], (case, s)
            ctx.flip_segment(A, s, w0, [b0])
            ctx.flip_segment(A, s, w1, [b1])
        a, b = order[0], order[-1]
        ctx.flip_segment(A, a, 0, [5])
        ctx.flip_segment(A, b, 0, [7])
        assert ctx.verify_matrix(A) == [a, b]
        ctx.flip_segment(A, a, 0, [5])
        ctx.flip_segment(A, b, 0, [7])
        assert ctx.verify_matrix(A) == [] and ctx.matrix_digest(A) == clean
        assert box.take() == ([], False)  # the synchronous verification queues nothing
        # the injector refuses what is not there
        with pytest.raises(amd.AbftError) as e:
            ctx.flip_segment(A, order[0], 1 << 40, [0])
        assert e.value.code == -1
        with pytest.raises(amd.AbftError):
            ctx.flip_segment(A, order[0], 0, [32])
        absent = "elems" if box.ctx.fmt == 0 else "cols"
        with pytest.raises(amd.AbftError) as e:
            ctx.flip_segment(A, absent, 0, [0])
        assert absent in str(e.value)
    finally:
        box.close()


# ---- 3. the enqueue-only verification -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["csr-stream-none", "csr-sweep", "coo-constraints"])
def test_verify_dev_queues_one_event_per_bad_segment(amd, monkeypatch, case):
    from abft_sparse_cg_amd import capi
    box = Box(amd, monkeypatch, case, "lap40")
    ctx, A = box.ctx, box.A
    try:
        for call in (ctx.verify_matrix_dev, ctx.verify_matrix):
            with pytest.raises(amd.AbftError) as e:  # not armed: refused, and the message names the remedy
                call(A)
            assert e.value.code == -1 and "abft_hip_matrix_digest_arm" in str(e.value)
        ctx.arm_matrix(A)
        order = [s for s, _ in ctx.matrix_segments(A)]
        first, last = order[1], order[-1]
        bad = sorted((EV_DIGEST, capi.segment_kind(s), 0) for s in (first, last))
        for _ in range(2):  # clean twice in a row: the second run starts from accumulators the first one zeroed
            ctx.verify_matrix_dev(A)
            assert box.take() == ([], False)
        ctx.flip_segment(A, first, 0, [0])
        ctx.flip_segment(A, last, 0, [31 if dict(ctx.matrix_segments(A))[last] >= 4 else 0])
        for _ in range(2):
            ctx.verify_matrix_dev(A)
            assert box.take() == (bad, True)
        # captured once, replayed three times: the same events per launch, none once the words are back
        ctx.graph_begin()
        try:
            ctx.verify_matrix_dev(A)
        finally:
            g = ctx.graph_end()
        try:
            for _ in range(3):
                ctx.graph_launch(g)
                assert box.take() == (bad, True)
            ctx.flip_segment(A, first, 0, [0])
            ctx.flip_segment(A, last, 0, [31 if dict(ctx.matrix_segments(A))[last] >= 4 else 0])
            for _ in range(3):
                ctx.graph_launch(g)
                assert box.take() == ([], False)
            # two verifications in one drain: the events of both, one per bad segment and launch
            ctx.flip_segment(A, first, 0, [3])
            ctx.graph_launch(g)
            ctx.graph_launch(g)
            assert box.take() == ([(EV_DIGEST, capi.segment_kind(first), 0)] * 2, True)
            ctx.flip_segment(A, first, 0, [3])
            assert ctx.verify_matrix(A) == []
        finally:
            ctx.graph_destroy(g)
    finally:
        box.close()


# ---- 4. legitimate writes --------------------------------------------------------------------------------------------

def test_a_repaired_word_passes_again_and_a_miscorrected_one_does_not(amd, monkeypatch):
    n = S.matrix("lap40")[3]
    x = rhs(n, 7) - 0.5
    # secded: one flipped bit is repaired by the SpMV that meets it, the stored word restored
    box = Box(amd, monkeypatch, "csr-stream-secded", "lap40")
    try:
        ctx, A = box.ctx, box.A
        ctx.arm_matrix(A)
        vx, vy = box.vec(x), box.vec(np.zeros(n))
        ctx.inject_at(A, 777, [13])
        assert ctx.verify_matrix(A) == ["vals"]
        ctx.spmv(A, vx, vy)
        ev, fatal = box.take()
        assert ev == [(2, 777, 13)] and not fatal
        assert ctx.verify_matrix(A) == []
    finally:
        box.close()
    # sec7 cannot tell two flips from one: whatever it stores back, the word is not the original
    box = Box(amd, monkeypatch, "csr-stream-sec7", "lap40")
    try:
        ctx, A = box.ctx, box.A
        ctx.arm_matrix(A)
        vx, vy = box.vec(x), box.vec(np.zeros(n))
        ctx.inject_at(A, 777, [13, 40])
        ctx.spmv(A, vx, vy)
        box.take()
        bad = ctx.verify_matrix(A)
        assert "vals" in bad and set(bad) <= {"vals", "cols"}, bad
    finally:
        box.close()


def test_a_packed_replan_keeps_the_registry_usable_and_fails_verification(amd, monkeypatch):
    box = Box(amd, monkeypatch, "csr-stream-none", "lap40")
    try:
        ctx, A = box.ctx, box.A
        ctx.arm_matrix(A)
        before = ctx.matrix_segments(A)
        packed = ctx.packed_stats(A)[0]
        ctx.inject_at(A, 300, [51])  # a value no palette of the matrix holds: the block is planned anew
        assert ctx.matrix_segments(A) == before  # pointers and lengths as they were: nothing is reallocated
        assert ctx.matrix_digest(A) == model_digests(box)
        bad = ctx.verify_matrix(A)
        assert "vals" in bad and set(bad) <= {"vals", "code16", "pdesc", "pal", "fast"}, bad
        ctx.inject_at(A, 300, [95])  # a column bit: the compact copy follows, or the block goes wide
        assert ctx.matrix_digest(A) == model_digests(box)
        assert "cols" in ctx.verify_matrix(A)
        assert ctx.packed_stats(A)[0] <= packed
        ctx.arm_matrix(A)  # arming again takes a new reference
        assert ctx.verify_matrix(A) == []
    finally:
        box.close()


# ---- 5. the solvers ---------------------------------------------------------------------------------------------------

ITRS = 40


def count_host(itr, M):
    """verifications of a host loop that ran itr iterations: behind every M-th, and one on the final state unless it
    has just been seen"""
    return itr // M + (1 if itr % M or itr == 0 else 0)


def count_device(itr, M, stride):
    """... of a device loop that ran all of max_itrs = itr: one per batch that reaches or passes a multiple of M, and
    one behind the loop when the last batch had none"""
    done, seen, last = 0, 0, False
    while done < itr:
        m = min(stride, itr - done)
        last = (done + m) // M > done // M
        seen += last
        done += m
    return seen + (0 if last else 1)


class Solve:
    """one solver on one matrix: fresh vectors per run, so every run starts from the same bits"""

    def __init__(self, amd, box, kind, **kw):
        self.amd, self.box, self.kind, self.kw = amd, box, kind, kw
        self.k = 3 if "block" in kind else None
        n = box.n
        self.b = rhs(n, 11) if self.k is None else np.stack([rhs(n, 11 + j) for j in range(self.k)], axis=1)

    def run(self, **more):
        box, ctx, k = self.box, self.box.ctx, self.k
        shape = self.b.shape
        vs = [box.vec(self.b, k)] + [box.vec(np.zeros(shape), k) for _ in range(4)]
        hist = []
        user = more.pop("on_iteration", None)

        def on_it(i, rr, *active):
            hist.append((i, u64(np.atleast_1d(rr)).tolist()) + active)
            if user is not None:
                user(i)

        f = getattr(self.amd, self.kind)
        before = ctx.matrix_verifications
        try:
            itr, rr = f(ctx, box.A, *vs, ITRS, 1e-300, on_iteration=on_it, **self.kw, **more)
            x = ctx.download(vs[1])
        finally:
            for v in vs:
                ctx.destroy_vector(v)
        return dict(itr=itr, rr=u64(np.atleast_1d(rr)).tolist(), hist=hist, x=x, verified=ctx.matrix_verifications - before)


SOLVERS = [("cg_solve", {}), ("cg_solve_block", {}), ("cg_solve_block", dict(fused=True)),
           ("cg_solve_block_device", dict(stride=5))] + \
          [("cg_solve_device", dict(stride=s, graph=g)) for s in (1, 3, 16) for g in (True, False)]


@pytest.mark.parametrize("name", ["lap40", "rand"])
@pytest.mark.parametrize("kind,kw", SOLVERS, ids=lambda v: v if isinstance(v, str) else "-".join("%s%s" % i for i in v.items()) or "plain")
def test_a_clean_run_is_the_run_without_the_keyword(amd, monkeypatch, name, kind, kw):
    box = Box(amd, monkeypatch, "csr-stream-none", name, collect=False)
    try:
        s = Solve(amd, box, kind, **kw)
        plain = s.run()
        assert plain["verified"] == 0 and not box.A.digest_armed
        itr = plain["itr"] if np.isscalar(plain["itr"]) else max(plain["itr"])
        assert itr == ITRS  # the threshold is out of reach: every run makes all its iterations
        for M in (1, 7, 16):
            got = s.run(matrix_check_every=M)
            for key in ("itr", "rr", "hist"):
                assert got[key] == plain[key], (kind, kw, M, key)
            assert np.array_equal(u64(got["x"]), u64(plain["x"])), (kind, kw, M)
            want = count_device(ITRS, M, kw["stride"]) if "device" in kind else count_host(ITRS, M)
            assert got["verified"] == want, (kind, kw, M, got["verified"], want)
        assert box.A.digest_armed
        assert s.run(matrix_check_every=0)["verified"] == 0
    finally:
        box.close()


def flip_at(box, segment, word, bit, when):
    def hook(i):
        if i == when:
            box.ctx.flip_segment(box.A, segment, word, [bit])
    return hook


# (rand does not pack in mode none: it has no palette; its sweep tables are as unprotected as lap40's)
# The last field: must the damaged solve still converge?  The palette flip scales every -1 of the Laplacian alike: the
# matrix stays symmetric and diagonally dominant, CG converges on it.  A shifted wbase word moves a few rows' elements
# by one: the matrix is no longer symmetric.  rand is strictly diagonally dominant with a wide margin (diagonal minus
# off-diagonal sum > 0.99) and stays so: the recurrence still converges, to another x.  lap40 is dominant with no margin
# at all (4 against four -1): a row that gains or loses an element is not dominant any more, and CG owes nothing on
# such a matrix -- measured there, rr grows from 1.7e3 to 4.6e5 in 40 iterations.  That run, too, ends without an
# event or an exception, all residuals finite: asserted for every case.
GAPS = [("csr-stream-none", "lap40", "pal", 1, 10, True),  # the high word of palette entry 0: its value moves by 2^-10 of itself
        ("csr-sweep", "lap40", "wbase", None, 0, False),   # the first element of a (segment, wave) in the middle: rows shift by one
        ("csr-sweep", "rand", "wbase", None, 0, True)]


def middle_base(box, segment):
    """the base of a (segment, wave) that holds elements, in the middle of the sweep table"""
    wb = box.ctx.read_segment(box.A, segment).view(np.uint32)
    holds = [i for i in range(1, len(wb) - 1) if wb[i + 1] > wb[i]]
    return holds[len(holds) // 2]


def rr_history(run):
    return np.array([h[1][0] for h in run["hist"]], dtype=np.uint64).view(np.float64)


@pytest.mark.parametrize("case,name,segment,word,bit,converges", GAPS)
@pytest.mark.parametrize("kind,kw,M", [("cg_solve", {}, 7), ("cg_solve", {}, 1), ("cg_solve_device", dict(stride=3), 7),
                                        ("cg_solve_device", dict(stride=16, graph=False), 16)])
def test_the_gap_it_closes(amd, monkeypatch, capfd, case, name, segment, word, bit, converges, kind, kw, M):
    box = Box(amd, monkeypatch, case, name, collect=False)
    try:
        ctx, A = box.ctx, box.A
        if word is None:
            word = middle_base(box, segment)
        s = Solve(amd, box, kind, **kw)
        clean = s.run()
        # without the keyword the run goes through on the damaged matrix, all checks of its own passed, to another x
        blind = s.run(on_iteration=flip_at(box, segment, word, bit, 5))
        assert blind["itr"] == ITRS and blind["verified"] == 0
        # ... and "converges": every residual finite, the last one far below the first, as on the clean matrix -- no
        # event, no exception, nothing a caller could tell from a good solve
        for run, must in ((clean, True), (blind, converges)):
            rr = rr_history(run)
            print(case, name, kind, "rr first %.3e last %.3e" % (rr[0], rr[-1]))
            assert len(rr) == ITRS and np.all(np.isfinite(rr)), (rr[0], rr[-1])
            if must:
                assert rr[-1] < 1e-2 * rr[0], (rr[0], rr[-1])
        assert not np.array_equal(u64(blind["x"]), u64(clean["x"]))
        ctx.flip_segment(A, segment, word, [bit])  # back
        assert np.array_equal(u64(s.run()["x"]), u64(clean["x"]))
        capfd.readouterr()
        # with it: FatalEvent, with the digest line, no later than the latency bound
        seen = []
        with pytest.raises(amd.FatalEvent) as e:
            s.run(matrix_check_every=M, on_iteration=lambda i: (seen.append(i), flip_at(box, segment, word, bit, 5)(i)))
        assert e.value.code == 1
        out = capfd.readouterr().out
        assert out.count("[ABFT] matrix digest mismatch in segment %s\n" % segment) == 1 and out.count("[ABFT]") == 1, out
        stride = kw.get("stride", 1)
        # the flip follows iteration 5; on_iteration has seen at most the iterations of the batch that found it
        assert max(seen) <= 5 + M + stride - 1, (seen, M, stride)
        if "device" not in kind:
            assert max(seen) == (5 // M + 1) * M - 1  # the first multiple of M behind the flip
    finally:
        box.close()


@pytest.mark.parametrize("case,name,segment,word,bit", [GAPS[0][:5], GAPS[2][:5]])
def test_no_checkpoint_on_an_unverified_matrix(amd, monkeypatch, capfd, case, name, segment, word, bit):
    """check_every=10 and a flip planted at iteration 12: the checkpoint of iteration 9 stays, and the verification in
    front of the check at iteration 19 raises before that check copies anything"""
    box = Box(amd, monkeypatch, case, name, collect=False)
    try:
        ctx, n = box.ctx, box.n
        if word is None:
            word = middle_base(box, segment)
        b, x, r, p, w = [box.vec(rhs(n, 11))] + [box.vec(np.zeros(n)) for _ in range(4)]
        ckpt = box.vec(np.full(n, -3.0))
        checks, kept = [], {}

        def on_check(itr, gap, ok, back):
            checks.append((itr, ok, back))
            kept[itr] = (ctx.download(ckpt), ctx.download(x))

        before = ctx.matrix_verifications
        with pytest.raises(amd.FatalEvent):
            amd.cg_solve(ctx, box.A, b, x, r, p, w, ITRS, 1e-300, on_iteration=lambda i, rr: flip_at(box, segment, word, bit, 12)(i),
                         check_every=10, x_ckpt=ckpt, on_check=on_check, matrix_check_every=50)
        assert "[ABFT] matrix digest mismatch in segment %s\n" % segment in capfd.readouterr().out
        assert checks == [(9, True, None)]
        assert np.array_equal(u64(kept[9][0]), u64(kept[9][1]))          # the check of iteration 9 took its checkpoint
        assert np.array_equal(u64(ctx.download(ckpt)), u64(kept[9][0]))  # and nothing has been copied over it since
        assert ctx.matrix_verifications - before == 2  # in front of the two checks, the second of which never ran
    finally:
        box.close()


def test_every_check_has_a_verification_in_front_of_it(amd, monkeypatch):
    box = Box(amd, monkeypatch, "csr-stream-secded", "rand", collect=False)
    try:
        ctx, n = box.ctx, box.n
        for k, f in ((None, amd.cg_solve), (3, amd.cg_solve_block)):
            shape = (n,) if k is None else (n, k)
            vs = [box.vec(np.stack([rhs(n, 11 + j) for j in range(k or 1)], axis=1).reshape(shape), k)] + \
                 [box.vec(np.zeros(shape), k) for _ in range(4)]
            order = []
            real = ctx.verify_matrix
            monkeypatch.setattr(ctx, "verify_matrix", lambda A: (order.append("v"), real(A))[1])
            f(ctx, box.A, *vs, 25, 1e-300, on_iteration=lambda i, rr, *a: order.append("i"),
              on_check=lambda *a: order.append("c"), check_every=10, matrix_check_every=4)
            monkeypatch.undo()
            text = "".join(order)
            states = text.replace("c", "")
            # never twice on one state; behind every fourth iteration; in front of every check (the columns of a block
            # check share one), with no iteration between; the last thing before returning unless a check was
            assert "vv" not in states and states.endswith("v"), text
            ran = 0
            for at, ch in enumerate(states):
                ran += ch == "i"
                if ch == "i" and ran % 4 == 0:
                    assert states[at + 1] == "v", (text, at)
            for at, ch in enumerate(text):
                if ch == "c":
                    assert text[:at].rstrip("c").endswith("v"), (text, at)
            assert ran == 25 and text.count("c") == 3 * (k or 1)
            assert states.count("v") == len({4, 8, 12, 16, 20, 24} | {10, 20} | {25}), text
    finally:
        box.close()


def test_other_loops_and_the_refusal(amd, monkeypatch, capfd):
    """precond, vector_ecc and trail_ecc loops take the keyword; the device loop refuses it beside check_every"""
    box = Box(amd, monkeypatch, "csr-stream-secded", "lap40", collect=False)
    try:
        ctx, n, A = box.ctx, box.n, box.A

        def vecs():
            return [box.vec(rhs(n, 11))] + [box.vec(np.zeros(n)) for _ in range(4)]

        with pytest.raises(ValueError) as e:
            amd.cg_solve_device(ctx, A, *vecs(), 10, 1e-300, check_every=5, matrix_check_every=5)
        assert "matrix_check_every" in str(e.value) and ctx.matrix_verifications == 0 and not A.digest_armed
        runs = [(amd.cg_solve, dict(precond=ctx.jacobi(A))),
                (amd.cg_solve, dict(vector_ecc=True)),
                (amd.cg_solve_device, dict(stride=4, trail_ecc=True)),
                (amd.cg_solve_device, dict(stride=4, vector_ecc=True, precond=ctx.jacobi(A, protected=True)))]
        for f, kw in runs:
            plain = f(ctx, A, *vecs(), 12, 1e-300, **kw)
            before = ctx.matrix_verifications
            vs = vecs()
            got = f(ctx, A, *vs, 12, 1e-300, matrix_check_every=5, **kw)
            assert got[0] == plain[0] == 12 and u64([got[1]]).tolist() == u64([plain[1]]).tolist(), kw
            want = count_device(12, 5, 4) if f is amd.cg_solve_device else count_host(12, 5)
            assert ctx.matrix_verifications - before == want, (kw, want)
        # a flip found through the protected device loop as through the plain one
        with pytest.raises(amd.FatalEvent):
            amd.cg_solve_device(ctx, A, *vecs(), 12, 1e-300, stride=4, trail_ecc=True, matrix_check_every=5,
                                # (a padding word of vals: loaded by the SpMV at most, never used)
                                on_batch=lambda done, trail: ctx.flip_segment(A, "vals", 2 * box.nnz + 1, [3]) if done == 4 else None)
        assert capfd.readouterr().out.count("[ABFT] matrix digest mismatch in segment vals\n") == 1
    finally:
        box.close()


# ---- 6. the command line -----------------------------------------------------------------------------------------------

def cli(*args):
    return subprocess.run([sys.executable, "-m", "abft_sparse_cg_amd.cg", "-t", "hip", "-s", "laplace5:40,40", "-i", "30", "-c", "0"]
                          + list(args), cwd=ROOT, capture_output=True, text=True, timeout=300)


def without_time(text):
    return [line for line in text.split("\n") if not line.startswith("time taken")]


def test_command_line():
    plain = cli("-m", "none")
    assert plain.returncode == 0 and "matrix" not in plain.stdout.replace("matrix size", "").replace("matrix block size", "")
    for extra in ([], ["--device-loop", "4"]):
        base = plain if not extra else cli("-m", "none", *extra)
        p = cli("-m", "none", "--verify-matrix", "8", *extra)
        assert p.returncode == 0, p.stdout + p.stderr
        lines = without_time(p.stdout)
        digests = [line for line in lines if line.startswith("matrix digests:")]
        assert len(digests) == 1
        words = digests[0].split()
        assert words[3] == "segments," and int(words[2]) == 10 and words[5] == "bytes," and words[-3:] == ["every", "8", "iterations"]
        assert lines.index(digests[0]) < lines.index(next(line for line in lines if line.startswith("iteration ") and "rr =" in line))
        want = count_device(30, 8, 4) if extra else count_host(30, 8)
        assert lines[lines.index("ran for 30 iterations") + 1] == "matrix verifications: %d passed" % want
        # the two lines are all the flag adds
        assert [line for line in lines if not line.startswith("matrix digests:") and not line.startswith("matrix verifications:")] \
            == without_time(base.stdout)
        # a flipped palette word: bit 40 counted from word 3 is bit 8 of word 4
        bad = cli("-m", "none", "--verify-matrix", "8", "--flip-matrix", "5:pal:3:40", *extra)
        assert bad.returncode == 1, bad.stdout + bad.stderr
        assert bad.stdout.count("[ABFT] matrix digest mismatch in segment pal\n") == 1
        assert "*** flipping bit 8 of word 4 of matrix segment pal ***" in bad.stdout and "ran for" not in bad.stdout
    # with the other flags: a residual check, block right-hand sides, another format and mode
    # (verified states: 16 and 30; with checks at 10, 20 and 30 as well: 10, 16, 20, 30)
    for args, segs, passed in ((["-m", "none", "--check-every", "10"], 10, 4), (["-m", "secded", "--rhs", "3"], 4, 2),
                               (["-m", "sec7", "--format", "coo"], 5, 2)):
        p = cli(*args, "--verify-matrix", "16")
        assert p.returncode == 0, p.stdout + p.stderr
        assert "matrix digests: %d segments, " % segs in p.stdout and "matrix verifications: %d passed" % passed in p.stdout, p.stdout
    # refusals are the parser's
    for args in (["--verify-matrix", "0"], ["--flip-matrix", "5:pal:3"], ["--flip-matrix", "5:nosuch:0:1"],
                 ["--flip-matrix", "5:pal:99999999:1"]):
        p = cli("-m", "none", *args)
        assert p.returncode == 1 and "Invalid --" in p.stdout, (args, p.stdout)
