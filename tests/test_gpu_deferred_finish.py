"""ABFT_HIP_DEFER_FINISH: the reductions in front of a kernel that runs ahead leave their finish to that kernel's head.
The same launches carry the same bits, so the host-scalar loop played over the C ABI with the switch at 0 and at 1
must hand back every scalar, leave every vector and count every commit, drop, absorption and flush alike, bit for
bit, at run-ahead levels 1 and 2.

"After every iteration": a download between two iterations is itself an entry point that flushes what is pending and
disarms the prediction, so it would change what runs.  The state after iteration j is therefore read at the end of the
script cut to j iterations, for every j (`every_prefix`).  The one large matrix is played once, whole: there every
iteration's p.w, alpha, r.r and beta (each a function of all of that iteration's vectors) and the vectors after the
last iteration are compared.

Shapes, the smallest that reach each path (a reduction block covers 2048 elements):
    n = 1                   one block, one partial (3.3 on the diagonal: r.r stays finite and non-zero for 6 iterations)
    n = 2047, 2048, 2049    reduce_blocks goes 1 -> 2
    n = 2049 behind views   an operand that is a view at an odd offset: not plain_vector, must not arm
    laplace5:90,93          a few blocks; 33 row blocks, so the fused p.w is finished by the one-workgroup kernel, and
                            level 2 leaves that hand-off as it is
    laplace5:2048,2049      n = 4 196 352: reduce_blocks capped at 2048 with a second stride pass, more than 8192 row
                            blocks, so the multi-workgroup fold runs and level 2 defers its finish too"""
import numpy as np
import pytest

import _ahead
from _ahead import predicted, same
from _matrices import diagonal
from _oracle import laplace5

pytestmark = pytest.mark.gpu

LEVELS = ["1", "2"]
_made = {}


@pytest.fixture
def amd(monkeypatch):
    """the package, with the loop's other switches as the library sets them"""
    for name in ("ABFT_HIP_X_IN_SPMV", "ABFT_HIP_SPECULATE", "ABFT_HIP_FUSE_X", "ABFT_HIP_FUSE_DOT"):
        monkeypatch.delenv(name, raising=False)
    import abft_sparse_cg_amd
    return abft_sparse_cg_amd


def matrix(name):
    if name not in _made:
        if name == "one":
            _made[name] = (np.array([0], np.uint32), np.array([0], np.uint32), np.array([3.3]), 1)
        elif name.startswith("diag"):
            _made[name] = diagonal(int(name[4:]), True)
        else:
            nx, ny = name[3:].split("x")
            _made[name] = laplace5(int(nx), int(ny))
    return _made[name]


def both(amd, monkeypatch, level, script, mat, run=_ahead.run, **kw):
    """the script with the switch at 0 and at 1 -> the two results, equal in everything a caller can see"""
    monkeypatch.setenv("ABFT_HIP_AHEAD", level)
    res = []
    for switch in "01":
        monkeypatch.setenv("ABFT_HIP_DEFER_FINISH", switch)
        res.append(run(amd, "none", mat, script, **kw))
    off, on = res
    same(on, off)
    for counters in ("ahead", "xin", "spec"):
        assert on.get(counters) == off.get(counters), (counters, on.get(counters), off.get(counters))
    return on


def every_prefix(amd, monkeypatch, level, script, mat):
    for j in range(1, len(script) + 1):
        res = both(amd, monkeypatch, level, script[:j], mat)
    return res


def ran_ahead(res, script, level):
    """the run-ahead did what the arming rule says: with the switch on, every one of these went through the deferred pair"""
    flat = [s for s in res["scalars"] if not isinstance(s, np.ndarray)]
    want = _ahead.expected(script, flat, int(level))
    assert res["ahead"] == want, (res["ahead"], want)
    return want


CLEAN = predicted(5)
ALPHA_OFF = [{}, {}, {"alpha_ulps": 1}, {}, {}, {}]  # dropped (level 2) or not launched (level 1); armed again behind it
BETA_OFF = [{}, {}, {"beta_ulps": 1}, {}, {}, {}]    # the calc_p that ran ahead -- and published r.r -- is dropped


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", ["one", "diag2047", "diag2048", "diag2049", "lap90x93"])
def test_clean_loop_after_every_iteration(amd, monkeypatch, name, level):
    res = every_prefix(amd, monkeypatch, level, CLEAN, matrix(name))
    cp, cr, dropped = ran_ahead(res, CLEAN, level)
    assert cp == len(CLEAN) - 1 and dropped == 0 and (cr > 0) == (level == "2")


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("script", [ALPHA_OFF, BETA_OFF], ids=["alpha_one_ulp_off", "beta_one_ulp_off"])
@pytest.mark.parametrize("name", ["diag2049", "lap90x93"])
def test_drop_paths_after_every_iteration(amd, monkeypatch, name, script, level):
    """the published r.r must arrive, and be right, also where what published it is dropped"""
    res = every_prefix(amd, monkeypatch, level, script, matrix(name))
    cp, cr, dropped = ran_ahead(res, script, level)
    assert cp > 0 and (dropped > 0 or (script is ALPHA_OFF and level == "1"))


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", ["diag2049", "lap90x93"])
def test_stop_after_calc_xr(amd, monkeypatch, name, level):
    """the script ends between calc_xr and calc_p (a spare vector destroyed): the calc_p in flight is never asked for"""
    script = predicted(3) + [{"before_p": [("destroy", "q")]}]
    res = both(amd, monkeypatch, level, script, matrix(name))
    assert "q" not in res["vectors"] and res["ahead"][2] >= 1


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", ["diag2049", "lap90x93"])
def test_download_r_between_calc_xr_and_calc_p(amd, monkeypatch, name, level):
    script = predicted(3) + [{"before_p": [("download", "r")]}, {}, {}]
    res = both(amd, monkeypatch, level, script, matrix(name))
    assert res["ahead"][0] > 0 and res["ahead"][2] >= 1


@pytest.mark.parametrize("level", LEVELS)
def test_two_lengths_taking_turns(amd, monkeypatch, level):
    """two solves of different lengths in one context, four iterations each in turn (a turn's second iteration arms,
    its third and fourth run ahead), one turn cut short inside an iteration: the partial areas are the context's,
    used by both"""
    mats = [matrix("diag2049"), matrix("lap90x93")]
    turns = [(0, 16), (1, 16), (0, 14), (1, 16), (0, 18), (1, 16)]

    def run(amd, mode, mats, turns):
        res = _ahead.run_turns(amd, mode, mats, turns)
        res["spec"] = None
        return res

    res = both(amd, monkeypatch, level, turns, mats, run=run)
    assert res["ahead"][0] > 0


def _run_behind_views(amd, mode, mat, script):
    """_ahead.run with x, r, p and w as views at offset 1 of allocations one element longer: 8 bytes off the 16-byte
    alignment, and not plain_vector"""
    cols, rows, vals, n = mat
    ctx = amd.HIPContext(mode, "csr")
    out = {"scalars": [], "events": []}
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        whole = {c: ctx.create_vector(n + 1) for c in "xrpw"}
        V = {c: ctx.view_vector(whole[c], 1, n) for c in "xrpw"}
        start = _ahead.start_vectors(n)
        for c in "xrpw":
            ctx.upload(V[c], start[c])
        _ahead.play(ctx, A, V, n, script, out, [])
        out["vectors"] = {c: ctx.download(whole[c]) for c in "xrpw"}
        out["ahead"] = ctx.ahead_stats()
        out["xin"] = ctx.x_in_spmv_stats()
        out["spec"] = _ahead.spec_stats(ctx)
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("level", LEVELS)
def test_unaligned_views_do_not_arm(amd, monkeypatch, level):
    mat = matrix("diag2049")
    res = both(amd, monkeypatch, level, CLEAN, mat, run=_run_behind_views)
    assert res["ahead"] == (0, 0, 0)


@pytest.mark.parametrize("level", LEVELS)
def test_capped_grid_and_deferred_fold(amd, monkeypatch, level):
    script = predicted(8)
    res = both(amd, monkeypatch, level, script, matrix("lap2048x2049"))
    cp, cr, dropped = ran_ahead(res, script, level)
    assert cp == 7 and dropped == 0 and (cr > 0) == (level == "2")
