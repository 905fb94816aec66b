"""The x update inside the next SpMV (ABFT_HIP_X_IN_SPMV; include/abft_hip.h: abft_hip_x_in_spmv_stats; DESIGN.md
section 4, "Fourth cross-call fusion"): in the host-scalar loop spmv, dot, calc_xr, calc_p the library leaves
x += alpha p pending on the old p and lets the following spmv(A, p, w) apply it.  Transparent: every case plays one
call script on two contexts, the switch on and off, and compares the bit patterns of every scalar handed back, of
x, r, p, w (and the spare q), and the drained events; a third run (switch off) looks at x, r and p around every
calc_xr and calc_p and holds them against the numpy formulas x + alpha * p and r + beta * p.  alpha and beta are
chosen, not CG's quotients: nothing here needs to converge.  The counters say which path ran."""
import numpy as np
import pytest

import _x_in_spmv as X

pytestmark = pytest.mark.gpu

MODES = ["none", "constraints", "sed", "sec7", "sec8", "secded"]
K = 9


def both(monkeypatch, mode, mat, script, check_formulas=True, **kw):
    import abft_sparse_cg_amd as amd
    monkeypatch.setenv("ABFT_HIP_X_IN_SPMV", "1")
    on = X.run(amd, mode, mat, script, **kw)
    monkeypatch.setenv("ABFT_HIP_X_IN_SPMV", "0")
    off = X.run(amd, mode, mat, script, **kw)
    assert off["stats"] == (0, 0)
    X.same(on, off)
    if check_formulas:
        peeked = X.run(amd, mode, mat, script, peek=True, **kw)
        X.formulas_hold(peeked)
        for c in "xp":
            if c in on.get("vectors", {}):
                assert np.array_equal(X.bits(on["vectors"][c]), X.bits(peeked["vectors"][c])), c
    return on["stats"]


# ---- the predicted loop: K iterations, K - 2 updates applied by an SpMV, the last one by the download ----
PLAIN = [(m, "lap40") for m in MODES] + [(m, "rand") for m in MODES] + [
    ("none", "lap37x41"), ("none", "lap3"), ("none", "one"), ("secded", "one"), ("none", "diag23"), ("none", "diag1"),
    ("sec8", "diag23"), ("none", "arrow"), ("secded", "arrow"), ("constraints", "arrow"), ("none", "holes"),
    ("constraints", "holes"), ("sed", "holes")]


@pytest.mark.parametrize("mode,which", PLAIN)
def test_predicted_loop_same_bits_and_counters(mode, which, monkeypatch):
    assert both(monkeypatch, mode, X.matrix(which), X.loop(K)) == (K - 2, 1)


@pytest.mark.parametrize("env", ["ABFT_HIP_PACKED", "ABFT_HIP_COMPACT_COLS"])
def test_other_builds_of_the_data_path(env, monkeypatch):
    monkeypatch.setenv(env, "0")
    assert both(monkeypatch, "none", X.matrix("lap40"), X.loop(K)) == (K - 2, 1)


# ---- a flip in an element that an absorbing SpMV reads ----
def element_of_row(mat, row, k):
    return int(np.searchsorted(mat[1], row)) + k


@pytest.mark.parametrize("mode,bit,kinds", [("secded", 37, {2}), ("sed", 37, {1}), ("constraints", 70, {8})])
def test_flip_read_by_an_absorbing_spmv(mode, bit, kinds, monkeypatch):
    """the flip goes in right behind an SpMV (nothing pending, the prediction stays armed): the next SpMV applies the
    pending update AND meets the flipped element -- corrected (secded), fatal (sed), an order event (constraints)"""
    mat = X.matrix("lap40")
    at = element_of_row(mat, 700, 2)  # the diagonal of row 700
    script = X.loop(3) + [("spmv", "A", "p", "w"), ("inject", "A", at, [bit]), ("dot", "p", "w"), ("calc_xr", 0.4),
                          ("calc_p", 0.55), ("stats",)] + X.loop(2, first=4)
    import abft_sparse_cg_amd as amd
    monkeypatch.setenv("ABFT_HIP_X_IN_SPMV", "1")
    on = X.run(amd, mode, mat, script)
    assert on["scalars"][-5] == (2, 0) and on["stats"] == (4, 1)  # iteration 5's SpMV absorbed: it read the flip first
    assert on["events"] and {e[0] for e in on["events"]} == kinds and all(e[1] == at for e in on["events"])
    assert both(monkeypatch, mode, mat, script) == (4, 1)


# ---- scripts that must flush, or never arm ----
def between(extra):
    """three iterations (the third SpMV absorbs), `extra` between calc_p and the SpMV that would have absorbed, two more
    iterations: the second of them arms again, and its calc_p leaves an update for the download"""
    return X.loop(3) + [("stats",)] + extra + [("stats",)] + X.loop(2, first=3)


BETWEEN = {
    "download x": [("download", "x")],
    "download p": [("download", "p")],
    "upload x": [("upload", "x")],
    "dot(r, r)": [("dot", "r", "r")],
    "copy q <- p": [("copy", "q", "p")],
    "inject": [("inject", "A", 17, [3])],
    "calc_p again": [("calc_p", 0.25)],
}


@pytest.mark.parametrize("what", sorted(BETWEEN))
def test_something_else_comes_first(what, monkeypatch):
    import abft_sparse_cg_amd as amd
    script = between(BETWEEN[what])
    monkeypatch.setenv("ABFT_HIP_X_IN_SPMV", "1")
    on = X.run(amd, "secded" if what == "inject" else "none", X.matrix("lap40"), script)
    counters = [s for s in on["scalars"] if isinstance(s, tuple)]
    assert counters == [(1, 0), (1, 1)], counters  # applied on its own, by the call that came first
    assert both(monkeypatch, "secded" if what == "inject" else "none", X.matrix("lap40"), script) == (1, 2)


OTHER_SPMV = {
    "another vector": ([("spmv", "A", "q", "w")], None),
    "a COO matrix": ([("spmv", "B", "p", "w")], ("coo", None, None)),
    "the sweep layout": ([("spmv", "B", "p", "w")], ("csr", "ABFT_HIP_LAYOUT", "sweep")),
    "the panel layout": ([("spmv", "B", "p", "w")], ("csr", "ABFT_HIP_LAYOUT", "panels")),
    "result aliases x": ([("spmv", "A", "p", "x")], None),
}


@pytest.mark.parametrize("what", sorted(OTHER_SPMV))
def test_a_different_spmv(what, monkeypatch):
    """iteration 4 starts with an SpMV that is not the predicted one: the pending update is applied first"""
    spmv, second = OTHER_SPMV[what]
    script = (X.loop(3) + spmv + [("stats",), ("dot", "p", "w"), ("calc_xr", 0.4), ("calc_p", 0.55)] + X.loop(1, first=4))
    import abft_sparse_cg_amd as amd
    monkeypatch.setenv("ABFT_HIP_X_IN_SPMV", "1")
    on = X.run(amd, "none", X.matrix("lap40"), script, second=second)
    assert [s for s in on["scalars"] if isinstance(s, tuple)] == [(1, 1)]
    assert both(monkeypatch, "none", X.matrix("lap40"), script, second=second) == (1, 2)


def test_stop_right_after_calc_p_then_close(monkeypatch):
    import abft_sparse_cg_amd as amd
    monkeypatch.setenv("ABFT_HIP_X_IN_SPMV", "1")
    out = X.run(amd, "none", X.matrix("lap40"), X.loop(3), finish="close")  # shutdown applies it and frees both buffers
    assert out["stats"] == (1, 0)
    assert both(monkeypatch, "none", X.matrix("lap40"), X.loop(3)) == (1, 1)


def test_p_destroyed_while_pending(monkeypatch):
    script = X.loop(3) + [("destroy", "p"), ("stats",)]
    assert both(monkeypatch, "none", X.matrix("lap40"), script, check_formulas=False) == (1, 1)


@pytest.mark.parametrize("kw", [dict(expose=("p",)), dict(expose=("x",)), dict(p_view=True)], ids=["p exposed", "x exposed", "p a view"])
def test_vectors_the_caller_can_see_into_never_arm(kw, monkeypatch):
    assert both(monkeypatch, "none", X.matrix("lap40"), X.loop(K), **kw) == (0, 0)


def test_graph_begin_while_pending(monkeypatch):
    """the capture starts with the update applied, and from then on p's buffer is never swapped again"""
    script = X.loop(3) + [("graph",), ("stats",)] + X.loop(3, first=3)
    assert both(monkeypatch, "none", X.matrix("lap40"), script) == (1, 1)


@pytest.mark.parametrize("env,value", [("ABFT_HIP_FUSE_DOT", "0"), ("ABFT_HIP_FUSE_X", "0"), ("ABFT_HIP_SPECULATE", "1")])
def test_switches_that_keep_it_off(env, value, monkeypatch):
    monkeypatch.setenv(env, value)
    assert both(monkeypatch, "none", X.matrix("lap40"), X.loop(K)) == (0, 0)


@pytest.mark.parametrize("mode", MODES)
def test_default_arms_on_mode_none_only(mode, monkeypatch):
    """with the variable unset the prediction is armed on matrices of mode none alone (where it was measured to pay);
    the other modes run the calls as before"""
    import abft_sparse_cg_amd as amd
    monkeypatch.delenv("ABFT_HIP_X_IN_SPMV", raising=False)
    default = X.run(amd, mode, X.matrix("lap40"), X.loop(K))
    assert default["stats"] == ((K - 2, 1) if mode == "none" else (0, 0))
    monkeypatch.setenv("ABFT_HIP_X_IN_SPMV", "0")
    X.same(default, X.run(amd, mode, X.matrix("lap40"), X.loop(K)))


def test_two_lengths_alternate_without_reallocating(monkeypatch):
    """two solves of different lengths in one context, taking turns: each keeps its own second buffer"""
    import abft_sparse_cg_amd as amd
    out = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("ABFT_HIP_X_IN_SPMV", switch)
        ctx = amd.HIPContext("none", "csr")
        sets = []
        for name in ("lap40", "lap37x41"):
            cols, rows, vals, n = X.matrix(name)
            A = ctx.create_matrix(cols, rows, vals, n, len(vals))
            v = [ctx.create_vector(n) for _ in range(4)]
            rng = np.random.default_rng(3)
            for u in v[:3]:
                ctx.upload(u, rng.random(n) - 0.5)
            ctx.upload(v[3], np.zeros(n))
            sets.append((A, v))
        for turn in range(6):
            A, (x, r, p, w) = sets[turn % 2]
            for j in range(4):
                ctx.spmv(A, p, w)
                ctx.dot(p, w)
                ctx.calc_xr(x, r, p, w, 0.3 + 0.01 * j)
                ctx.calc_p(p, r, 0.5 - 0.01 * j)
        got = [ctx.download(u) for _, v in sets for u in v]
        out[switch] = (got, ctx.x_in_spmv_stats())
        ctx.close()
    assert out["0"][1] == (0, 0) and out["1"][1][0] > 0
    for a, b in zip(out["1"][0], out["0"][0]):
        assert np.array_equal(X.bits(a), X.bits(b))
