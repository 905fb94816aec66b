"""The queue of x updates (ABFT_HIP_LAZY_X=1|2|4; include/abft_hip.h: abft_hip_lazy_x_stats; DESIGN.md section 4, "Sixth
cross-call fusion"): with depth d > 1 the predicted SpMV only queues the x += alpha p_old it takes over, and every d-th
one applies d of them in one pass.  Transparent: every case plays one call script with depth 2 and 4, with depth 1 and
with ABFT_HIP_X_IN_SPMV=0, and compares the bit patterns of every scalar handed back, of x, r, p, w (and the spare q)
and the drained events.  The counters of abft_hip_x_in_spmv_stats are those of depth 1; abft_hip_lazy_x_stats says how
many launches applied a full queue and how many queued updates something else had to apply first."""
import re
import types

import numpy as np
import pytest

import _ieee
import _x_in_spmv as X
from test_gpu_x_in_spmv import BETWEEN, MODES, OTHER_SPMV

pytestmark = pytest.mark.gpu

DEPTHS = (2, 4)


def play(monkeypatch, env, mode, mat, script, **kw):
    """X.run under `env`, plus what abft_hip_lazy_x_stats and abft_hip_ahead_stats say when the context goes"""
    import abft_sparse_cg_amd as amd
    seen = {}

    class Context(amd.HIPContext):
        def close(self):
            if self.h:
                seen["lazy"], seen["ahead"] = self.lazy_x_stats(), self.ahead_stats()
            super().close()

    for k in ("ABFT_HIP_X_IN_SPMV", "ABFT_HIP_LAZY_X"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = X.run(types.SimpleNamespace(HIPContext=Context), mode, mat, script, **kw)
    out.update(seen)
    return out


def counters(out):
    return [s for s in out["scalars"] if isinstance(s, tuple)] + [out["stats"]]


def all_depths(monkeypatch, mode, which, script, extra_env=None, **kw):
    """-> {depth: run}; depths 2 and 4 held against depth 1 and against the switch off"""
    env = dict(extra_env or {})
    mat = X.matrix(which)
    off = play(monkeypatch, dict(env, ABFT_HIP_X_IN_SPMV="0", ABFT_HIP_LAZY_X="4"), mode, mat, script, **kw)
    assert off["stats"] == (0, 0) and off["lazy"] == (0, 0, 0)
    runs = {d: play(monkeypatch, dict(env, ABFT_HIP_X_IN_SPMV="1", ABFT_HIP_LAZY_X=str(d)), mode, mat, script, **kw)
            for d in (1,) + DEPTHS}
    assert runs[1]["lazy"] == (0, 0, 0)
    X.same(runs[1], off)
    for d in DEPTHS:
        X.same(runs[d], runs[1])
        X.same(runs[d], off)
        assert counters(runs[d]) == counters(runs[1])
        assert runs[d]["ahead"] == runs[1]["ahead"]
        bursts, in_bursts, by_flush = runs[d]["lazy"]
        assert in_bursts == bursts * d
    return runs


def loop_to_fill(d, fill):
    """the shortest predicted loop (three iterations at least) that ends with `fill` updates queued and one pending"""
    L = 2 + fill
    return L if L >= 3 else L + d


# ---- the predicted loop at every length up to two bursts and a rest ----
@pytest.mark.parametrize("which", ["lap40", "lap3", "one", "lap37x41", "holes", "arrow", "rand"])
def test_loop_lengths(which, monkeypatch):
    for L in range(3, 2 * 4 + 4):
        runs = all_depths(monkeypatch, "none", which, X.loop(L))
        assert runs[1]["stats"] == (L - 2, 1)
        for d in DEPTHS:
            if L <= 2 * d + 3:
                assert runs[d]["lazy"] == ((L - 2) // d, (L - 2) // d * d, (L - 2) % d), (d, L)


@pytest.mark.parametrize("mode", MODES)
def test_all_six_modes(mode, monkeypatch):
    runs = all_depths(monkeypatch, mode, "lap40", X.loop(11))
    assert runs[4]["lazy"] == (2, 8, 1) and runs[2]["lazy"] == (4, 8, 1)


@pytest.mark.parametrize("mode,which", [("secded", "arrow"), ("constraints", "holes"), ("sed", "rand"), ("sec7", "lap37x41"),
                                        ("sec8", "one")])
def test_other_modes_on_the_other_row_paths(mode, which, monkeypatch):
    all_depths(monkeypatch, mode, which, X.loop(7))


# ---- something else comes while the queue holds 0 ... d - 1 updates ----
@pytest.mark.parametrize("what", sorted(BETWEEN))
def test_something_else_comes_first(what, monkeypatch):
    mode = "secded" if what == "inject" else "none"
    for d in DEPTHS:
        for fill in range(d):
            L = loop_to_fill(d, fill)
            script = X.loop(L) + [("stats",)] + BETWEEN[what] + [("stats",)] + X.loop(d + 2, first=L)
            runs = all_depths(monkeypatch, mode, "lap40", script)
            first, second = counters(runs[d])[:2]
            assert first == (L - 2, 0) and second == (L - 2, 1)  # the pending one applied on its own, behind the queue
            assert runs[d]["lazy"][2] >= fill


@pytest.mark.parametrize("what", sorted(OTHER_SPMV))
def test_a_different_spmv(what, monkeypatch):
    spmv, second = OTHER_SPMV[what]
    for d in DEPTHS:
        for fill in range(d):
            L = loop_to_fill(d, fill)
            script = (X.loop(L) + spmv + [("stats",), ("dot", "p", "w"), ("calc_xr", 0.4), ("calc_p", 0.55)] +
                      X.loop(d + 1, first=L + 1))
            runs = all_depths(monkeypatch, "none", "lap40", script, second=second)
            assert counters(runs[d])[0] == (L - 2, 1)
            assert runs[d]["lazy"][2] >= fill


@pytest.mark.parametrize("d", DEPTHS)
def test_close_destroy_and_graph_with_a_filled_queue(d, monkeypatch):
    for fill in range(1, d):
        L = loop_to_fill(d, fill)
        env = dict(ABFT_HIP_X_IN_SPMV="1", ABFT_HIP_LAZY_X=str(d))
        # (the counters are read before the context goes: the queue is still held; shutdown applies it, then the
        # pending update, and frees the ring)
        out = play(monkeypatch, env, "none", X.matrix("lap40"), X.loop(L), finish="close")
        assert out["stats"] == (L - 2, 0) and out["lazy"] == ((L - 2) // d, (L - 2) // d * d, 0)
        for tail in ([("destroy", "p"), ("stats",)], [("destroy", "x"), ("stats",)],
                     [("graph",), ("stats",)] + X.loop(3, first=L)):
            runs = all_depths(monkeypatch, "none", "lap40", X.loop(L) + tail)
            assert counters(runs[d])[0] == (L - 2, 1)
            assert runs[d]["lazy"] == (0, 0, fill)


@pytest.mark.parametrize("ahead", ["0", "1", "2"])
@pytest.mark.parametrize("finish", ["0", "1"])
def test_run_ahead_levels_and_deferred_finishes(ahead, finish, monkeypatch):
    """CG's own quotients are what arms the run-ahead; chosen scalars (X.loop) never do, so both kinds are played"""
    env = dict(ABFT_HIP_AHEAD=ahead, ABFT_HIP_DEFER_FINISH=finish)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    runs = all_depths(monkeypatch, "none", "lap40", X.loop(11), extra_env=env)
    assert runs[4]["lazy"] == (2, 8, 1)
    for d in (1,) + DEPTHS:
        for k, v in dict(env, ABFT_HIP_X_IN_SPMV="1", ABFT_HIP_LAZY_X=str(d)).items():
            monkeypatch.setenv(k, v)
        cg = cg_run("lap40", 14)
        if d == 1:
            base = cg
            continue
        assert cg["stats"] == base["stats"] and cg["ahead"] == base["ahead"]
        assert cg["lazy"] == (12 // d, 12 // d * d, 12 % d)
        if ahead != "0":
            assert cg["ahead"][0] > 0  # the calc_p run ahead wrote into the ring's buffers
        for a, b in zip(cg["bits"], base["bits"]):
            assert np.array_equal(a, b)


def cg_run(which, iters, specials=None):
    """the host-scalar loop with CG's own alpha and beta, a fixed number of iterations -> what a caller can see"""
    import abft_sparse_cg_amd as amd
    cols, rows, vals, n = X.matrix(which)
    ctx = amd.HIPContext("none", "csr")
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        x, r, p, w = (ctx.create_vector(n) for _ in range(4))
        rng = np.random.default_rng(7)
        x0, r0 = rng.random(n) - 0.5, rng.random(n) - 0.5
        p0 = r0.copy()
        if specials is not None:
            x0, p0 = specials(x0, p0)
        ctx.upload(x, x0); ctx.upload(r, r0); ctx.upload(p, p0); ctx.upload(w, np.zeros(n))
        scalars = []
        rr = ctx.dot(r, r)
        for _ in range(iters):
            ctx.spmv(A, p, w)
            pw = ctx.dot(p, w)
            with np.errstate(all="ignore"):
                alpha = float(np.float64(rr) / np.float64(pw))
            rr_new = ctx.calc_xr(x, r, p, w, alpha)
            with np.errstate(all="ignore"):
                beta = float(np.float64(rr_new) / np.float64(rr))
            ctx.calc_p(p, r, beta)
            scalars += [pw, rr_new]
            rr = rr_new
        vectors = [ctx.download(v) for v in (x, r, p, w)]
        return dict(bits=[X.bits(np.array(scalars))] + [X.bits(v) for v in vectors], stats=ctx.x_in_spmv_stats(),
                    lazy=ctx.lazy_x_stats(), ahead=ctx.ahead_stats())
    finally:
        ctx.close()


# ---- values on which a padded or reordered chain of updates changes bits ----
def with_specials(x0, p0):
    n = len(x0)
    kinds = [-0.0, _ieee.INF, -_ieee.INF, _ieee.QNAN, _ieee.TINY, -_ieee.MAX_SUB, _ieee.MIN_NORMAL, 0.0]
    x0, p0 = x0.copy(), p0.copy()
    at = np.arange(0, n, 7)
    x0[at] = np.array(kinds)[np.arange(len(at)) % len(kinds)]
    p0[at[::2]] = _ieee.TINY  # alpha * p underflows or stays subnormal beside the special x
    p0[np.signbit(x0) & (x0 == 0.0)] = -0.0  # -0.0 + alpha * -0.0 keeps its sign only if no update of +0 is padded in
    sub = np.arange(3, n, 11)
    p0[sub] = np.array([_ieee.MAX_SUB, -_ieee.TINY, _ieee.MIN_NORMAL])[np.arange(len(sub)) % 3]
    return x0, p0


@pytest.mark.parametrize("which", ["lap40", "arrow", "holes"])
def test_special_values_in_x_and_p(which, monkeypatch):
    """x holds -0.0, infinities, a NaN with a payload and subnormals, p zeros under the -0.0 (the first queued updates
    add -0.0 to -0.0) and subnormals elsewhere; the scalars are chosen, alpha 0 every third time"""
    import abft_sparse_cg_amd as amd
    cols, rows, vals, n = X.matrix(which)
    got = {}
    for name, env in [("off", dict(ABFT_HIP_X_IN_SPMV="0")), (1, dict(ABFT_HIP_X_IN_SPMV="1", ABFT_HIP_LAZY_X="1")),
                      (2, dict(ABFT_HIP_X_IN_SPMV="1", ABFT_HIP_LAZY_X="2")), (4, dict(ABFT_HIP_X_IN_SPMV="1", ABFT_HIP_LAZY_X="4"))]:
        for k in ("ABFT_HIP_X_IN_SPMV", "ABFT_HIP_LAZY_X"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = amd.HIPContext("none", "csr")
        try:
            A = ctx.create_matrix(cols, rows, vals, n, len(vals))
            x, r, p, w = (ctx.create_vector(n) for _ in range(4))
            rng = np.random.default_rng(5)
            x0, p0 = with_specials(rng.random(n) - 0.5, rng.random(n) - 0.5)
            ctx.upload(x, x0); ctx.upload(r, np.zeros(n)); ctx.upload(p, p0); ctx.upload(w, np.zeros(n))
            for j in range(11):
                ctx.spmv(A, p, w)
                ctx.dot(p, w)
                ctx.calc_xr(x, r, p, w, 0.0 if j % 3 == 2 else 0.37 + 0.01 * j)  # (alpha 0 every third time: r stays, x + 0 * p)
                ctx.calc_p(p, r, 1.0 if j % 2 else -0.5)
            got[name] = ([X.bits(ctx.download(v)) for v in (x, r, p, w)], ctx.lazy_x_stats())
        finally:
            ctx.close()
    assert got[4][1] == (2, 8, 1) and got[2][1] == (4, 8, 1) and got[1][1] == (0, 0, 0)
    x_off = got["off"][0][0].view(np.float64)
    assert np.isnan(x_off).any() and np.isinf(x_off).any()  # the specials were still there to be got wrong
    for name in (1, 2, 4):
        for a, b in zip(got[name][0], got["off"][0]):
            assert np.array_equal(a, b), name


# ---- vector lengths ----
def test_two_lengths_taking_turns_and_a_third(monkeypatch):
    """the queue and its spare buffers belong to one length: a pending update of another length finds the queue applied
    first, and the spares follow the length"""
    import abft_sparse_cg_amd as amd
    out = {}
    for name, env in [("off", dict(ABFT_HIP_X_IN_SPMV="0")), (1, dict(ABFT_HIP_X_IN_SPMV="1", ABFT_HIP_LAZY_X="1")),
                      (2, dict(ABFT_HIP_X_IN_SPMV="1", ABFT_HIP_LAZY_X="2")), (4, dict(ABFT_HIP_X_IN_SPMV="1", ABFT_HIP_LAZY_X="4"))]:
        for k in ("ABFT_HIP_X_IN_SPMV", "ABFT_HIP_LAZY_X"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = amd.HIPContext("none", "csr")
        try:
            sets = []
            for which in ("lap40", "lap37x41", "holes"):
                cols, rows, vals, n = X.matrix(which)
                A = ctx.create_matrix(cols, rows, vals, n, len(vals))
                v = [ctx.create_vector(n) for _ in range(4)]
                rng = np.random.default_rng(3)
                for u in v[:3]:
                    ctx.upload(u, rng.random(n) - 0.5)
                ctx.upload(v[3], np.zeros(n))
                sets.append((A, v))
            for turn, at in enumerate([0, 1, 0, 1, 2, 0, 2, 1]):
                A, (x, r, p, w) = sets[at]
                for j in range(4 + turn % 3):  # (the turn ends with 2 + turn % 3 updates taken over: queues of every fill)
                    ctx.spmv(A, p, w)
                    ctx.dot(p, w)
                    ctx.calc_xr(x, r, p, w, 0.3 + 0.01 * j)
                    ctx.calc_p(p, r, 0.5 - 0.01 * j)
            out[name] = ([X.bits(ctx.download(u)) for _, v in sets for u in v], ctx.x_in_spmv_stats(), ctx.lazy_x_stats())
        finally:
            ctx.close()
    assert out["off"][1] == (0, 0) and out[1][1][0] > 0
    for d in DEPTHS:
        assert out[d][1] == out[1][1]
        assert out[d][2][0] > 0 and out[d][2][2] > 0
        for a, b in zip(out[d][0], out["off"][0]):
            assert np.array_equal(a, b)
    for a, b in zip(out[1][0], out["off"][0]):
        assert np.array_equal(a, b)


# ---- the default ----
def test_unset_is_the_named_default(monkeypatch):
    with open(_ieee.INTERNAL_H) as f:
        default = int(re.search(r"#define\s+ABFT_LAZY_X_DEFAULT\s+(\d+)", f.read()).group(1))
    assert default in (1, 2, 4)
    unset = play(monkeypatch, {}, "none", X.matrix("lap40"), X.loop(11))
    named = play(monkeypatch, dict(ABFT_HIP_LAZY_X=str(default)), "none", X.matrix("lap40"), X.loop(11))
    assert unset["stats"] == named["stats"] == (9, 1) and unset["lazy"] == named["lazy"]
    assert unset["lazy"] == ((9 // default, 9 // default * default, 9 % default) if default > 1 else (0, 0, 0))
    X.same(unset, named)
    other_mode = play(monkeypatch, dict(ABFT_HIP_LAZY_X="4"), "secded", X.matrix("lap40"), X.loop(11))
    assert other_mode["stats"] == (0, 0) and other_mode["lazy"] == (0, 0, 0)  # no pending path on this mode: no queue
