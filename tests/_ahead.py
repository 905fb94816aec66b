"""Helper of test_gpu_ahead.py: the host-scalar CG loop played over the C ABI with alpha and beta formed from the
scalars handed back (the fixed-alpha scripts of _x_in_spmv.py never arm the run-ahead), once per level of
ABFT_HIP_AHEAD.

A script is a list of iterations.  An iteration is a dict (all keys optional):
    alpha_ulps, beta_ulps   hand in the quotient moved by that many ulps (nextafter)
    before_xr, before_p     extra steps between spmv / dot(p, w) and calc_xr, between calc_xr and calc_p
    before_spmv             extra steps in front of the iteration
An extra step is a tuple: ("download", v), ("upload", v), ("copy", dst, src), ("view", v), ("ptr", v), ("graph",),
("calc_xr",) (the same call once more), ("calc_p", p, r) (calc_p on these two first), ("dot", a, b), ("drain",),
("synchronize",), ("residual_gap",) (b = q, scratch s), ("inject", element, bits), ("spmv", src, dst), ("destroy", v)
and ("close",), which both end the script where they stand.  Vectors are named x, r, p, w and the spares q and s.

`run_turns` plays several solves in one context, taking turns (`turns`: [(solve, calls)], `calls` of the loop's four
calls of that solve next); `model_holds` holds what `run` or `run_turns` read against numpy and the oracle.

`run` returns what a caller can observe -- every scalar handed back, the vectors downloaded at the end (and what the
views made on the way show), the drained events -- and the counters of abft_hip_ahead_stats, abft_hip_x_in_spmv_stats
and abft_hip_speculation_stats."""
import ctypes as C

import numpy as np

from _loop_scripts import expected, predicted, ulps  # noqa: F401  (they live where a test without a GPU can import them)
from _x_in_spmv import bits, matrix, same  # noqa: F401  (same: re-exported for the tests)
from abft_sparse_cg_amd.context import fdiv


class _Stop(Exception):
    pass


def _extra(ctx, V, views, step, n, alpha, beta, out):
    op = step[0]
    if op == "download":
        out["scalars"].append(ctx.download(V[step[1]]))
    elif op == "upload":
        ctx.upload(V[step[1]], np.linspace(-1.0, 1.0, n))
    elif op == "copy":
        ctx.copy_vector(V[step[1]], V[step[2]])
    elif op == "view":
        views.append(ctx.view_vector(V[step[1]], 0, n))
    elif op == "ptr":
        assert V[step[1]].device_ptr
    elif op == "graph":  # capture one copy, replay it once
        ctx.graph_begin()
        ctx.copy_vector(V["q"], V["w"])
        graph = ctx.graph_end()
        ctx.graph_launch(graph)
        ctx.synchronize()
        ctx.graph_destroy(graph)
    elif op == "calc_xr":
        out["scalars"].append(ctx.calc_xr(V["x"], V["r"], V["p"], V["w"], alpha))
    elif op == "calc_p":
        ctx.calc_p(V[step[1]], V[step[2]], 0.5 if beta is None else beta)
    elif op == "dot":
        out["scalars"].append(ctx.dot(V[step[1]], V[step[2]]))
    elif op == "drain":
        ctx._drain()
    elif op == "synchronize":
        ctx.synchronize()
    elif op == "residual_gap":
        out["scalars"] += list(ctx.residual_gap(V["A"], V["q"], V["x"], V["r"], V["s"]))
    elif op == "inject":
        ctx.inject_at(V["A"], step[1], list(step[2]))
    elif op == "spmv":
        ctx.spmv(V["A"], V[step[1]], V[step[2]])
    elif op == "destroy":
        ctx.destroy_vector(V.pop(step[1]))
        raise _Stop
    elif op == "close":
        raise _Stop
    else:
        raise ValueError(op)


def play(ctx, A, V, n, script, out, views):
    """the loop of the reference driver: rr = r.r, then per iteration spmv, dot, calc_xr, calc_p"""
    rr = ctx.dot(V["r"], V["r"])
    out["scalars"].append(rr)
    for it in script:
        for step in it.get("before_spmv", ()):
            _extra(ctx, V, views, step, n, None, None, out)
        ctx.spmv(A, V["p"], V["w"])
        pw = ctx.dot(V["p"], V["w"])
        alpha = ulps(fdiv(rr, pw), it.get("alpha_ulps", 0))
        out["scalars"] += [pw, alpha]
        for step in it.get("before_xr", ()):
            _extra(ctx, V, views, step, n, alpha, None, out)
        rr_new = ctx.calc_xr(V["x"], V["r"], V["p"], V["w"], alpha)
        beta = ulps(fdiv(rr_new, rr), it.get("beta_ulps", 0))
        out["scalars"] += [rr_new, beta]
        for step in it.get("before_p", ()):
            _extra(ctx, V, views, step, n, alpha, beta, out)
        ctx.calc_p(V["p"], V["r"], beta)
        rr = rr_new


def spec_stats(ctx):
    from abft_sparse_cg_amd import capi
    t, d = C.c_long(), C.c_long()
    capi.check(ctx.L.abft_hip_speculation_stats(ctx.h, C.byref(t), C.byref(d)))
    return t.value, d.value


def start_vectors(n, scale=1.0, seed=11):
    """what `run` uploads: x, r = p = the right-hand side, w, the spares q and s (run_turns: seed 11 + k for solve k)"""
    rng = np.random.default_rng(seed)
    rhs = scale * (rng.random(n) + 0.5)
    return {"x": np.zeros(n), "r": rhs, "p": rhs.copy(), "w": np.zeros(n), "q": scale * (rng.random(n) - 0.5), "s": np.zeros(n)}


def run(amd, mode, mat, script, scale=1.0):
    cols, rows, vals, n = mat
    events = []
    ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: events.extend((k, i, b, fatal) for k, i, b in ev))
    out = {"scalars": []}
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        assert ctx.matrix_info(A)[0] == "stream"
        V = {name: ctx.create_vector(n) for name in "xrpwqs"}
        for name, v in start_vectors(n, scale).items():
            ctx.upload(V[name], v)
        V["A"] = A
        views = []
        closed = False
        try:
            play(ctx, A, V, n, script, out, views)
        except _Stop:
            closed = any(s == ("close",) for it in script for k in ("before_xr", "before_p") for s in it.get(k, ()))
        if not closed:
            out["vectors"] = {c: ctx.download(V[c]) for c in "xrpwqs" if c in V}
            out["views"] = [ctx.download(v) for v in views]
            ctx._drain()
        out["ahead"] = ctx.ahead_stats()
        out["xin"] = ctx.x_in_spmv_stats()
        out["spec"] = spec_stats(ctx)
        out["events"] = list(events)
    finally:
        ctx.close()
    return out


def run_turns(amd, mode, mats, turns, scale=1.0):
    """several solves in one context: solve k on mats[k] with start_vectors of its length; r.r of every solve first,
    then `turns`.  -> as `run`, the vectors named x0, r0, ... and the scalars in the order they were handed back"""
    events = []
    ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: events.extend((k, i, b, fatal) for k, i, b in ev))
    out = {"scalars": []}
    try:
        S = []
        for k, (cols, rows, vals, n) in enumerate(mats):
            A = ctx.create_matrix(cols, rows, vals, n, len(vals))
            assert ctx.matrix_info(A)[0] == "stream"
            V = {name: ctx.create_vector(n) for name in "xrpw"}
            for name in "xrpw":
                ctx.upload(V[name], start_vectors(n, scale, 11 + k)[name])
            S.append(dict(A=A, V=V, at=0))
        for v in S:
            v["rr"] = ctx.dot(v["V"]["r"], v["V"]["r"])
            out["scalars"].append(v["rr"])
        for k, calls in turns:
            v = S[k]
            A, V = v["A"], v["V"]
            for _ in range(calls):
                if v["at"] == 0:
                    ctx.spmv(A, V["p"], V["w"])
                elif v["at"] == 1:
                    v["pw"] = ctx.dot(V["p"], V["w"])
                    out["scalars"].append(v["pw"])
                elif v["at"] == 2:
                    v["alpha"] = fdiv(v["rr"], v["pw"])
                    v["rr_new"] = ctx.calc_xr(V["x"], V["r"], V["p"], V["w"], v["alpha"])
                    out["scalars"] += [v["alpha"], v["rr_new"]]
                else:
                    v["beta"] = fdiv(v["rr_new"], v["rr"])
                    ctx.calc_p(V["p"], V["r"], v["beta"])
                    out["scalars"].append(v["beta"])
                    v["rr"] = v["rr_new"]
                v["at"] = (v["at"] + 1) % 4
        out["vectors"] = {"%s%d" % (c, k): ctx.download(v["V"][c]) for k, v in enumerate(S) for c in "xrpw"}
        ctx._drain()
        out["ahead"] = ctx.ahead_stats()
        out["xin"] = ctx.x_in_spmv_stats()
        out["events"] = list(events)
    finally:
        ctx.close()
    return out


def model_turns_hold(mode, mats, turns, res, scale=1.0):
    """`run_turns` again in numpy -- w = the oracle's SpMV, x + alpha * p, r - alpha * w, r + beta * p, a multiply and an
    add each, with the alpha and beta the run handed in: the vectors at the end in every bit (a NaN matches a NaN), the
    sums handed back within 1e-12 of the sum of the magnitudes of their terms (not when those are subnormal)"""
    from _ieee import ieee_equal
    from _oracle import CSR, OracleMatrix
    got = iter(res["scalars"])
    held = scale * scale > 1e-290  # (below that r.r and p.w are subnormal: no relative precision to hold them to)

    def close(value, a, b):
        with np.errstate(all="ignore"):
            want, tol = np.dot(a, b), 1e-12 * np.abs(a * b).sum()
        assert not (held and np.isfinite(want)) or abs(value - want) <= tol, (value, float(want), float(tol))

    S = []
    for k, (cols, rows, vals, n) in enumerate(mats):
        S.append(dict(o=OracleMatrix(CSR, mode, cols, rows, vals, n), M=start_vectors(n, scale, 11 + k), at=0))
    for v in S:
        close(next(got), v["M"]["r"], v["M"]["r"])
    with np.errstate(all="ignore"):
        for k, calls in turns:
            v = S[k]
            M = v["M"]
            for _ in range(calls):
                if v["at"] == 0:
                    M["w"] = v["o"].spmv(M["p"])
                    assert v["o"].events() == ([], False)
                elif v["at"] == 1:
                    close(next(got), M["p"], M["w"])
                elif v["at"] == 2:
                    alpha = next(got)
                    M["x"] = M["x"] + alpha * M["p"]
                    M["r"] = M["r"] - alpha * M["w"]
                    close(next(got), M["r"], M["r"])
                else:
                    M["p"] = M["r"] + next(got) * M["p"]
                v["at"] = (v["at"] + 1) % 4
    for k, v in enumerate(S):
        for c in "xrpw":
            assert ieee_equal(res["vectors"]["%s%d" % (c, k)], v["M"][c]), (c, k)
        v["o"].close()


def model_holds(mode, mat, k, res, scale=1.0):
    """the predicted loop of k iterations that `run` played, against the numpy model"""
    names = {"%s0" % c: res["vectors"][c] for c in "xrpw"}
    model_turns_hold(mode, [mat], [(0, 4 * k)], dict(scalars=res["scalars"], vectors=names), scale)


def levels(amd, monkeypatch, mode, mat, script, run=run, **kw):
    """the script at ABFT_HIP_AHEAD=0, 1, 2 -> the three results, equal in every bit a caller can see"""
    res = []
    for level in "012":
        monkeypatch.setenv("ABFT_HIP_AHEAD", level)
        res.append(run(amd, mode, mat, script, **kw))
    assert res[0]["ahead"] == (0, 0, 0)
    same(res[1], res[0])
    same(res[2], res[0])
    return res
