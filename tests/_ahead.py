"""Helper of test_gpu_ahead.py: the host-scalar CG loop played over the C ABI with alpha and beta formed from the
scalars handed back (the fixed-alpha scripts of _x_in_spmv.py never arm the run-ahead), once per level of
ABFT_HIP_AHEAD.

A script is a list of iterations.  An iteration is a dict (all keys optional):
    alpha_ulps, beta_ulps   hand in the quotient moved by that many ulps (nextafter)
    before_xr, before_p     extra steps between spmv / dot(p, w) and calc_xr, between calc_xr and calc_p
An extra step is a tuple: ("download", v), ("upload", v), ("copy", dst, src), ("view", v), ("ptr", v), ("graph",),
("calc_xr",) (the same call once more), ("calc_p", p, r) (calc_p on these two first), ("destroy", v) and ("close",),
which both end the script where they stand.  Vectors are named x, r, p, w and the spare q.

`run` returns what a caller can observe -- every scalar handed back, the vectors downloaded at the end, the drained
events -- and the counters of abft_hip_ahead_stats and abft_hip_x_in_spmv_stats."""
import numpy as np

from _x_in_spmv import bits, matrix, same  # noqa: F401  (same: re-exported for the tests)
from abft_sparse_cg_amd.context import fdiv


def predicted(k):
    return [{} for _ in range(k)]


def ulps(v, k):
    for _ in range(abs(k)):
        v = float(np.nextafter(v, np.inf if k > 0 else -np.inf))
    return v


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


def run(amd, mode, mat, script):
    cols, rows, vals, n = mat
    events = []
    ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: events.extend((k, i, b, fatal) for k, i, b in ev))
    out = {"scalars": []}
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        assert ctx.matrix_info(A)[0] == "stream"
        V = {name: ctx.create_vector(n) for name in "xrpwq"}
        rng = np.random.default_rng(11)
        ctx.upload(V["x"], np.zeros(n))
        rhs = rng.random(n) + 0.5
        ctx.upload(V["r"], rhs)
        ctx.upload(V["p"], rhs)
        ctx.upload(V["w"], np.zeros(n))
        ctx.upload(V["q"], rng.random(n) - 0.5)
        views = []
        closed = False
        try:
            play(ctx, A, V, n, script, out, views)
        except _Stop:
            closed = any(s == ("close",) for it in script for k in ("before_xr", "before_p") for s in it.get(k, ()))
        if not closed:
            out["vectors"] = {c: ctx.download(V[c]) for c in "xrpwq" if c in V}
            ctx._drain()
        out["ahead"] = ctx.ahead_stats()
        out["xin"] = ctx.x_in_spmv_stats()
        out["events"] = list(events)
    finally:
        ctx.close()
    return out


def levels(amd, monkeypatch, mode, mat, script):
    """the script at ABFT_HIP_AHEAD=0, 1, 2 -> the three results, equal in every bit a caller can see"""
    res = []
    for level in "012":
        monkeypatch.setenv("ABFT_HIP_AHEAD", level)
        res.append(run(amd, mode, mat, script))
    assert res[0]["ahead"] == (0, 0, 0)
    same(res[1], res[0])
    same(res[2], res[0])
    return res
