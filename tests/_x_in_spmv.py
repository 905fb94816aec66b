"""Helper of test_gpu_x_in_spmv.py: call scripts over the C ABI, run once per setting of ABFT_HIP_X_IN_SPMV.

A script is a list of steps.  A step is a tuple (name, arguments...); the vectors are named by letters:
x, r, p, w the loop's four, q a spare of the same length.  `run` plays a script on a fresh context and returns
everything a caller can observe: the scalars handed back, the downloaded vectors, the drained events and
(absorbed, flushed) of abft_hip_x_in_spmv_stats.  With peek=True it also downloads x, r and p around every calc_xr
and calc_p (which applies whatever is pending: a run of its own, only ever used with the switch off) so that the
test can hold x and p against the numpy formulas step by step."""
import numpy as np

from _matrices import MATRICES, arrow, diagonal, every_third_row_empty, matrix, one_by_one  # noqa: F401  (the matrices: tests/_matrices.py)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def loop(k, first=0):
    """k iterations of the host-scalar loop with chosen alpha and beta (no CG: nothing needs to converge)"""
    steps = []
    for j in range(first, first + k):
        steps += [("spmv", "A", "p", "w"), ("dot", "p", "w"), ("calc_xr", 0.37 + 0.01 * j), ("calc_p", 0.61 - 0.02 * j)]
    return steps


def run(amd, mode, mat, script, peek=False, p_view=False, expose=(), second=None, finish="download"):
    """-> dict(scalars, vectors, events, stats, peeks).  second: (fmt, env, value) makes matrix B from the same
    triplets -- in the other format, or with an environment variable set while it is created.  finish: 'download'
    (x, r, p, w, q at the end), 'close' (stop where the script stops)."""
    import os
    from abft_sparse_cg_amd import capi
    cols, rows, vals, n = mat
    events = []
    ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: events.extend((k, i, b, fatal) for k, i, b in ev))
    try:
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        assert ctx.matrix_info(A)[0] == "stream"
        mats = {"A": A}
        if second:
            fmt, env, value = second
            old = os.environ.get(env) if env else None
            if env:
                os.environ[env] = value
            ctx.fmt = capi.FMT_COO if fmt == "coo" else capi.FMT_CSR
            try:
                mats["B"] = ctx.create_matrix(cols, rows, vals, n, len(vals))
            finally:
                ctx.fmt = capi.FMT_CSR
                if env:
                    if old is None:
                        del os.environ[env]
                    else:
                        os.environ[env] = old
            if env:
                assert ctx.matrix_info(mats["B"])[0] == value
        V = {}
        if p_view:  # p is the front of a longer allocation
            V["P"] = ctx.create_vector(n + 6)
            ctx.upload(V["P"], np.zeros(n + 6))
            V["p"] = ctx.view_vector(V["P"], 0, n)
        for name in "xrpwq":
            if name not in V:
                V[name] = ctx.create_vector(n)
        rng = np.random.default_rng(11)
        for name in "xrp":
            ctx.upload(V[name], rng.random(n) - 0.5)
        ctx.upload(V["w"], np.zeros(n))
        ctx.upload(V["q"], rng.random(n) - 0.5)
        for name in expose:
            assert V[name].device_ptr
        out = {"scalars": [], "peeks": []}
        graph = None

        def snap():
            return tuple(ctx.download(V[c]) for c in "xrp")

        for step in script:
            op = step[0]
            if op == "spmv":
                ctx.spmv(mats[step[1]], V[step[2]], V[step[3]])
            elif op == "dot":
                out["scalars"].append(ctx.dot(V[step[1]], V[step[2]]))
            elif op == "calc_xr":
                before = snap() if peek else None
                out["scalars"].append(ctx.calc_xr(V["x"], V["r"], V["p"], V["w"], step[1]))
                if peek:
                    out["peeks"].append(("calc_xr", step[1], before, snap()))
            elif op == "calc_p":
                before = snap() if peek else None
                ctx.calc_p(V["p"], V["r"], step[1])
                if peek:
                    out["peeks"].append(("calc_p", step[1], before, snap()))
            elif op == "download":
                out["scalars"].append(bits(ctx.download(V[step[1]])).sum(dtype=np.uint64))
            elif op == "upload":
                ctx.upload(V[step[1]], np.linspace(-1.0, 1.0, n))
            elif op == "copy":
                ctx.copy_vector(V[step[1]], V[step[2]])
            elif op == "inject":
                ctx.inject_at(mats[step[1]], step[2], step[3])
            elif op == "destroy":
                ctx.destroy_vector(V.pop(step[1]))
            elif op == "stats":
                out["scalars"].append(ctx.x_in_spmv_stats())
            elif op == "graph":  # capture one copy, replay it once
                ctx.graph_begin()
                ctx.copy_vector(V["q"], V["r"])
                graph = ctx.graph_end()
                ctx.graph_launch(graph)
                ctx.synchronize()
                ctx.graph_destroy(graph)
            else:
                raise ValueError(op)
        if finish == "download":
            out["vectors"] = {c: ctx.download(V[c]) for c in "xrpwq" if c in V}
            ctx._drain()
        out["stats"] = ctx.x_in_spmv_stats()
        out["events"] = list(events)
    finally:
        ctx.close()
    return out


def same(a, b):
    """everything a caller can see, bit for bit"""
    assert len(a["scalars"]) == len(b["scalars"])
    for s, t in zip(a["scalars"], b["scalars"]):
        if isinstance(s, tuple):
            continue  # the counters are what differs
        assert np.array_equal(bits(s), bits(t)), (s, t)
    assert a["events"] == b["events"], (a["events"][:4], b["events"][:4])
    assert a.get("vectors", {}).keys() == b.get("vectors", {}).keys()
    for c in a.get("vectors", {}):
        assert np.array_equal(bits(a["vectors"][c]), bits(b["vectors"][c])), c


def formulas_hold(peeked):
    """x + alpha * p and r + beta * p, a separate multiply and add each, at every calc_xr and calc_p"""
    assert peeked["peeks"]
    for op, s, (x0, r0, p0), (x1, r1, p1) in peeked["peeks"]:
        if op == "calc_xr":
            assert np.array_equal(bits(x1), bits(x0 + s * p0))
            assert np.array_equal(bits(p1), bits(p0))
        else:
            assert np.array_equal(bits(p1), bits(r0 + s * p0))
            assert np.array_equal(bits(x1), bits(x0)) and np.array_equal(bits(r1), bits(r0))
