"""Jacobi preconditioning: what it costs per iteration and what it saves in time to solution
(DESIGN.md section 5d).

  * per-iteration cost: the Python cg_solve loop, -c 0, a fixed number of iterations, plain and with
    precond=jacobi(A), alternating in one process, one solve each per block; the median over the blocks
    of the time per iteration, and their ratio.  The deferred x update is left on.  Cases: config 2's
    matrix (laplace5:3162,3162, CSR, none and secded) and config 5's (powerlaw:2097152,2, COO sec7);
  * time to solution on config 5's matrix at thresholds 1e-3 and 1e-10: iterations and wall time of
    plain CG and of PCG (the jacobi call included), alternating, median over the blocks;
  * `--kernels M`: instead, M calls each of precond_start, calc_xr_precond and calc_p_precond on
    vectors of config 2's length (for a `rocprofv3 --kernel-trace --stats` run of its own), their rates
    by HIP-event brackets, and ctx.stream_probe's bandwidth on the same device.

    python tools/precond_bench.py --out profiles/r08/precond_bench.json [--iters 200] [--blocks 5]

One JSON file; a line per measurement on stdout as it goes.  Measurement only: nothing here is
checked (tests/test_gpu_precond.py is the check).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import abft_sparse_cg_amd as amd  # noqa: E402
from abft_sparse_cg_amd import capi, generators  # noqa: E402

CASES = [("config2", "laplace5:3162,3162", "csr", "none"), ("config2", "laplace5:3162,3162", "csr", "secded"),
         ("config5", "powerlaw:2097152,2", "coo", "sec7")]
SOLVE_CASE = ("config5", "powerlaw:2097152,2", "coo", "sec7")


def timed_solve(ctx, A, vecs, n, its, conv, dinv):
    ctx.upload(vecs[1], np.zeros(n))
    ctx.synchronize()
    t0 = time.perf_counter()
    it, rr = amd.cg_solve(ctx, A, *vecs, max_itrs=its, conv_threshold=conv, precond=dinv)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, it, rr


def loop_times(ctx, A, n, iters, blocks):
    """-> (ms per iteration plain, with Jacobi, the blocks): medians over `blocks` alternating pairs"""
    vecs = [ctx.create_vector(n) for _ in range(5)]
    ctx.upload(vecs[0], generators.reference_rhs(n))
    dinv = ctx.jacobi(A)
    for d in (None, dinv):
        timed_solve(ctx, A, vecs, n, 5, 0.0, d)
    per = {"cg": [], "pcg": []}
    for _ in range(blocks):
        for name, d in (("cg", None), ("pcg", dinv)):
            per[name].append(timed_solve(ctx, A, vecs, n, iters, 0.0, d)[0] / iters)
    for v in vecs + [dinv]:
        ctx.destroy_vector(v)
    return statistics.median(per["cg"]), statistics.median(per["pcg"]), per


def solve_times(ctx, A, n, conv, blocks):
    """time to solution: -> dict with iterations and median wall ms of CG and PCG (jacobi() included)"""
    vecs = [ctx.create_vector(n) for _ in range(5)]
    ctx.upload(vecs[0], generators.reference_rhs(n))
    out = {"cg": [], "pcg": []}
    its = {}
    for b in range(blocks + 1):  # the first pair warms up
        ms, its["cg"], rr_cg = timed_solve(ctx, A, vecs, n, 5000, conv, None)
        t0 = time.perf_counter()
        dinv = ctx.jacobi(A)
        ms_j = (time.perf_counter() - t0) * 1e3
        ms_p, its["pcg"], rr_pcg = timed_solve(ctx, A, vecs, n, 5000, conv, dinv)
        ctx.destroy_vector(dinv)
        if b:
            out["cg"].append(ms)
            out["pcg"].append(ms_p + ms_j)
    for v in vecs:
        ctx.destroy_vector(v)
    return dict(threshold=conv, cg_iterations=its["cg"], pcg_iterations=its["pcg"], cg_ms=statistics.median(out["cg"]),
                pcg_ms=statistics.median(out["pcg"]), jacobi_ms_last=ms_j, cg_rr=rr_cg, pcg_rr=rr_pcg,
                blocks_cg=out["cg"], blocks_pcg=out["pcg"])


def kernel_rates(ctx, n, calls):
    """M calls of each kernel under HIP-event brackets -> GB/s by the bytes each moves"""
    x, r, p, w, d = (ctx.create_vector(n) for _ in range(5))
    for v, seed in ((x, 2), (r, 3), (p, 4), (w, 5)):
        ctx.upload(v, generators.reference_rhs(n, seed=seed))
    ctx.upload(d, 0.5 + generators.reference_rhs(n, seed=6))
    rows = []
    # bytes per entry: start reads r, dinv, writes p; the r half reads r, w, dinv, writes r; calc_p_precond with
    # the deferred x half reads p, r, dinv, x and writes p, x
    for name, kid, nbytes, before, call in (
            ("precond_start", capi.K_DOT, 24, None, lambda: ctx.precond_start(r, d, p)),
            ("calc_xr_precond (r half)", capi.K_CALC_XR, 32, None, lambda: ctx.calc_xr_precond(x, r, p, w, d, 1e-9)),
            ("calc_p_precond (+ x half)", capi.K_CALC_P, 48, lambda: ctx.calc_xr_precond(x, r, p, w, d, 1e-9),
             lambda: ctx.calc_p_precond(p, r, d, 0.5))):
        ctx.profile(1 << kid)  # brackets this kernel's launches only: `before` (another kernel id) runs unbracketed
        for _ in range(calls):
            if before:
                before()  # leaves the x half for the call that is timed
            call()
        ms, launches = ctx.profile_read(kid)
        ctx.profile(0)
        us = ms * 1e3 / max(launches, 1)
        rows.append(dict(kernel=name, us=us, launches=launches, bytes_per_entry=nbytes,
                         gbps=nbytes * n / (us * 1e-6) / 1e9 if us else None))
    ctx.synchronize()
    for v in (x, r, p, w, d):
        ctx.destroy_vector(v)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="precond_bench.json")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--kernels", type=int, default=0, help="M calls of each preconditioned kernel instead of the loops")
    ap.add_argument("--skip-solves", action="store_true", help="per-iteration costs only")
    a = ap.parse_args()
    argv = [v for i, v in enumerate(sys.argv) if v != "--out" and (i == 0 or sys.argv[i - 1] != "--out")]
    res = {"cmd": " ".join(argv), "iters": a.iters, "blocks": a.blocks, "rows": []}

    def emit(row):
        res["rows"].append(row)
        print(json.dumps(row), flush=True)

    if a.kernels:
        n = generators.dim(CASES[0][1])
        ctx = amd.HIPContext("none", "csr")
        for row in kernel_rates(ctx, n, a.kernels):
            emit(dict(row, n=n))
        copy_gbps, read_gbps = ctx.stream_probe()
        emit(dict(stream_probe_copy_gbps=copy_gbps, stream_probe_read_gbps=read_gbps))
        ctx.close()
    else:
        mats = {}
        for config, spec, fmt, mode in CASES:
            if spec not in mats:
                mats = {spec: generators.generate(spec)}
            cols, rows, vals, n = mats[spec]
            ctx = amd.HIPContext(mode, fmt, on_event=lambda ev, fatal: None)
            A = ctx.create_matrix(cols, rows, vals, n, len(vals))
            cg, pcg, per = loop_times(ctx, A, n, a.iters, a.blocks)
            emit(dict(config=config, spec=spec, fmt=fmt, mode=mode, n=n, nnz=len(vals), layout=ctx.matrix_info(A)[0],
                      ms_per_iter_cg=cg, ms_per_iter_pcg=pcg, ratio=pcg / cg, blocks_cg=per["cg"], blocks_pcg=per["pcg"]))
            if not a.skip_solves and (config, spec, fmt, mode) == SOLVE_CASE:
                for conv in (1e-3, 1e-10):
                    emit(dict(solve_times(ctx, A, n, conv, a.blocks), config=config, spec=spec, fmt=fmt, mode=mode, n=n))
            ctx.destroy_matrix(A)
            ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
