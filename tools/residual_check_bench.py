"""Residual checks: what check_every costs the CG loop ("Residual checks with rollback").

On config 2's matrix (laplace5:3162,3162), for the modes none and secded:

  * the Python cg_solve loop, -c 0, a fixed number of iterations, with check_every=0 and with
    check_every=N, alternating, one solve each per block; the median over the blocks of the time per
    iteration, and their ratio.  The checkpoint vector is made once and passed in (x_ckpt), as a
    caller that solves repeatedly would;
  * the same for cg_solve_block at K columns on the streaming layout;
  * `--kernels M`: instead of the loops, M calls each of residual_gap, residual_restart and their
    block forms (for a `rocprofv3 --kernel-trace --stats` run of its own), and ctx.stream_probe's
    read bandwidth on the same device;
  * `--gaps`: instead, the clean gap ||b - A x - r|| / ||b|| after every iteration of configs 2, 4 and
    5 (their matrix, format and mode; -c 0, --iters iterations), its largest value over the run and
    its value at the end -- what the default check_tol has to sit above.

    python tools/residual_check_bench.py --out profiles/r06/residual_check_bench.json [--iters 200] [--every 50]

One JSON file; a line per measurement on stdout as it goes.  Measurement only: nothing here is
checked (tests/test_gpu_residual_check.py is the check).
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
from abft_sparse_cg_amd import generators  # noqa: E402

SPEC = "laplace5:3162,3162"
GAP_CONFIGS = {"config2": ("laplace5:3162,3162", "csr", "secded"), "config4": ("random:4194304,24,1", "csr", "secded"),
               "config5": ("powerlaw:2097152,2", "coo", "sec7")}


def loop_times(ctx, A, n, k, iters, every, blocks):
    """-> (ms per iteration without checks, with checks): medians over `blocks` alternating pairs"""
    make = (lambda: ctx.create_vector(n)) if k == 1 else (lambda: ctx.create_block(n, k))
    vecs = [make() for _ in range(5)]
    ckpt = make()
    if k == 1:
        ctx.upload(vecs[0], generators.reference_rhs(n))
        solve, zero = amd.cg_solve, np.zeros(n)
    else:
        ctx.upload(vecs[0], np.stack([generators.reference_rhs(n, seed=1 + j) for j in range(k)], axis=1))
        solve, zero = amd.cg_solve_block, np.zeros((n, k))

    def run(ce, its):
        ctx.upload(vecs[1], zero)
        ctx.synchronize()
        t0 = time.perf_counter()
        solve(ctx, A, *vecs, max_itrs=its, conv_threshold=0.0, check_every=ce, x_ckpt=ckpt)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / its

    run(0, 5)
    run(every, 5)
    per = {0: [], every: []}
    for _ in range(blocks):
        for ce in (0, every):
            per[ce].append(run(ce, iters))
    for v in vecs + [ckpt]:
        ctx.destroy_vector(v)
    return statistics.median(per[0]), statistics.median(per[every]), per


def kernel_calls(ctx, A, n, calls, k):
    b, x, r, p, w = (ctx.create_vector(n) for _ in range(5))
    ctx.upload(b, generators.reference_rhs(n))
    ctx.upload(x, generators.reference_rhs(n, seed=2))
    for _ in range(calls):
        ctx.residual_gap(A, b, x, r, w)
        ctx.residual_restart(A, b, x, r, p, w)
    B, X, R, P, W = (ctx.create_block(n, k) for _ in range(5))
    ctx.upload(B, np.stack([generators.reference_rhs(n, seed=1 + j) for j in range(k)], axis=1))
    mask = (1 << k) - 1
    for _ in range(calls):
        ctx.residual_gap_block(A, B, X, R, W, k, mask)
        ctx.residual_restart_block(A, B, X, R, P, W, k, mask)
        ctx.copy_block(X, P, k, mask)
    ctx.synchronize()
    for v in (b, x, r, p, w, B, X, R, P, W):
        ctx.destroy_vector(v)


def clean_gaps(name, iters):
    spec, fmt, mode = GAP_CONFIGS[name]
    cols, rows, vals, n = generators.generate(spec)
    ctx = amd.HIPContext(mode, fmt, on_event=lambda ev, fatal: None)
    A = ctx.create_matrix(cols, rows, vals, n, len(vals))
    del cols, rows, vals
    b, x, r, p, w = (ctx.create_vector(n) for _ in range(5))
    bh = generators.reference_rhs(n)
    ctx.upload(b, bh)
    ctx.upload(x, np.zeros(n))
    bnorm = float(np.linalg.norm(bh))
    gaps = []
    # a tolerance nothing fails: every gap is recorded, nothing is rolled back
    amd.cg_solve(ctx, A, b, x, r, p, w, iters, 0.0, check_every=1, check_tol=1e100,
                 on_check=lambda i, gap, ok, back: gaps.append(gap / bnorm))
    ctx.close()
    return dict(config=name, spec=spec, fmt=fmt, mode=mode, n=n, iters=iters, max_gap_over_b=max(gaps),
                last_gap_over_b=gaps[-1], first_gap_over_b=gaps[0], checks=len(gaps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="residual_check_bench.json")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--every", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--modes", default="none,secded")
    ap.add_argument("--kernels", type=int, default=0, help="M calls of each check kernel instead of the loops")
    ap.add_argument("--gaps", action="store_true", help="clean gaps of configs 2, 4, 5 instead of the loops")
    a = ap.parse_args()
    argv = [v for i, v in enumerate(sys.argv) if v != "--out" and (i == 0 or sys.argv[i - 1] != "--out")]
    res = {"cmd": " ".join(argv), "spec": SPEC, "iters": a.iters, "every": a.every, "blocks": a.blocks, "k": a.k,
           "rows": []}
    if a.gaps:
        for name in GAP_CONFIGS:
            row = clean_gaps(name, a.iters)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        a.modes = ""
    else:
        cols, rows, vals, n = generators.generate(SPEC)
        nnz = len(vals)
    for mode in filter(None, a.modes.split(",")):
        ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: None)
        A = ctx.create_matrix(cols, rows, vals, n, nnz, layout="stream")
        if a.kernels:
            kernel_calls(ctx, A, n, a.kernels, a.k)
            copy_gbps, read_gbps = ctx.stream_probe()
            row = dict(mode=mode, n=n, nnz=nnz, kernel_calls=a.kernels, stream_probe_copy_gbps=copy_gbps,
                       stream_probe_read_gbps=read_gbps)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        else:
            for k in (1, a.k):
                off, on, per = loop_times(ctx, A, n, k, a.iters, a.every, a.blocks)
                row = dict(mode=mode, k=k, n=n, nnz=nnz, ms_per_iter_no_checks=off, ms_per_iter_checks=on,
                           ratio=on / off, blocks_no_checks=per[0], blocks_checks=per[a.every])
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
        ctx.destroy_matrix(A)
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
