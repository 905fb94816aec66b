"""The device-scalar loop with a stop test against the host-scalar loop.

cg_solve and cg_solve_device alternating in one process: max_itrs = 200 and a threshold of 1e-300, so that every
iteration is live and both loops run the same 200 iterations; one solve each per block (the device loop once per
stride), the median over the blocks of the time per iteration, and the ratio device / host.  Matrices:
laplace5:3162,3162 (config 2, 10 M rows), laplace5:1000,1000 and laplace5:316,316, all CSR `none`.  Strides 4, 8,
16 and 32.  The host loop is the yardstick: this feature does not touch it.

    python tools/device_loop_bench.py --out profiles/device_loop_bench.json [--iters 200] [--blocks 5]
                                      [--specs laplace5:1000,1000,...] [--strides 4,8,16,32]
                                      [--precond jacobi]

--precond jacobi alternates cg_solve(precond=dinv) and cg_solve_device(precond=dinv) instead,
dinv = ctx.jacobi(A); the JSON says so under `precond`, in the file and in every row.  The yardstick is then
cg_solve(precond=) of the same build.

Also reported per matrix: `best_stride`, the smallest stride within 2 % of the best device-loop time (what
DEFAULT_STRIDE is to be on the 1 M-row matrix), and `frozen_spmv_worst`, stride - 1: the SpMVs a solve can waste
behind convergence.

One JSON file; a line per measurement on stdout as it goes.  Measurement only: nothing here is checked
(tests/test_gpu_device_loop.py is the check).
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

SPECS = ("laplace5:3162,3162", "laplace5:1000,1000", "laplace5:316,316")
STRIDES = (4, 8, 16, 32)
THRESHOLD = 1e-300


def timed_solve(ctx, A, vecs, n, its, stride, dinv=None):
    """stride 0: the host loop; dinv: the preconditioned loops -> (ms, iterations run)"""
    ctx.upload(vecs[1], np.zeros(n))
    ctx.synchronize()
    t0 = time.perf_counter()
    if stride:
        itr, _ = amd.cg_solve_device(ctx, A, *vecs, max_itrs=its, conv_threshold=THRESHOLD, stride=stride,
                                     precond=dinv)
    else:
        itr, _ = amd.cg_solve(ctx, A, *vecs, max_itrs=its, conv_threshold=THRESHOLD, precond=dinv)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, itr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="device_loop_bench.json")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--specs", default=";".join(SPECS), help="matrices, separated by ';'")
    ap.add_argument("--strides", default=",".join(str(s) for s in STRIDES))
    ap.add_argument("--precond", choices=("none", "jacobi"), default="none")
    a = ap.parse_args()
    strides = [int(s) for s in a.strides.split(",")]
    argv = [v for i, v in enumerate(sys.argv) if v != "--out" and (i == 0 or sys.argv[i - 1] != "--out")]
    res = {"cmd": " ".join(argv), "iters": a.iters, "blocks": a.blocks, "threshold": THRESHOLD,
           "precond": a.precond, "rows": []}
    for spec in a.specs.split(";"):
        cols, rows, vals, n = generators.generate(spec)
        ctx = amd.HIPContext("none", "csr", on_event=lambda ev, fatal: None)
        A = ctx.create_matrix(cols, rows, vals, n, len(vals))
        nnz = len(vals)
        del cols, rows, vals
        vecs = [ctx.create_vector(n) for _ in range(5)]
        ctx.upload(vecs[0], generators.reference_rhs(n))
        dinv = ctx.jacobi(A) if a.precond == "jacobi" else None
        kinds = [0] + strides
        for k in kinds:  # warm-up: first launches, the graph's instantiation path
            timed_solve(ctx, A, vecs, n, max(k, 5), k, dinv)
        per = {k: [] for k in kinds}
        for _ in range(a.blocks):
            for k in kinds:
                ms, itr = timed_solve(ctx, A, vecs, n, a.iters, k, dinv)
                assert itr == a.iters, (spec, k, itr)  # every iteration live in both loops
                per[k].append(ms / a.iters)
        host = statistics.median(per[0])
        dev = {k: statistics.median(per[k]) for k in strides}
        best = min(dev.values())
        row = dict(spec=spec, fmt="csr", mode="none", layout=ctx.matrix_info(A)[0], precond=a.precond, n=n, nnz=nnz,
                   ms_per_iter_host=host,
                   ms_per_iter_device={str(k): v for k, v in dev.items()},
                   ratio_device_over_host={str(k): v / host for k, v in dev.items()},
                   best_stride=min(k for k in strides if dev[k] <= 1.02 * best),
                   frozen_spmv_worst={str(k): k - 1 for k in strides},
                   blocks={str(k): v for k, v in per.items()})
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
