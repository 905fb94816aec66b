"""Matrix digests: what a verification costs, and what it adds to a solve.

1. The digest itself.  For config 2's matrix in modes none and secded and config 4's matrix (secded) in its default
   layout: the matrix is armed, then `--reps` verify_matrix_dev calls behind one synchronisation per block, the median
   over `--blocks` blocks of the time per verification, and GB/s over the bytes matrix_segments reports.  Beside them
   ctx.stream_probe()'s read figure from the same process on the same box: the kernel is a plain read stream with a
   few integer operations per word, so that probe is its yardstick, per segment size.
2. The solvers.  cg_solve and cg_solve_device (stride 16) on config 2's matrix in mode none, `--iterations` iterations
   with the threshold out of reach, matrix_check_every 0, 16 and 50 alternating in one process: the median over the
   blocks of the time per solve.

    python tools/matrix_digest_bench.py --out profiles/matrix_digest_bench.json [--reps 20] [--blocks 5]

One JSON file; a line per measurement on stdout as it goes.  One run on one box: measurement only, nothing here is
checked and no ratio is a claim (tests/test_gpu_matrix_digest.py is the check).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import abft_sparse_cg_amd as amd  # noqa: E402
from abft_sparse_cg_amd import generators  # noqa: E402

MATRICES = (("config2", "laplace5:3162,3162", ("none", "secded")), ("config4", "random:4194304,24,1", ("secded",)))
EVERY = (0, 16, 50)


def timed_verify(ctx, A, reps):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.verify_matrix_dev(A)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def digest_rows(a, res):
    for name, spec, modes in MATRICES:
        if name not in a.matrices.split(","):
            continue
        cols, rows, vals, n = generators.generate(spec)
        for mode in modes:
            ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: None)
            A = ctx.create_matrix(cols, rows, vals, n, len(vals))
            ctx.arm_matrix(A)
            segs = ctx.matrix_segments(A)
            nbytes = sum(size for _, size in segs)
            timed_verify(ctx, A, 3)
            per = [timed_verify(ctx, A, a.reps) for _ in range(a.blocks)]
            us = statistics.median(per)
            _, probe_read = ctx.stream_probe(max(1 << 20, min(nbytes, 1 << 30)), 10)
            row = dict(kind="digest", config=name, spec=spec, mode=mode, layout=ctx.matrix_info(A)[0], n=n, nnz=len(vals),
                       segments={s: size for s, size in segs}, bytes=nbytes, us_per_verification=us,
                       gbps=nbytes / us / 1e3, probe_read_gbps=probe_read, probe_bytes=max(1 << 20, min(nbytes, 1 << 30)),
                       blocks=per, clean=ctx.verify_matrix(A) == [])
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            stray = ctx.drain_events()
            if stray[0]:
                print("events queued during the measurement: %r" % (stray,), flush=True)
            ctx.close()


def solver_rows(a, res):
    name, spec, _ = MATRICES[0]
    if name not in a.matrices.split(","):
        return
    cols, rows, vals, n = generators.generate(spec)
    ctx = amd.HIPContext("none", "csr", on_event=lambda ev, fatal: None)
    A = ctx.create_matrix(cols, rows, vals, n, len(vals))
    b, x, r, p, w = (ctx.create_vector(n) for _ in range(5))
    ctx.upload(b, generators.reference_rhs(n))
    zero = np.zeros(n)

    def solve(f, every, **kw):
        ctx.upload(x, zero)
        ctx.synchronize()
        t0 = time.perf_counter()
        itr, _ = f(ctx, A, b, x, r, p, w, a.iterations, 0.0, **kw, **({"matrix_check_every": every} if every else {}))
        ctx.synchronize()
        assert itr == a.iterations, itr
        return (time.perf_counter() - t0) * 1e3

    for label, f, kw in (("cg_solve", amd.cg_solve, {}), ("cg_solve_device", amd.cg_solve_device, dict(stride=16))):
        for every in EVERY:
            solve(f, every, **kw)  # warm: the graphs' first capture, the arming
        per = {every: [] for every in EVERY}
        for _ in range(a.blocks):
            for every in EVERY:
                per[every].append(solve(f, every, **kw))
        row = dict(kind="solve", solver=label, config=name, spec=spec, mode="none", iterations=a.iterations, **kw,
                   ms_per_solve={str(every): statistics.median(v) for every, v in per.items()},
                   blocks={str(every): v for every, v in per.items()})
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="matrix_digest_bench.json")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--matrices", default="config2,config4")
    a = ap.parse_args()
    argv = [v for i, v in enumerate(sys.argv) if v != "--out" and (i == 0 or sys.argv[i - 1] != "--out")]
    res = {"cmd": " ".join(argv), "reps": a.reps, "blocks": a.blocks, "rows": []}
    digest_rows(a, res)
    solver_rows(a, res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
