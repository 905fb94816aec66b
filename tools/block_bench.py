"""Block right-hand sides against K single solves ("Block right-hand sides").

For config 2's matrix (laplace5:3162,3162) and config 4's matrix in the streaming layout
(random:4194304,24,1), for K in {1, 2, 4, 8} and the modes none, sed, secded:

  * spmm of K columns against K single spmv: device time per call from the library's HIP-event
    brackets (abft_hip_profile_*, kernel ABFT_K_SPMV), the median over 5 blocks of launches, and the
    algorithmic bytes 12 nnz + 4 (N + 1) + 16 N K (one pass over the ECC-protected matrix, K columns
    of x read and of y written);
  * the CG iteration time per right-hand side: cg_solve_block on K columns against cg_solve on one,
    both from Python, -c 0, a fixed number of iterations after a warm-up.

    python tools/block_bench.py --out profiles/r05/block_bench.json [--iters 20] [--calls 20]

One JSON file; a line per measurement on stdout as it goes.  Measurement only: nothing here is
checked (tests/test_gpu_block.py is the check).
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

MATRICES = {"config2": "laplace5:3162,3162", "config4": "random:4194304,24,1"}


def spmv_times(ctx, A, n, k, calls, blocks=5):
    """-> (ms per spmm of k columns, ms per single spmv), medians over `blocks` blocks of `calls`"""
    X, Y = ctx.create_block(n, k), ctx.create_block(n, k)
    x, y = ctx.create_vector(n), ctx.create_vector(n)
    ctx.upload(X, np.stack([generators.reference_rhs(n, seed=1 + j) for j in range(k)], axis=1))
    ctx.upload(x, generators.reference_rhs(n))
    out = []
    for run in (lambda: ctx.spmm(A, X, Y, k, drain=False), lambda: ctx.spmv(A, x, y)):
        for _ in range(3):
            run()
        per = []
        for _ in range(blocks):
            ctx.profile(1 << capi.K_SPMV)
            for _ in range(calls):
                run()
            ms, launches = ctx.profile_read(capi.K_SPMV)
            per.append(ms / max(launches, 1))
        ctx.profile(0)
        out.append(statistics.median(per))
    for v in (X, Y, x, y):
        ctx.destroy_vector(v)
    return out


def cg_times(ctx, A, n, k, iters, warmup):
    """-> (ms per block iteration, ms per single iteration), -c 0"""
    B = np.stack([generators.reference_rhs(n, seed=1 + j) for j in range(k)], axis=1)
    V = [ctx.create_block(n, k) for _ in range(5)]
    v = [ctx.create_vector(n) for _ in range(5)]
    ctx.upload(V[0], B)
    ctx.upload(v[0], B[:, 0])
    out = []
    for solve, vecs, zero in ((amd.cg_solve_block, V, np.zeros((n, k))), (amd.cg_solve, v, np.zeros(n))):
        ctx.upload(vecs[1], zero)
        solve(ctx, A, *vecs, max_itrs=warmup, conv_threshold=0.0)
        ctx.upload(vecs[1], zero)
        ctx.synchronize()
        t0 = time.perf_counter()
        solve(ctx, A, *vecs, max_itrs=iters, conv_threshold=0.0)
        ctx.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    for w in V + v:
        ctx.destroy_vector(w)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="block_bench.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--modes", default="none,sed,secded")
    ap.add_argument("--matrices", default="config2,config4")
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    # the command as run, without where its output went
    argv = [v for i, v in enumerate(sys.argv) if v != "--out" and (i == 0 or sys.argv[i - 1] != "--out")]
    res = {"cmd": " ".join(argv), "ks": ks, "iters": a.iters, "warmup": a.warmup, "calls": a.calls, "rows": []}
    for name in a.matrices.split(","):
        spec = MATRICES[name]
        cols, rows, vals, n = generators.generate(spec)
        nnz = len(vals)
        for mode in a.modes.split(","):
            ctx = amd.HIPContext(mode, "csr")
            A = ctx.create_matrix(cols, rows, vals, n, nnz, layout="stream")
            for k in ks:
                spmm_ms, spmv_ms = spmv_times(ctx, A, n, k, a.calls)
                blk_ms, one_ms = cg_times(ctx, A, n, k, a.iters, a.warmup)
                nbytes = 12 * nnz + 4 * (n + 1) + 16 * n * k
                row = dict(matrix=name, spec=spec, mode=mode, k=k, n=n, nnz=nnz,
                           spmm_us=spmm_ms * 1e3, spmv_us=spmv_ms * 1e3, spmm_over_spmv=spmm_ms / spmv_ms,
                           spmm_over_k_spmv=spmm_ms / (k * spmv_ms), spmm_bytes=nbytes,
                           spmm_gbps=nbytes / (spmm_ms * 1e-3) / 1e9,
                           cg_block_ms_per_iter=blk_ms, cg_single_ms_per_iter=one_ms,
                           cg_per_rhs_over_single=blk_ms / k / one_ms)
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
            ctx.destroy_matrix(A)
            ctx.close()
        del cols, rows, vals
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
