"""Protected vectors: what the (64, 57) code costs per iteration.

The Python cg_solve loop, -c 0, a fixed number of iterations, plain and with vector_ecc=True,
alternating in one process, one solve each per block; the median over the blocks of the time per
iteration, and their ratio.  Cases: config 2's matrix (laplace5:3162,3162, CSR, streaming layout) in
modes none, secded and sed.  The plain loop is the yardstick: it defers the x update (64 N bytes of
vector traffic per iteration), the protected loop does not (72 N).
The protected solve's time includes what cg_solve does around its loop -- two encodes, a copy, three scrubs
with their host synchronisations and one layout query -- which the plain solve does not have: over 200
iterations that raises the ratio by about half a percent.

    python tools/vector_ecc_bench.py --out profiles/r09/vector_ecc_bench.json [--iters 200] [--blocks 5]

`--kernels M`: instead, M iterations of each loop on config 2 `none` (for a `rocprofv3 --kernel-trace
--stats` run of its own: the four protected kernels beside their plain counterparts on one box).

`--rhs K[,K...]`: instead, the protected BLOCK loop, cg_solve_block(vector_ecc=True), against
the plain fused block loop of the same build, cg_solve_block(fused=True) -- the yardstick: both move 64 N K bytes of
vectors behind the SpMM --, alternating in one process, the median of --blocks; on config 2's and config 4's matrices
in modes none and secded.  The protected solve's window also holds its two encodes, two copies and three scrubs.

    python tools/vector_ecc_bench.py --rhs 2,4,8 --out profiles/vector_ecc_block_bench.json [--iters 20]

One JSON file; a line per measurement on stdout as it goes.  Measurement only: nothing here is
checked (tests/test_gpu_vector_ecc.py is the check).
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
MODES = ("none", "secded", "sed")


def timed_solve(ctx, A, vecs, b, n, its, ecc):
    ctx.upload(vecs[0], b)  # (the protected solve encodes b in place)
    ctx.upload(vecs[1], np.zeros(n))
    ctx.synchronize()
    t0 = time.perf_counter()
    amd.cg_solve(ctx, A, *vecs, max_itrs=its, conv_threshold=0.0, vector_ecc=ecc)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


BLOCK_MATRICES = {"config2": SPEC, "config4": "random:4194304,24,1"}
BLOCK_MODES = ("none", "secded")


def timed_block_solve(ctx, A, V, B, zero, its, ecc):
    ctx.upload(V[0], B)  # (the protected solve encodes B in place)
    ctx.upload(V[1], zero)
    ctx.synchronize()
    t0 = time.perf_counter()
    amd.cg_solve_block(ctx, A, *V, max_itrs=its, conv_threshold=0.0, **({"vector_ecc": True} if ecc else {"fused": True}))
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def block_rows(a, res):
    ks = [int(k) for k in a.rhs.split(",")]
    for name in a.matrices.split(","):
        spec = BLOCK_MATRICES[name]
        cols, rows, vals, n = generators.generate(spec)
        for mode in BLOCK_MODES:
            ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: None)
            A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
            for k in ks:
                B = np.stack([generators.reference_rhs(n, seed=1 + j) for j in range(k)], axis=1)
                zero = np.zeros((n, k))
                V = [ctx.create_block(n, k) for _ in range(5)]
                for ecc in (False, True):
                    timed_block_solve(ctx, A, V, B, zero, 3, ecc)
                per = {False: [], True: []}
                for _ in range(a.blocks):
                    for ecc in (False, True):
                        per[ecc].append(timed_block_solve(ctx, A, V, B, zero, a.iters, ecc) / a.iters)
                plain, prot = statistics.median(per[False]), statistics.median(per[True])
                row = dict(config=name, spec=spec, fmt="csr", mode=mode, k=k, n=n, nnz=len(vals),
                           ms_per_iter_plain_fused=plain, ms_per_iter_protected=prot, ratio=prot / plain,
                           blocks_plain_fused=per[False], blocks_protected=per[True])
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                for v in V:
                    ctx.destroy_vector(v)
            ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rhs", default="", metavar="K[,K...]", help="the protected block loop against the plain fused one")
    ap.add_argument("--matrices", default="config2,config4", help="with --rhs: which of config2, config4")
    ap.add_argument("--out", default="vector_ecc_bench.json")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--kernels", type=int, default=0, help="M iterations of each loop on config 2 `none`, nothing timed")
    a = ap.parse_args()
    argv = [v for i, v in enumerate(sys.argv) if v != "--out" and (i == 0 or sys.argv[i - 1] != "--out")]
    res = {"cmd": " ".join(argv), "iters": a.iters, "blocks": a.blocks, "rows": []}
    if a.rhs:
        block_rows(a, res)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        return 0
    cols, rows, vals, n = generators.generate(SPEC)
    b = generators.reference_rhs(n)
    for mode in MODES[:1] if a.kernels else MODES:
        ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: None)
        A = ctx.create_matrix(cols, rows, vals, n, len(vals), layout="stream")
        vecs = [ctx.create_vector(n) for _ in range(5)]
        for ecc in (False, True):
            timed_solve(ctx, A, vecs, b, n, a.kernels or 5, ecc)
        if not a.kernels:
            per = {False: [], True: []}
            for _ in range(a.blocks):
                for ecc in (False, True):
                    per[ecc].append(timed_solve(ctx, A, vecs, b, n, a.iters, ecc) / a.iters)
            plain, prot = statistics.median(per[False]), statistics.median(per[True])
            row = dict(config="config2", spec=SPEC, fmt="csr", mode=mode, n=n, nnz=len(vals),
                       ms_per_iter_plain=plain, ms_per_iter_protected=prot, ratio=prot / plain,
                       blocks_plain=per[False], blocks_protected=per[True])
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
