"""The fused block iteration against the unfused one.

For config 2's matrix (laplace5:3162,3162; modes none and secded) and config 4's matrix in the
streaming layout (random:4194304,24,1), for K in {2, 4, 8}: cg_solve_block(fused=True) and
cg_solve_block(fused=False) alternate in ONE process at -c 0, a fixed number of iterations after a
warm-up, five blocks each; per loop the median ms per iteration and the spread (max - min) of the
five blocks, their ratio, and the time per right-hand side against the single loop (cg_solve on one
column, the same way).  A second pass brackets the kernels with the library's HIP events
(abft_hip_profile_*) and gives the device time per call of each of the four kernel classes in both
loops: the SpMM with and without the fused product, the fold / the dot pass, calc_xr / calc_r,
calc_p / calc_px.

    python tools/block_fused_bench.py --out profiles/r10/block_fused_bench.json
    rocprofv3 --kernel-trace --stats -- python tools/block_fused_bench.py --kernels 20 --matrices config2 \
        --modes none --ks 4        # both loops, nothing timed or written: for a trace of its own

One JSON file; a line per measurement on stdout as it goes.  Measurement only: nothing here is
checked (tests/test_gpu_block_fused.py is the check).
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
KERNELS = (("spmm", capi.K_SPMV), ("dot_or_fold", capi.K_DOT), ("calc_xr_or_r", capi.K_CALC_XR),
           ("calc_p_or_px", capi.K_CALC_P))


class Loops:
    """the vectors of one (matrix, K) and the three loops on them"""

    def __init__(self, ctx, A, n, k):
        self.ctx, self.A, self.n, self.k = ctx, A, n, k
        B = np.stack([generators.reference_rhs(n, seed=1 + j) for j in range(k)], axis=1)
        self.V = [ctx.create_block(n, k) for _ in range(5)]
        self.v = [ctx.create_vector(n) for _ in range(5)]
        ctx.upload(self.V[0], B)
        ctx.upload(self.v[0], B[:, 0])
        self.zero, self.zero1 = np.zeros((n, k)), np.zeros(n)

    def block(self, iters, fused):
        self.ctx.upload(self.V[1], self.zero)
        self.ctx.synchronize()
        t0 = time.perf_counter()
        amd.cg_solve_block(self.ctx, self.A, *self.V, max_itrs=iters, conv_threshold=0.0, fused=fused)
        self.ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    def single(self, iters):
        self.ctx.upload(self.v[1], self.zero1)
        self.ctx.synchronize()
        t0 = time.perf_counter()
        amd.cg_solve(self.ctx, self.A, *self.v, max_itrs=iters, conv_threshold=0.0)
        self.ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    def kernel_us(self, iters, fused):
        """device time per launch of each kernel class over `iters` iterations of one loop"""
        mask = sum(1 << kid for _, kid in KERNELS)
        self.ctx.upload(self.V[1], self.zero)
        self.ctx.profile(mask)
        amd.cg_solve_block(self.ctx, self.A, *self.V, max_itrs=iters, conv_threshold=0.0, fused=fused)
        out = {}
        for name, kid in KERNELS:
            ms, launches = self.ctx.profile_read(kid)
            out[name] = dict(us=ms * 1e3 / max(launches, 1), launches=launches)
        self.ctx.profile(0)
        return out

    def close(self):
        for w in self.V + self.v:
            self.ctx.destroy_vector(w)


def med_spread(v):
    return statistics.median(v), max(v) - min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="block_fused_bench.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--modes", default="none,secded")
    ap.add_argument("--matrices", default="config2,config4")
    ap.add_argument("--kernels", type=int, default=0, metavar="M",
                    help="run M iterations of each loop and nothing else (for a kernel trace)")
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    argv = [v for i, v in enumerate(sys.argv) if v != "--out" and (i == 0 or sys.argv[i - 1] != "--out")]
    res = {"cmd": " ".join(argv), "ks": ks, "iters": a.iters, "warmup": a.warmup, "blocks": a.blocks, "rows": []}
    for name in a.matrices.split(","):
        spec = MATRICES[name]
        cols, rows, vals, n = generators.generate(spec)
        nnz = len(vals)
        for mode in a.modes.split(","):
            ctx = amd.HIPContext(mode, "csr")
            A = ctx.create_matrix(cols, rows, vals, n, nnz, layout="stream")
            for k in ks:
                L = Loops(ctx, A, n, k)
                if a.kernels:
                    for fused in (False, True):
                        L.block(a.warmup, fused)
                        L.block(a.kernels, fused)
                    L.close()
                    continue
                for fused in (False, True):
                    L.block(a.warmup, fused)
                L.single(a.warmup)
                un, fu, one = [], [], []
                for _ in range(a.blocks):  # the loops alternate: drift hits all three alike
                    un.append(L.block(a.iters, False))
                    fu.append(L.block(a.iters, True))
                    one.append(L.single(a.iters))
                (un_ms, un_sp), (fu_ms, fu_sp), (one_ms, one_sp) = med_spread(un), med_spread(fu), med_spread(one)
                row = dict(matrix=name, spec=spec, mode=mode, k=k, n=n, nnz=nnz,
                           unfused_ms_per_iter=un_ms, unfused_spread_ms=un_sp, unfused_blocks_ms=un,
                           fused_ms_per_iter=fu_ms, fused_spread_ms=fu_sp, fused_blocks_ms=fu,
                           fused_over_unfused=fu_ms / un_ms,
                           single_ms_per_iter=one_ms, single_spread_ms=one_sp,
                           unfused_per_rhs_over_single=un_ms / k / one_ms,
                           fused_per_rhs_over_single=fu_ms / k / one_ms,
                           kernels_unfused=L.kernel_us(a.iters, False), kernels_fused=L.kernel_us(a.iters, True))
                L.close()
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
            ctx.destroy_matrix(A)
            ctx.close()
        del cols, rows, vals
    if a.kernels:
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
