"""The protected row structure: what the two codes cost per SpMV.

`spmv` on a matrix created with structure_ecc=True against the same matrix with layout="stream" alone -- and, for the
first matrix, against the default layout too, because giving up compact and packed blocks is part of the price --,
alternating in one process, `--reps` calls per block behind one synchronisation; the median over the blocks of the
time per call, and the ratios.  tools/vector_ecc_bench.py's method.  Matrices:

  laplace5:3162,3162   (config 2) every block is uniform: no row word is read, only the descriptor check is paid
  random:4194304,24,1  (config 4) forced to the streaming layout: every row's word is read

each in modes none and secded.

    python tools/structure_ecc_bench.py --out profiles/structure_ecc_bench.json [--reps 50] [--blocks 5]

One JSON file; a line per measurement on stdout as it goes.  Measurement only: nothing here is checked
(tests/test_gpu_structure_ecc.py is the check).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import abft_sparse_cg_amd as amd  # noqa: E402
from abft_sparse_cg_amd import generators  # noqa: E402

MATRICES = (("config2", "laplace5:3162,3162", True), ("config4", "random:4194304,24,1", False))  # (.., with the default layout)
MODES = ("none", "secded")


def timed(ctx, A, x, y, reps):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.spmv(A, x, y)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="structure_ecc_bench.json")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--matrices", default="config2,config4")
    a = ap.parse_args()
    argv = [v for i, v in enumerate(sys.argv) if v != "--out" and (i == 0 or sys.argv[i - 1] != "--out")]
    res = {"cmd": " ".join(argv), "reps": a.reps, "blocks": a.blocks, "unit": "us per spmv", "rows": []}
    for name, spec, with_default in MATRICES:
        if name not in a.matrices.split(","):
            continue
        cols, rows, vals, n = generators.generate(spec)
        for mode in MODES:
            ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: None)
            x, y = ctx.create_vector(n), ctx.create_vector(n)
            ctx.upload(x, generators.reference_rhs(n))
            kinds = {"stream": dict(layout="stream"), "protected": dict(layout="stream", structure_ecc=True)}
            if with_default:
                kinds["default"] = {}
            mats = {k: ctx.create_matrix(cols, rows, vals, n, len(vals), **kw) for k, kw in kinds.items()}
            for A in mats.values():
                timed(ctx, A, x, y, 5)
            per = {k: [] for k in mats}
            for _ in range(a.blocks):
                for k, A in mats.items():
                    per[k].append(timed(ctx, A, x, y, a.reps))
            med = {k: statistics.median(v) for k, v in per.items()}
            row = dict(config=name, spec=spec, fmt="csr", mode=mode, n=n, nnz=len(vals),
                       layout_default=ctx.matrix_info(mats["default"])[0] if with_default else None,
                       us_stream=med["stream"], us_protected=med["protected"], us_default=med.get("default"),
                       ratio_protected_to_stream=med["protected"] / med["stream"],
                       ratio_protected_to_default=med["protected"] / med["default"] if with_default else None,
                       blocks={k: v for k, v in per.items()})
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            stray = ctx.drain_events()
            if stray[0]:
                print("events queued during the measurement: %r" % (stray,), flush=True)
            ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
