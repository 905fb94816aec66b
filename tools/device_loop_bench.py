"""The device-scalar loop with a stop test against the host-scalar loop.

cg_solve and cg_solve_device alternating in one process: max_itrs = 200 and a threshold of 1e-300, so that every
iteration is live and both loops run the same 200 iterations; one solve each per block (the device loop once per
stride), the median over the blocks of the time per iteration, and the ratio device / host.  Matrices:
laplace5:3162,3162 (config 2, 10 M rows), laplace5:1000,1000 and laplace5:316,316, all CSR `none`.  Strides 4, 8,
16 and 32.  The host loop is the yardstick: this feature does not touch it.

    python tools/device_loop_bench.py --out profiles/device_loop_bench.json [--iters 200] [--blocks 5]
                                      [--specs laplace5:1000,1000,...] [--strides 4,8,16,32]
                                      [--precond jacobi] [--rhs 4,8 [--modes none,secded]]
                                      [--vector-ecc [--precond jacobi] [--modes none,secded]]
                                      [--vector-ecc --rhs 4,8 [--modes none,secded]]
                                      [--check-every 50 [--precond jacobi] [--modes none,secded]]

--precond jacobi alternates cg_solve(precond=dinv) and cg_solve_device(precond=dinv) instead,
dinv = ctx.jacobi(A); the JSON says so under `precond`, in the file and in every row.  The yardstick is then
cg_solve(precond=) of the same build.

--rhs K[,K...] measures the block loops instead: cg_solve_block(fused=True) and
cg_solve_block_device alternating on the same matrix (streaming layout) and the same K seeded right-hand sides, in
every mode of --modes (default none,secded), over the strides 4, 16 and 64 unless --strides says otherwise; the
per-column counts of the two loops are asserted equal.  Matrices by default laplace5:3162,3162 and
laplace5:1000,1000; times are per iteration of all K columns.  --out defaults to
profiles/device_loop_bench_block.json there.  Without --rhs nothing changes.

--vector-ecc measures the loops on protected vectors instead: cg_solve(vector_ecc=True) and
cg_solve_device(vector_ecc=True) alternating on the same matrix (streaming layout), in every mode of --modes (default
none,secded).  Matrices by default laplace5:3162,3162 and laplace5:1000,1000.  The yardstick is
cg_solve(vector_ecc=True) of the same build; both loops pay the same start (two encodes, a scrub) and end (two
scrubs) inside the timed window.  --out defaults to profiles/device_loop_bench_vecc.json there.  Without the flag
nothing changes.

--vector-ecc --precond jacobi measures Jacobi-preconditioned CG on protected vectors:
cg_solve(vector_ecc=True, precond=dinv) and cg_solve_device(vector_ecc=True, precond=dinv) alternating, dinv =
ctx.jacobi(A, protected=True) made once per context.  The yardstick is the protected host PCG loop of the same build;
both loops pay the same start and the same end (three scrubs now) inside the timed window.  --out defaults to
profiles/device_loop_bench_vecc_precond.json there; the rows say precond: jacobi.

--vector-ecc --rhs K[,K...] measures the block loops on protected vectors: three loops over the
same iterations -- cg_solve_block(vector_ecc=True), cg_solve_block_device(vector_ecc=True) and, for context, the plain
cg_solve_block_device -- alternating on the same matrix (streaming layout) and the same K seeded right-hand sides, with
the specs, strides and modes of --rhs; the per-column counts are asserted equal.  The yardstick is the protected host
block loop of the same build; both protected loops pay the same start and end inside the timed window.  --out defaults
to profiles/device_loop_bench_block_vecc.json there.  --precond jacobi is refused: the protected block loops have no
Jacobi form.

--check-every N measures the cost of residual checks in the device-resident loop:
cg_solve_device without checks and cg_solve_device(check_every=N) alternating in one process on the same matrix, in
every mode of --modes, at the strides of --strides (default 16); the checkpoint vector is made once and passed in.  The
yardstick is the same loop without checks of the same build; `ratio_check_over_plain` is the figure.  Every check
must pass (asserted).  Matrices by default laplace5:3162,3162 and laplace5:1000,1000.  --out defaults to
profiles/device_loop_bench_check.json there.  Without the flag nothing changes.

Also reported per matrix: `best_stride`, the smallest stride within 2 % of the best device-loop time (what
DEFAULT_STRIDE is to be on the 1 M-row matrix), and `frozen_spmv_worst`, stride - 1: the SpMVs a solve can waste
behind convergence.

--trail-ecc measures what the protected scalar trail costs: cg_solve_device without and with
trail_ecc=True alternating in one process on the same matrix, in every mode of --modes, at every stride of --strides
(default 4,16), on the 1 M-row and 10 M-row Laplacians unless --specs says otherwise; ratio_trail_over_plain is against
the same loop without the keyword.  Goes with --precond jacobi and with --vector-ecc; --out defaults to
profiles/device_loop_bench_trail.json there.  Without the flag nothing changes.

--trail-ecc --rhs K[,K...] [--vector-ecc] measures the same for the block loop:
cg_solve_block_device without and with trail_ecc=True alternating in one process, on the K seeded right-hand sides of
--rhs and the streaming layout, with the kinds, strides, specs and modes of --trail-ecc; the per-column counts are
asserted equal.  --out defaults to profiles/device_loop_bench_block_trail.json there.  --check-every stays refused.

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


def timed_solve(ctx, A, vecs, n, its, stride, dinv=None, vecc=False):
    """stride 0: the host loop; dinv: the preconditioned loops; vecc: the loops on protected vectors
    -> (ms, iterations run)"""
    kw = {"vector_ecc": True} if vecc else {}
    ctx.upload(vecs[1], np.zeros(n))
    ctx.synchronize()
    t0 = time.perf_counter()
    if stride:
        itr, _ = amd.cg_solve_device(ctx, A, *vecs, max_itrs=its, conv_threshold=THRESHOLD, stride=stride,
                                     precond=dinv, **kw)
    else:
        itr, _ = amd.cg_solve(ctx, A, *vecs, max_itrs=its, conv_threshold=THRESHOLD, precond=dinv, **kw)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, itr


BLOCK_SPECS = ("laplace5:3162,3162", "laplace5:1000,1000")
BLOCK_STRIDES = (4, 16, 64)


def timed_block_solve(ctx, A, vecs, n, k, its, stride, dinv=None, vecc=False, b=None):
    """stride 0: cg_solve_block(fused=True); else cg_solve_block_device; vecc: the loops on protected block vectors (b:
    the right-hand sides, uploaded again outside the timed window -- a protected solve leaves codewords in them)
    -> (ms, per-column counts)"""
    kw = {"vector_ecc": True} if vecc else {}
    if b is not None:
        ctx.upload(vecs[0], b)
    ctx.upload(vecs[1], np.zeros((n, k)))
    ctx.synchronize()
    t0 = time.perf_counter()
    if stride:
        itrs, _ = amd.cg_solve_block_device(ctx, A, *vecs, max_itrs=its, conv_threshold=THRESHOLD, stride=stride,
                                            precond=dinv, **kw)
    elif vecc:
        itrs, _ = amd.cg_solve_block(ctx, A, *vecs, max_itrs=its, conv_threshold=THRESHOLD, vector_ecc=True)
    else:
        itrs, _ = amd.cg_solve_block(ctx, A, *vecs, max_itrs=its, conv_threshold=THRESHOLD, precond=dinv, fused=True)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, list(itrs)


def block_main(a, res):
    """--rhs: the block loops, one row per (matrix, mode, K)"""
    strides = [int(s) for s in (a.strides or ",".join(str(s) for s in BLOCK_STRIDES)).split(",")]
    res["rhs"] = [int(k) for k in a.rhs.split(",")]
    res["modes"] = a.modes.split(",")
    for spec in (a.specs or ";".join(BLOCK_SPECS)).split(";"):
        cols, rows, vals, n = generators.generate(spec)
        nnz = len(vals)
        for mode in res["modes"]:
            ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: None)
            A = ctx.create_matrix(cols, rows, vals, n, nnz, layout="stream")
            dinv = ctx.jacobi(A) if a.precond == "jacobi" else None
            for k in res["rhs"]:
                vecs = [ctx.create_block(n, k) for _ in range(5)]
                ctx.upload(vecs[0], np.random.default_rng(7).random((n, k)) + 0.5)
                kinds = [0] + strides
                for st in kinds:  # warm-up: first launches, the graph's instantiation path
                    timed_block_solve(ctx, A, vecs, n, k, max(st, 5), st, dinv)
                per = {st: [] for st in kinds}
                for _ in range(a.blocks):
                    counts = None
                    for st in kinds:
                        ms, itrs = timed_block_solve(ctx, A, vecs, n, k, a.iters, st, dinv)
                        counts = counts or itrs
                        assert itrs == counts == [a.iters] * k, (spec, mode, k, st, itrs, counts)  # equal counts, all live
                        per[st].append(ms / a.iters)
                host = statistics.median(per[0])
                dev = {st: statistics.median(per[st]) for st in strides}
                best = min(dev.values())
                row = dict(spec=spec, fmt="csr", mode=mode, layout=ctx.matrix_info(A)[0], precond=a.precond, rhs=k, n=n,
                           nnz=nnz, ms_per_iter_host_fused=host,
                           ms_per_iter_device={str(st): v for st, v in dev.items()},
                           ratio_device_over_host={str(st): v / host for st, v in dev.items()},
                           best_stride=min(st for st in strides if dev[st] <= 1.02 * best),
                           frozen_spmm_worst={str(st): st - 1 for st in strides},
                           blocks={str(st): v for st, v in per.items()})
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                for v in vecs:
                    ctx.destroy_vector(v)
            ctx.close()
        del cols, rows, vals


def block_vecc_main(a, res):
    """--vector-ecc --rhs: the block loops on protected vectors, one row per (matrix, mode, K).  Kinds: ("host", 0) the
    protected host loop, ("vecc", stride) the protected device loop, ("plain", stride) the plain device loop"""
    strides = [int(s) for s in (a.strides or ",".join(str(s) for s in BLOCK_STRIDES)).split(",")]
    res["rhs"] = [int(k) for k in a.rhs.split(",")]
    res["vector_ecc"] = True
    res["modes"] = a.modes.split(",")
    for spec in (a.specs or ";".join(BLOCK_SPECS)).split(";"):
        cols, rows, vals, n = generators.generate(spec)
        nnz = len(vals)
        for mode in res["modes"]:
            ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: None)
            A = ctx.create_matrix(cols, rows, vals, n, nnz, layout="stream")
            for k in res["rhs"]:
                vecs = [ctx.create_block(n, k) for _ in range(5)]
                b = np.random.default_rng(7).random((n, k)) + 0.5
                kinds = [("host", 0)] + [("vecc", st) for st in strides] + [("plain", st) for st in strides]

                def run(kind, its):
                    return timed_block_solve(ctx, A, vecs, n, k, its, kind[1], vecc=kind[0] != "plain", b=b)
                for kind in kinds:  # warm-up: first launches, the graph's instantiation path
                    run(kind, max(kind[1], 5))
                per = {kind: [] for kind in kinds}
                for _ in range(a.blocks):
                    for kind in kinds:
                        ms, itrs = run(kind, a.iters)
                        assert itrs == [a.iters] * k, (spec, mode, k, kind, itrs)  # equal counts, all live
                        per[kind].append(ms / a.iters)
                host = statistics.median(per[("host", 0)])
                dev = {st: statistics.median(per[("vecc", st)]) for st in strides}
                plain = {st: statistics.median(per[("plain", st)]) for st in strides}
                best = min(dev.values())
                row = dict(spec=spec, fmt="csr", mode=mode, layout=ctx.matrix_info(A)[0], vector_ecc=True, precond="none",
                           rhs=k, n=n, nnz=nnz, ms_per_iter_host_vecc=host,
                           ms_per_iter_device_vecc={str(st): v for st, v in dev.items()},
                           ms_per_iter_device_plain={str(st): v for st, v in plain.items()},
                           ratio_device_over_host={str(st): v / host for st, v in dev.items()},
                           best_stride=min(st for st in strides if dev[st] <= 1.02 * best),
                           frozen_spmm_worst={str(st): st - 1 for st in strides},
                           blocks={"%s:%d" % kind: v for kind, v in per.items()})
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                for v in vecs:
                    ctx.destroy_vector(v)
            ctx.close()
        del cols, rows, vals


VECC_SPECS = ("laplace5:3162,3162", "laplace5:1000,1000")


def vecc_main(a, res):
    """--vector-ecc: the loops on protected vectors (with --precond jacobi: the protected PCG loops), one row per
    (matrix, mode)"""
    strides = [int(s) for s in (a.strides or ",".join(str(s) for s in STRIDES)).split(",")]
    res["vector_ecc"] = True
    res["modes"] = a.modes.split(",")
    for spec in (a.specs or ";".join(VECC_SPECS)).split(";"):
        cols, rows, vals, n = generators.generate(spec)
        nnz = len(vals)
        for mode in res["modes"]:
            ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: None)
            A = ctx.create_matrix(cols, rows, vals, n, nnz, layout="stream")
            vecs = [ctx.create_vector(n) for _ in range(5)]
            ctx.upload(vecs[0], generators.reference_rhs(n))
            dinv = ctx.jacobi(A, protected=True) if a.precond == "jacobi" else None
            kinds = [0] + strides
            for k in kinds:  # warm-up: first launches, the graph's instantiation path
                timed_solve(ctx, A, vecs, n, max(k, 5), k, dinv, vecc=True)
            per = {k: [] for k in kinds}
            for _ in range(a.blocks):
                for k in kinds:
                    ms, itr = timed_solve(ctx, A, vecs, n, a.iters, k, dinv, vecc=True)
                    assert itr == a.iters, (spec, mode, k, itr)  # every iteration live in both loops
                    per[k].append(ms / a.iters)
            host = statistics.median(per[0])
            dev = {k: statistics.median(per[k]) for k in strides}
            best = min(dev.values())
            row = dict(spec=spec, fmt="csr", mode=mode, layout=ctx.matrix_info(A)[0], vector_ecc=True,
                       precond=a.precond, n=n, nnz=nnz, ms_per_iter_host_vecc=host,
                       ms_per_iter_device_vecc={str(k): v for k, v in dev.items()},
                       ratio_device_over_host={str(k): v / host for k, v in dev.items()},
                       best_stride=min(k for k in strides if dev[k] <= 1.02 * best),
                       frozen_spmv_worst={str(k): k - 1 for k in strides},
                       blocks={str(k): v for k, v in per.items()})
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            ctx.close()
        del cols, rows, vals


CHECK_SPECS = ("laplace5:3162,3162", "laplace5:1000,1000")
CHECK_STRIDES = (16,)


def check_main(a, res):
    """--check-every N: cg_solve_device without and with residual checks, one row per (matrix, mode).  Kinds:
    ("plain", stride) and ("check", stride), the checkpoint vector made once and passed in"""
    strides = [int(s) for s in (a.strides or ",".join(str(s) for s in CHECK_STRIDES)).split(",")]
    res["check_every"] = a.check_every
    res["modes"] = a.modes.split(",")
    for spec in (a.specs or ";".join(CHECK_SPECS)).split(";"):
        cols, rows, vals, n = generators.generate(spec)
        nnz = len(vals)
        for mode in res["modes"]:
            ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: None)
            A = ctx.create_matrix(cols, rows, vals, n, nnz)
            vecs = [ctx.create_vector(n) for _ in range(5)]
            ckpt = ctx.create_vector(n)
            ctx.upload(vecs[0], generators.reference_rhs(n))
            dinv = ctx.jacobi(A) if a.precond == "jacobi" else None
            kinds = [(kind, st) for st in strides for kind in ("plain", "check")]
            checks = []

            def run(kind, its):
                kw = dict(check_every=a.check_every, x_ckpt=ckpt, on_check=lambda *c: checks.append(c[2])) \
                    if kind[0] == "check" else {}
                ctx.upload(vecs[1], np.zeros(n))
                ctx.synchronize()
                t0 = time.perf_counter()
                itr, _ = amd.cg_solve_device(ctx, A, *vecs, max_itrs=its, conv_threshold=THRESHOLD, stride=kind[1],
                                             precond=dinv, **kw)
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e3, itr
            for kind in kinds:  # warm-up: first launches, the graphs' instantiation path
                run(kind, max(kind[1], a.check_every, 5))
            per = {kind: [] for kind in kinds}
            n_checks = 0
            for _ in range(a.blocks):
                for kind in kinds:
                    del checks[:]
                    ms, itr = run(kind, a.iters)
                    assert itr == a.iters and all(checks), (spec, mode, kind, itr, checks)  # all live, nothing rolled back
                    n_checks = max(n_checks, len(checks))
                    per[kind].append(ms / a.iters)
            plain = {st: statistics.median(per[("plain", st)]) for st in strides}
            chk = {st: statistics.median(per[("check", st)]) for st in strides}
            row = dict(spec=spec, fmt="csr", mode=mode, layout=ctx.matrix_info(A)[0], precond=a.precond, n=n, nnz=nnz,
                       check_every=a.check_every, checks_per_solve=n_checks,
                       ms_per_iter_plain={str(st): v for st, v in plain.items()},
                       ms_per_iter_check={str(st): v for st, v in chk.items()},
                       ratio_check_over_plain={str(st): chk[st] / plain[st] for st in strides},
                       blocks={"%s:%d" % kind: v for kind, v in per.items()})
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            ctx.close()
        del cols, rows, vals


TRAIL_SPECS = ("laplace5:1000,1000", "laplace5:3162,3162")
TRAIL_STRIDES = (4, 16)


def trail_main(a, res):
    """--trail-ecc: cg_solve_device without and with trail_ecc=True, one row per (matrix, mode).  Kinds: ("plain",
    stride) and ("trail", stride)"""
    strides = [int(s) for s in (a.strides or ",".join(str(s) for s in TRAIL_STRIDES)).split(",")]
    res["trail_ecc"] = True
    res["vector_ecc"] = bool(a.vector_ecc)
    res["modes"] = a.modes.split(",")
    for spec in (a.specs or ";".join(TRAIL_SPECS)).split(";"):
        cols, rows, vals, n = generators.generate(spec)
        nnz = len(vals)
        for mode in res["modes"]:
            ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: None)
            A = ctx.create_matrix(cols, rows, vals, n, nnz, layout="stream" if a.vector_ecc else None)
            vecs = [ctx.create_vector(n) for _ in range(5)]
            dinv = ctx.jacobi(A, protected=a.vector_ecc) if a.precond == "jacobi" else None
            kinds = [(kind, st) for st in strides for kind in ("plain", "trail")]

            def run(kind, its):
                kw = {"trail_ecc": True} if kind[0] == "trail" else {}
                if a.vector_ecc:
                    kw["vector_ecc"] = True
                ctx.upload(vecs[0], generators.reference_rhs(n))  # (a protected solve leaves codewords in b)
                ctx.upload(vecs[1], np.zeros(n))
                ctx.synchronize()
                t0 = time.perf_counter()
                itr, _ = amd.cg_solve_device(ctx, A, *vecs, max_itrs=its, conv_threshold=THRESHOLD, stride=kind[1],
                                             precond=dinv, **kw)
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e3, itr
            for kind in kinds:  # warm-up: first launches, the graphs' instantiation path
                run(kind, max(kind[1], 5))
            per = {kind: [] for kind in kinds}
            for _ in range(a.blocks):
                for kind in kinds:
                    ms, itr = run(kind, a.iters)
                    assert itr == a.iters, (spec, mode, kind, itr)  # every iteration live in both loops
                    per[kind].append(ms / a.iters)
            plain = {st: statistics.median(per[("plain", st)]) for st in strides}
            trail = {st: statistics.median(per[("trail", st)]) for st in strides}
            row = dict(spec=spec, fmt="csr", mode=mode, layout=ctx.matrix_info(A)[0], precond=a.precond,
                       vector_ecc=bool(a.vector_ecc), n=n, nnz=nnz,
                       ms_per_iter_plain={str(st): v for st, v in plain.items()},
                       ms_per_iter_trail={str(st): v for st, v in trail.items()},
                       ratio_trail_over_plain={str(st): trail[st] / plain[st] for st in strides},
                       blocks={"%s:%d" % kind: v for kind, v in per.items()})
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            ctx.close()
        del cols, rows, vals


def block_trail_main(a, res):
    """--trail-ecc --rhs: cg_solve_block_device without and with trail_ecc=True, one row per (matrix, mode, K).  Kinds,
    strides, specs and modes as trail_main's"""
    strides = [int(s) for s in (a.strides or ",".join(str(s) for s in TRAIL_STRIDES)).split(",")]
    res["trail_ecc"] = True
    res["vector_ecc"] = bool(a.vector_ecc)
    res["rhs"] = [int(k) for k in a.rhs.split(",")]
    res["modes"] = a.modes.split(",")
    for spec in (a.specs or ";".join(TRAIL_SPECS)).split(";"):
        cols, rows, vals, n = generators.generate(spec)
        nnz = len(vals)
        for mode in res["modes"]:
            ctx = amd.HIPContext(mode, "csr", on_event=lambda ev, fatal: None)
            A = ctx.create_matrix(cols, rows, vals, n, nnz, layout="stream")
            dinv = ctx.jacobi(A) if a.precond == "jacobi" else None
            for k in res["rhs"]:
                vecs = [ctx.create_block(n, k) for _ in range(5)]
                b = np.random.default_rng(7).random((n, k)) + 0.5
                kinds = [(kind, st) for st in strides for kind in ("plain", "trail")]

                def run(kind, its):
                    kw = {"trail_ecc": True} if kind[0] == "trail" else {}
                    if a.vector_ecc:
                        kw["vector_ecc"] = True
                    ctx.upload(vecs[0], b)  # (a protected solve leaves codewords in B)
                    ctx.upload(vecs[1], np.zeros((n, k)))
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    itrs, _ = amd.cg_solve_block_device(ctx, A, *vecs, max_itrs=its, conv_threshold=THRESHOLD,
                                                        stride=kind[1], precond=dinv, **kw)
                    ctx.synchronize()
                    return (time.perf_counter() - t0) * 1e3, list(itrs)
                for kind in kinds:  # warm-up: first launches, the graphs' instantiation path
                    run(kind, max(kind[1], 5))
                per = {kind: [] for kind in kinds}
                for _ in range(a.blocks):
                    for kind in kinds:
                        ms, itrs = run(kind, a.iters)
                        assert itrs == [a.iters] * k, (spec, mode, k, kind, itrs)  # every column live in both loops
                        per[kind].append(ms / a.iters)
                plain = {st: statistics.median(per[("plain", st)]) for st in strides}
                trail = {st: statistics.median(per[("trail", st)]) for st in strides}
                row = dict(spec=spec, fmt="csr", mode=mode, layout=ctx.matrix_info(A)[0], precond=a.precond,
                           vector_ecc=bool(a.vector_ecc), rhs=k, n=n, nnz=nnz,
                           ms_per_iter_plain={str(st): v for st, v in plain.items()},
                           ms_per_iter_trail={str(st): v for st, v in trail.items()},
                           ratio_trail_over_plain={str(st): trail[st] / plain[st] for st in strides},
                           blocks={"%s:%d" % kind: v for kind, v in per.items()})
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                for v in vecs:
                    ctx.destroy_vector(v)
            ctx.close()
        del cols, rows, vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--specs", default=None, help="matrices, separated by ';'")
    ap.add_argument("--strides", default=None)
    ap.add_argument("--precond", choices=("none", "jacobi"), default="none")
    ap.add_argument("--rhs", default=None, help="K[,K...]: the block loops with K right-hand sides")
    ap.add_argument("--modes", default="none,secded", help="with --rhs or --vector-ecc: the ECC modes")
    ap.add_argument("--vector-ecc", action="store_true", help="the loops on protected vectors")
    ap.add_argument("--check-every", type=int, default=0,
                    help="N: cg_solve_device with a residual check every N iterations against the same loop without")
    ap.add_argument("--trail-ecc", action="store_true",
                    help="cg_solve_device(trail_ecc=True) against the same loop without the keyword")
    a = ap.parse_args()
    if a.trail_ecc and a.check_every:
        ap.error("--trail-ecc does not go with --check-every: the checked loop has no protected trail")
    if a.vector_ecc and a.rhs and a.precond == "jacobi":
        ap.error("--vector-ecc --rhs does not go with --precond jacobi: the protected block loops have no Jacobi form")
    if a.check_every and (a.vector_ecc or a.rhs):
        ap.error("--check-every goes with neither --vector-ecc nor --rhs: those loops have no residual checks")
    if a.check_every < 0:
        ap.error("--check-every must be >= 0")
    argv = [v for i, v in enumerate(sys.argv) if v != "--out" and (i == 0 or sys.argv[i - 1] != "--out")]
    res = {"cmd": " ".join(argv), "iters": a.iters, "blocks": a.blocks, "threshold": THRESHOLD,
           "precond": a.precond, "rows": []}
    if a.trail_ecc and a.rhs:
        a.out = a.out or os.path.join(ROOT, "profiles", "device_loop_bench_block_trail.json")
        block_trail_main(a, res)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        return 0
    if a.trail_ecc:
        a.out = a.out or os.path.join(ROOT, "profiles", "device_loop_bench_trail.json")
        trail_main(a, res)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        return 0
    if a.check_every:
        a.out = a.out or os.path.join(ROOT, "profiles", "device_loop_bench_check.json")
        check_main(a, res)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        return 0
    if a.rhs and a.vector_ecc:
        a.out = a.out or os.path.join(ROOT, "profiles", "device_loop_bench_block_vecc.json")
        block_vecc_main(a, res)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        return 0
    if a.rhs:
        a.out = a.out or os.path.join(ROOT, "profiles", "device_loop_bench_block.json")
        block_main(a, res)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        return 0
    if a.vector_ecc:
        a.out = a.out or os.path.join(ROOT, "profiles", "device_loop_bench_vecc_precond.json" if a.precond == "jacobi"
                                      else "device_loop_bench_vecc.json")
        vecc_main(a, res)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        return 0
    a.out = a.out or "device_loop_bench.json"
    strides = [int(s) for s in (a.strides or ",".join(str(s) for s in STRIDES)).split(",")]
    for spec in (a.specs or ";".join(SPECS)).split(";"):
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
