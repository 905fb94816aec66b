#!/usr/bin/env python3
"""Randomised parity campaign on the GPU: HIP path (through the C ABI) against the CPU
oracle on random matrices, modes, layouts and bit flips -- stored words, SpMV results
(bit for bit, two passes: corrections persist), event streams, SpMV-in-two-parts and the
block SpMV.

    python tools/fuzz_parity.py [seconds] [first_seed]

Two families of cases, each with its own seeds (tools/fuzz_gen.py draws both):
  * the first (default): random sparse matrices of all-distinct values, every format, mode and
    layout, up to 3 flips;
  * ABFT_FUZZ_FAMILY=packed: mostly CSR in mode none on the streaming layout -- banded matrices
    of few distinct values whose row blocks pack (CsrPacked), with column spans around every
    threshold of the planner, shards, and up to 40 flips that re-plan blocks; compared after
    creation and after every few flips.  Its summary counts what the cases reached.

A checker like the tests (it loads oracle/ through tests/_oracle.py); prints one line per
failure with the seed that reproduces it, and a summary."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _ieee import ieee_diff, ieee_equal  # noqa: E402
from _oracle import COO, CSR, OracleMatrix  # noqa: E402

import fuzz_gen  # noqa: E402

import abft_sparse_cg_amd as amd  # noqa: E402
from abft_sparse_cg_amd import capi  # noqa: E402

FNAME = {CSR: "csr", COO: "coo"}


def bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def one_case(seed):
    rng = np.random.default_rng(seed)
    d = fuzz_gen.legacy_draw(rng)
    cols, rows, vals, n, fmt, mode, layout, flips, x = (d[k] for k in ("cols", "rows", "vals", "n", "fmt", "mode", "layout", "flips", "x"))
    nnz = len(vals)
    os.environ.update(d["env"])
    seen = []
    o = OracleMatrix(fmt, mode, cols, rows, vals, n)
    ctx = amd.HIPContext(mode, FNAME[fmt], on_event=lambda ev, fatal: seen.append((list(ev), fatal)))
    what = "seed %d: n=%d nnz=%d %s %s layout=%s flips=%s" % (seed, n, nnz, FNAME[fmt], mode, layout, flips)
    try:
        A = ctx.create_matrix(cols, rows, vals, n, nnz)
        if not np.array_equal(ctx.stored_words(A), o.stored_words()):
            return what + " : stored words differ"
        split = fmt == CSR and rng.random() < 0.5 and n > 2
        if split:
            lo = int(rng.integers(0, n))
            ctx.set_interior(A, lo, int(rng.integers(lo, n + 1)))
        for i, b in flips:
            o.inject(i, b)
            ctx.inject_at(A, i, b)
        vx, vy = ctx.create_vector(n), ctx.create_vector(n)
        ctx.upload(vx, x)
        for p in range(2):
            ctx.upload(vy, np.full(n, np.nan))
            seen.clear()
            if split:
                ctx.spmv(A, vx, vy, capi.PART_INTERIOR)
                ctx.spmv(A, vx, vy, capi.PART_BOUNDARY)
            else:
                ctx.spmv(A, vx, vy)
            y = ctx.download(vy)
            ev = [e for evs, _ in seen for e in evs]
            fatal = any(f for _, f in seen)
            want = o.spmv(x)
            oev, ofatal = o.events()
            if (sorted(ev), fatal) != (sorted(oev), ofatal) and not (fatal and ofatal and ev[:1] == oev[:1]):
                return what + " : pass %d events %s fatal=%s, oracle %s fatal=%s" % (p, ev, fatal, oev, ofatal)
            if fatal:
                return None  # the reference stops here
            if not bits_equal(y, want):
                bad = np.nonzero(np.asarray(y).view(np.uint64) != np.asarray(want).view(np.uint64))[0]
                return what + " : pass %d y differs at rows %s" % (p, bad[:5])
        # the block SpMV, where it runs (whole CSR matrix, streaming layout); its draws come from a generator
        # of their own, so that the case's other draws stay what the seed always gave
        rng2 = np.random.default_rng([0x5B, seed])
        if fmt == CSR and n > 0 and ctx.matrix_info(A)[0] == "stream" and rng2.random() < 0.25:
            msg = spmm_check(ctx, A, o, n, x, int(rng2.integers(2, 9)), rng2, seen)
            if msg:
                return what + " : " + msg
        return None
    finally:
        ctx.close()


def spmm_check(ctx, A, o, n, x, k, rng, seen):
    """Y = A X for k columns (the first one x): every column against the oracle's SpMV of it, and the events
    of one SpMV on the same matrix state -> a message, or None"""
    X = rng.standard_normal((n, k))
    X[:, 0] = x
    vX, vY = ctx.create_block(n, k), ctx.create_block(n, k)
    ctx.upload(vX, X)
    ctx.upload(vY, np.full((n, k), np.nan))
    seen.clear()
    ctx.spmm(A, vX, vY, k)
    Y = ctx.download(vY)
    ev, fatal = [e for evs, _ in seen for e in evs], any(f for _, f in seen)
    want = o.spmv(x)
    oev, ofatal = o.events()
    if (sorted(ev), fatal) != (sorted(oev), ofatal) and not (fatal and ofatal and ev[:1] == oev[:1]):
        return "spmm k=%d events %s fatal=%s, oracle %s fatal=%s" % (k, ev, fatal, oev, ofatal)
    for j in range(k if not fatal else 0):
        if j:
            want = o.spmv(np.ascontiguousarray(X[:, j]))
            o.events()
        if not ieee_equal(Y[:, j], want):
            return "spmm k=%d column %d differs: %s" % (k, j, ieee_diff(Y[:, j], want, 4))
    ctx.destroy_vector(vX)
    ctx.destroy_vector(vY)
    return None


def _stats(ctx, A, name):
    a, t, m = C.c_uint32(), C.c_uint32(), C.c_uint32()
    capi.check(getattr(ctx.L, name)(A.h, C.byref(a), C.byref(t), C.byref(m)))
    return a.value, t.value, m.value


def packed_case(seed, reached):
    """one case of the packed family -> (message or None, skipped); `reached` counts fuzz_gen.CLASSES"""
    c = fuzz_gen.packed_case(seed)
    n, nnz = c.n, len(c.vals)
    os.environ["ABFT_HIP_LAYOUT"] = c.layout
    none_csr = (c.fmt, c.mode) == (CSR, "none")
    reached["other_modes"] += not none_csr
    seen = []
    o = OracleMatrix(c.fmt, c.mode, c.cols, c.rows, c.vals, n, n_in=c.n_in, index_base=c.index_base)
    ctx = amd.HIPContext(c.mode, FNAME[c.fmt], on_event=lambda ev, fatal: seen.append((list(ev), fatal)))
    what = ("packed seed %d: %s n=%d n_in=%d base=%d nnz=%d %s %s layout=%s mark=%s path=%s interior=%s values=%s flips=%s"
            % (seed, c.kind, n, c.n_in, c.index_base, nnz, FNAME[c.fmt], c.mode, c.layout, c.mark, c.path, c.interior,
               [s[2] for s in c.segs], [(i, b) for i, b, _ in c.flips]))
    hit = set()
    try:
        if c.spmm_k:  # (the whole-matrix streaming entry; only drawn for whole CSR matrices with layout stream)
            A = ctx.create_matrix(c.cols, c.rows, c.vals, n, nnz, layout="stream")
        else:
            A = ctx.create_matrix(c.cols, c.rows, c.vals, n, nnz, n_in=c.n_in, index_base=c.index_base)
        if c.interior:
            ctx.set_interior(A, *c.interior)
        vx, vy, sc = ctx.create_vector(c.n_in), ctx.create_vector(n), ctx.create_vector(2)
        ctx.upload(vx, c.x)
        state = {}

        def compare(tag):
            """-> message, or None; "fatal" once the oracle reports a fatal event (other modes only)"""
            if not np.array_equal(ctx.stored_words(A), o.stored_words()):
                return tag + ": stored words differ"
            if c.fmt == CSR:
                p, t, m = _stats(ctx, A, "abft_hip_matrix_packed_stats")
                cm = _stats(ctx, A, "abft_hip_matrix_compact_stats")[2]
                if m or cm:
                    return tag + ": %d packed / %d compact codes do not decode to the stored words" % (m, cm)
                if not none_csr and p:
                    return tag + ": %d packed blocks in mode %s" % (p, c.mode)
                if "t" not in state:
                    state["t"], state["p"] = t, p
                    if c.mark == "all" and p != t:
                        return tag + ": every block must pack, %d of %d do" % (p, t)
                    if c.mark == "none" and p:
                        return tag + ": no block may pack, %d of %d do" % (p, t)
                    if p:
                        hit.add("packed_at_creation")
                if t != state["t"] or p > state["p"]:
                    return tag + ": packed / tiles %d / %d after %d / %d" % (p, t, state["p"], state["t"])
                state["dropped"], state["all"], state["p"] = p < state["p"], p == t and t > 0, p
            for ps in range(2):
                ctx.upload(vy, np.full(n, np.nan))
                seen.clear()
                if c.path == "parts":
                    ctx.spmv(A, vx, vy, capi.PART_INTERIOR)
                    ctx.spmv(A, vx, vy, capi.PART_BOUNDARY)
                elif c.path == "dot":
                    capi.check(ctx.L.abft_hip_spmv_dot_part_dev(ctx.h, A.h, vx.h, vy.h, c.row0, sc.device_ptr, capi.PART_ALL))
                else:
                    ctx.spmv(A, vx, vy)
                y = ctx.download(vy)
                ev, fatal = [e for evs, _ in seen for e in evs], any(f for _, f in seen)
                want = o.spmv(c.x)
                oev, ofatal = o.events()
                if (sorted(ev), fatal) != (sorted(oev), ofatal) and not (fatal and ofatal and ev[:1] == oev[:1]):
                    return tag + ": pass %d events %s fatal=%s, oracle %s fatal=%s" % (ps, ev, fatal, oev, ofatal)
                if fatal:
                    return "fatal"  # the reference stops here
                if not ieee_equal(y, want):
                    return tag + ": pass %d y differs: %s" % (ps, ieee_diff(y, want, 4))
                if c.path == "dot":
                    got = float(ctx.download(sc)[0])
                    with np.errstate(all="ignore"):
                        terms = c.x[c.row0:c.row0 + n] * want
                        exact, tol = float(terms.sum()), 1e-12 * float(np.abs(terms).sum()) + 1e-300
                    if np.isfinite(exact) and np.isfinite(tol):
                        if not abs(got - exact) <= tol:
                            return tag + ": pass %d fused dot %r vs %r" % (ps, got, exact)
                    elif np.isfinite(got) or (np.isinf(exact) and got != exact):  # NaN for NaN, an Inf of the same sign
                        return tag + ": pass %d fused dot %r vs %r" % (ps, got, exact)
            return None

        def verdict(msg):
            if msg == "fatal":
                if none_csr:
                    return what + " : a fatal event in mode none", False
                return None, True
            return what + " : " + msg, False

        msg = compare("at creation")
        if msg:
            return verdict(msg)
        at = 0
        for stop in c.checks:
            kinds = set()
            for i, b, cls in c.flips[at:stop]:
                o.inject(i, b)
                ctx.inject_at(A, i, b)
                kinds.add(cls)
            was_all = state.get("all", False)
            msg = compare("after %d flips" % stop)
            if msg:
                return verdict(msg)
            at = stop
            if none_csr:
                if was_all and not state["dropped"]:
                    hit.add("replan_kept")  # every block was packed, every flipped one was planned anew and stayed so
                if state["dropped"] and kinds <= {"in_palette", "new_value", "repeat"}:
                    hit.add("demoted_by_palette")
                if state["dropped"] and kinds == {"column"}:
                    hit.add("demoted_by_span")
        if c.spmm_k:
            msg = spmm_check(ctx, A, o, n, c.x, c.spmm_k, np.random.default_rng([0x5B, seed]), seen)
            if msg:
                return what + " : " + msg, False
        hit |= c.classes & {"k0", "k1", "k2", "k3", "k4", "inject_before_parts", "shard", "spmm"}
        for k in hit:
            reached[k] += 1
        return None, False
    finally:
        ctx.close()


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    packed = os.environ.get("ABFT_FUZZ_FAMILY") == "packed"
    reached = {k: 0 for k in fuzz_gen.CLASSES + ["other_modes"]}
    t0, done, bad, skipped = time.time(), 0, 0, 0
    while time.time() - t0 < budget:
        try:
            if packed:
                msg, skip = packed_case(seed, reached)
                skipped += skip
            else:
                msg = one_case(seed)
        except Exception as e:  # noqa: BLE001
            msg = "seed %d: exception %r" % (seed, e)
        if msg:
            bad += 1
            print("FAIL " + msg, flush=True)
        done += 1
        seed += 1
        if done % 50 == 0:
            print("... %d cases, %d failures, %.0f s" % (done, bad, time.time() - t0), flush=True)
    if packed:
        others = reached["other_modes"]
        print("reached: " + " ".join("%s=%d" % (k, reached[k]) for k in fuzz_gen.CLASSES), flush=True)
        print("skipped after a fatal event: %d of the %d cases in other modes or COO (none of the %d CSR mode-none cases)"
              % (skipped, others, done - others), flush=True)
    print("fuzz: %d cases, %d failures" % (done, bad), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
