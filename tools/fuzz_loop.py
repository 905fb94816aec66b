#!/usr/bin/env python3
"""CG-shaped call sequences through the C ABI against a numpy model, once per setting of the switches that keep state
between the calls of the host-scalar loop: the x update applied inside the next SpMV (ABFT_HIP_X_IN_SPMV), the
run-ahead of calc_p and calc_r (ABFT_HIP_AHEAD) and the speculation (ABFT_HIP_SPECULATE).

    python tools/fuzz_loop.py FIRST_SEED COUNT

The cases come from tools/fuzz_gen.py (loop_case): one to three solves in one context taking turns, alpha and beta
formed from the scalars handed back (so the run-ahead and the speculation arm), scalars one ulp off, constants, extra
calls of every kind in every gap of an iteration, injects, right-hand sides scaled to the ends of the exponent range.

Per case:
  * model -- every downloaded vector and all vectors at the end equal the numpy model (w = the oracle's SpMV,
    x + alpha * p, r - alpha * w, r + beta * p, a multiply and an add each, with the alpha and beta handed in) in
    every bit, a NaN matching a NaN; scalars within 1e-12 of the sum of the magnitudes of their terms.  Not held:
    scalars of a solve scaled by 2^-530 (subnormal sums carry no relative precision), and everything in a case with a
    standing `constraints` violation (the oracle, like the reference, stops at the fatal event; what the row holds
    after it is not the reference's to say) -- those are held across the configurations only;
  * transparency -- every scalar, every vector and the drained events are the same bits in all six configurations,
    and the events are the oracle's.  One exception, as everywhere in this project's comparisons (tests/_ieee.py:
    ieee_equal): a NaN matches a NaN of another sign or payload.  Once a solve has converged to r = 0, alpha is 0 / 0,
    and which operand's NaN an addition of two NaNs passes on depends on the order the compiler gave the operands in
    each kernel: r + beta * p out of calc_p and out of the fused calc_px differ in the sign of such a NaN;
  * counters -- zero where a switch is off, bounded by the iterations played, the arming rule's (tests/_ahead.py:
    expected) in a case without extra calls, and at least one commit / absorbed update where the case holds three
    clean iterations in a row (fuzz_gen.loop_tags: must_commit).

The summary prints the sums of the counters per configuration and the cases per tag; a campaign that never dropped a
run-ahead in flight at level 1 and at level 2, never flushed a pending update or never dropped a speculation fails."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _ahead import expected, ulps  # noqa: E402
from _ieee import ieee_diff, ieee_equal  # noqa: E402
from _oracle import COO, CSR, OracleMatrix  # noqa: E402

import fuzz_gen  # noqa: E402

import abft_sparse_cg_amd as amd  # noqa: E402
from abft_sparse_cg_amd import capi  # noqa: E402
from abft_sparse_cg_amd.context import fdiv  # noqa: E402

SWITCHES = ["ABFT_HIP_X_IN_SPMV", "ABFT_HIP_AHEAD", "ABFT_HIP_SPECULATE"]
# the first one carries the model; the others are compared with it
CONFIGS = [("x_in_spmv_off", {"ABFT_HIP_X_IN_SPMV": "0"}),
           ("ahead0", {"ABFT_HIP_X_IN_SPMV": "1", "ABFT_HIP_AHEAD": "0"}),
           ("ahead1", {"ABFT_HIP_X_IN_SPMV": "1", "ABFT_HIP_AHEAD": "1"}),
           ("ahead2", {"ABFT_HIP_X_IN_SPMV": "1", "ABFT_HIP_AHEAD": "2"}),
           ("unset", {}),
           ("speculate", {"ABFT_HIP_SPECULATE": "1"})]
COUNTERS = ["committed_p", "committed_r", "dropped", "absorbed", "flushed", "spec_commits", "spec_drops"]
LOOP_VECTORS = "xrpwqstub"


class Mismatch(Exception):
    pass


def context(mode, env, on_event):
    """a context created under `env` (the library reads the switches in abft_hip_init), the environment as before"""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return amd.HIPContext(mode, "csr", on_event=on_event)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def spec_stats(ctx):
    t, d = C.c_long(), C.c_long()
    capi.check(ctx.L.abft_hip_speculation_stats(ctx.h, C.byref(t), C.byref(d)))
    return t.value, d.value


def content(seed, shape, scale, shift=0.5):
    return scale * (np.random.default_rng(seed).random(shape) - shift)


class Player:
    """one case on one context.  model=True: the numpy model runs beside it and every value read is held against it."""

    def __init__(self, case, env, model):
        self.c, self.model = case, model
        self.events, self.obs, self.trace = [], [], []
        self.fatal = False
        self.mpend = []  # the oracle's events since the library last delivered any
        self.batches = []  # (what one drain delivered, what the oracle had reported until then)
        self.hold = model and not case.tags["event_every_spmv"]
        self.ctx = context(case.mode, env, self.on_event)
        self.S = []
        self.profiling = False

    def on_event(self, ev, fatal):
        self.events.extend(ev)
        self.fatal = self.fatal or fatal
        self.batches.append((list(ev), self.mpend))
        self.mpend = []

    # ---- what is read ----
    def scalar(self, got, want=None, tol=0.0, s=None):
        self.obs.append(np.float64(got))
        if self.hold and want is not None and self.c.solves[s]["scale"] != -530 and np.isfinite(want):
            if not abs(got - want) <= tol:
                raise Mismatch("scalar %r, the model's %r (tolerance %r)" % (got, float(want), float(tol)))

    def vector(self, got, want=None):
        self.obs.append(np.array(got, dtype=np.float64).reshape(-1))
        if self.hold and want is not None and not ieee_equal(got, want):
            raise Mismatch("vector differs from the model at (index, got, model) %s" % (ieee_diff(got, want, 4),))

    def dot(self, s, a, b):
        v = self.S[s]
        got = self.ctx.dot(v["V"][a], v["V"][b])
        if self.model:
            with np.errstate(all="ignore"):
                self.scalar(got, np.dot(v["M"][a], v["M"][b]), 1e-12 * np.abs(v["M"][a] * v["M"][b]).sum(), s)
        else:
            self.scalar(got)
        return got

    def spmv_model(self, v, src, dst, o=None):
        """(before the library's call where that call drains: the oracle's events must be there when it delivers)"""
        if self.model:
            o = o or v["o"]
            v["M"][dst] = o.spmv(v["M"][src])
            ev, fatal = o.events()
            self.mpend += ev

    def events_hold(self):
        """Every drain delivered what the oracle had reported since the one before: the same events, or, where they are
        fatal ones (a constraints violation), one of them -- a drain hands on the events sorted and cut after the first
        fatal one, as one run of the reference prints them (deliberate difference 6) -- and
        nothing the oracle reported is left over at the end."""
        for lib, ora in self.batches:
            if self.c.mode == "constraints":
                ok = len(lib) == 1 and lib[0] in ora
            else:
                ok = sorted(lib) == sorted(ora)
            if not ok:
                return "a drain delivered %s, the oracle had reported %s" % (lib[:6], ora[:6])
        if self.mpend:
            return "the oracle's events %s were never delivered" % (self.mpend[:6],)
        return None

    # ---- the case ----
    def setup(self):
        ctx, c = self.ctx, self.c
        wants_precond = {i[1] for i in c.script if i[0] == "extra" and i[2] == "precond"}
        for s, sv in enumerate(c.solves):
            cols, rows, vals, n = fuzz_gen.loop_matrix(sv["spec"])
            A = ctx.create_matrix(cols, rows, vals, n, len(vals))
            if ctx.matrix_info(A)[0] != "stream":
                raise Mismatch("matrix %r is not in the streaming layout" % (sv["spec"],))
            sc = 2.0 ** sv["scale"]
            rng = np.random.default_rng(sv["rhs_seed"])
            rhs = sc * (rng.random(n) + 0.5)
            M = {"x": sc * 0.125 * (rng.random(n) - 0.5), "r": rhs.copy(), "p": rhs.copy(), "w": np.zeros(n), "b": rhs.copy()}
            for name in "qstu":
                M[name] = sc * (rng.random(n) - 0.5)
            V = {name: ctx.create_vector(n) for name in LOOP_VECTORS}
            for name in LOOP_VECTORS:
                ctx.upload(V[name], M[name])
            v = dict(A=A, V=V, M=M, n=n, sc=sc, mat=(cols, rows, vals, n), second={}, blocks={}, alpha=0.25, pw=None,
                     o=OracleMatrix(CSR, c.mode, cols, rows, vals, n) if self.model else None)
            if s in wants_precond:  # (made before any inject: the diagonal it reads is the clean one)
                v["dinv"] = ctx.jacobi(A, strict=False)
                v["dm"] = ctx.download(v["dinv"])
            self.S.append(v)
        for s in range(len(self.S)):
            self.S[s]["rr"] = self.dot(s, "r", "r")

    def second(self, v, which):
        """matrix B of the same triplets: COO, or CSR in the sweep / panel layout (tests/_x_in_spmv.py: run)"""
        if which not in v["second"]:
            ctx = self.ctx
            cols, rows, vals, n = v["mat"]
            old = os.environ.get("ABFT_HIP_LAYOUT")
            if which != "coo":
                os.environ["ABFT_HIP_LAYOUT"] = which
            ctx.fmt = capi.FMT_COO if which == "coo" else capi.FMT_CSR
            try:
                B = ctx.create_matrix(cols, rows, vals, n, len(vals))
            finally:
                ctx.fmt = capi.FMT_CSR
                os.environ.pop("ABFT_HIP_LAYOUT", None)
                if old is not None:
                    os.environ["ABFT_HIP_LAYOUT"] = old
            o = OracleMatrix(COO if which == "coo" else CSR, self.c.mode, cols, rows, vals, n) if self.model else None
            v["second"][which] = (B, o)
        return v["second"][which]

    def extra(self, s, kind, args):
        ctx, v = self.ctx, self.S[s]
        V, M, n, sc = v["V"], v["M"], v["n"], v["sc"]
        if kind == "download":
            self.vector(ctx.download(V[args[0]]), M[args[0]])
        elif kind == "upload":
            M[args[0]] = content(args[1], n, sc)
            ctx.upload(V[args[0]], M[args[0]])
        elif kind in ("copy_in", "copy_out"):
            ctx.copy_vector(V[args[0]], V[args[1]])
            M[args[0]] = M[args[1]].copy()
        elif kind == "map_unmap":
            h = ctx.map_vector(V[args[0]])
            self.vector(h.copy(), M[args[0]])
            ctx.unmap_vector(V[args[0]], h)
        elif kind == "view":
            ctx.destroy_vector(ctx.view_vector(V[args[0]], 0, n))
        elif kind == "ptr":
            if not V[args[0]].device_ptr:
                raise Mismatch("no device pointer")
        elif kind == "dot":
            self.dot(s, args[0], args[1])
        elif kind == "dot_rr":
            self.dot(s, "r", "r")
        elif kind == "dot_pw":
            self.dot(s, "p", "w")
        elif kind == "spmv_other":
            ctx.spmv(v["A"], V[args[0]], V[args[1]])
            self.spmv_model(v, args[0], args[1])
        elif kind == "spmv_second":
            B, o = self.second(v, args[0])
            ctx.spmv(B, V[args[1]], V[args[2]])
            self.spmv_model(v, args[1], args[2], o)
        elif kind == "calc_xr_again":
            self.calc_xr(s, v["alpha"])
        elif kind == "calc_p_other":
            ctx.calc_p(V[args[0]], V[args[1]], args[2])
            with np.errstate(all="ignore"):
                M[args[0]] = M[args[1]] + args[2] * M[args[0]]
        elif kind == "drain":
            ctx._drain()
        elif kind == "synchronize":
            ctx.synchronize()
        elif kind == "residual_gap":
            self.spmv_model(v, "x", "s")
            gap2, tt2 = ctx.residual_gap(v["A"], V["b"], V["x"], V["r"], V["s"])
            self.scalar(gap2)
            with np.errstate(all="ignore"):
                t = M["b"] - M["s"]
                self.scalar(tt2, np.dot(t, t), 1e-12 * np.dot(t, t), s)
        elif kind == "block":
            k = args[0]
            if k not in v["blocks"]:
                v["blocks"][k] = (ctx.create_block(n, k), ctx.create_block(n, k))
            X, Y = v["blocks"][k]
            xm = content(args[1], (n, k), sc)
            ctx.upload(X, xm)
            ctx.upload(Y, np.zeros((n, k)))  # (a row the constraints checks give up on is left as it was)
            ym = None
            if self.model:  # every column the oracle's SpMV of it; the events those of one SpMV
                ym = np.empty((n, k))
                for j in range(k):
                    ym[:, j] = v["o"].spmv(np.ascontiguousarray(xm[:, j]))
                    ev, _ = v["o"].events()
                    if j == 0:
                        self.mpend += ev
            ctx.spmm(v["A"], X, Y, k)
            got = ctx.dot_block(X, Y, k)
            for j in range(k):
                with np.errstate(all="ignore"):
                    self.scalar(got[j], None if ym is None else np.dot(xm[:, j], ym[:, j]),
                                0.0 if ym is None else 1e-12 * np.abs(xm[:, j] * ym[:, j]).sum(), s)
            self.vector(ctx.download(Y), ym)
        elif kind == "precond":
            a, b = args
            dinv, dm = v["dinv"], v["dm"]
            with np.errstate(all="ignore"):
                rz, rr = ctx.precond_start(V["q"], dinv, V["s"])
                M["s"] = dm * M["q"]
                self.scalar(rz, np.dot(M["q"], M["s"]), 1e-12 * np.abs(M["q"] * M["s"]).sum(), s)
                self.scalar(rr, np.dot(M["q"], M["q"]), 1e-12 * np.dot(M["q"], M["q"]), s)
                rz, rr = ctx.calc_xr_precond(V["t"], V["q"], V["s"], V["u"], dinv, a)
                M["t"] = M["t"] + a * M["s"]
                M["q"] = M["q"] - a * M["u"]
                z = dm * M["q"]
                self.scalar(rz, np.dot(M["q"], z), 1e-12 * np.abs(M["q"] * z).sum(), s)
                self.scalar(rr, np.dot(M["q"], M["q"]), 1e-12 * np.dot(M["q"], M["q"]), s)
                ctx.calc_p_precond(V["s"], V["q"], dinv, b)
                M["s"] = z + b * M["s"]
        elif kind == "profile":
            if not self.profiling:
                ctx.profile(0xF)
            else:
                for k in range(4):
                    ctx.profile_read(k)
                ctx.profile(0)
            self.profiling = not self.profiling
        elif kind == "graph":  # capture one copy, replay it once (a capture is refused while kernels are bracketed)
            if self.profiling:
                ctx.profile(0)
                self.profiling = False
            ctx.graph_begin()
            ctx.copy_vector(V["s"], V["q"])
            graph = ctx.graph_end()
            ctx.graph_launch(graph)
            ctx.synchronize()
            ctx.graph_destroy(graph)
            M["s"] = M["q"].copy()
        elif kind == "respare":
            ctx.destroy_vector(V["q"])
            V["q"] = ctx.create_vector(n)
            M["q"] = content(args[0], n, sc)
            ctx.upload(V["q"], M["q"])
        elif kind == "inject":
            if self.model:
                v["o"].inject(args[0], list(args[1]))
            ctx.inject_at(v["A"], args[0], list(args[1]))
        else:
            raise ValueError(kind)

    def calc_xr(self, s, alpha):
        v = self.S[s]
        V, M = v["V"], v["M"]
        got = self.ctx.calc_xr(V["x"], V["r"], V["p"], V["w"], alpha)
        with np.errstate(all="ignore"):
            M["x"] = M["x"] + alpha * M["p"]
            M["r"] = M["r"] - alpha * M["w"]
            want = np.dot(M["r"], M["r"])
            self.scalar(got, want, 1e-12 * want, s)
        return got

    def play(self):
        self.setup()
        ctx = self.ctx
        for item in self.c.script:
            self.trace.append(item)
            s = item[1]
            v = self.S[s]
            V, M = v["V"], v["M"]
            if item[0] == "extra":
                self.extra(s, item[2], item[3])
            elif item[0] == "spmv":
                ctx.spmv(v["A"], V["p"], V["w"])
                self.spmv_model(v, "p", "w")
            elif item[0] == "dot":
                v["pw"] = self.dot(s, "p", "w")
            elif item[0] == "dot_copies":
                ctx.copy_vector(V["q"], V["p"])
                ctx.copy_vector(V["s"], V["w"])
                M["q"], M["s"] = M["p"].copy(), M["w"].copy()
                v["pw"] = self.dot(s, "q", "s")
            elif item[0] == "calc_xr":
                v["alpha"] = ulps(fdiv(v["rr"], v["pw"]), item[3]) if item[2] == "q" else item[3]
                self.obs.append(np.float64(v["alpha"]))
                v["rr_new"] = self.calc_xr(s, v["alpha"])
            elif item[0] == "calc_p":
                beta = ulps(fdiv(v["rr_new"], v["rr"]), item[3]) if item[2] == "q" else item[3]
                self.obs.append(np.float64(beta))
                ctx.calc_p(V["p"], V["r"], beta)
                with np.errstate(all="ignore"):
                    M["p"] = M["r"] + beta * M["p"]
                v["rr"] = v["rr_new"]
        self.trace.append(("the end",))
        for s, v in enumerate(self.S):
            for name in LOOP_VECTORS:
                self.trace.append(("download", s, name))
                self.vector(ctx.download(v["V"][name]), v["M"][name])
        ctx._drain()
        return dict(obs=self.obs, events=list(self.events), fatal=self.fatal, events_msg=self.events_hold() if self.model else None,
                    counters=ctx.ahead_stats() + ctx.x_in_spmv_stats() + spec_stats(ctx))

    def close(self):
        self.ctx.close()
        for v in self.S:
            if v["o"]:
                v["o"].close()
            for _, o in v["second"].values():
                if o:
                    o.close()


def as_ahead_script(case, scalars):
    """the flat script of a case without extra calls as tests/_ahead.py writes one: a dict per iteration.  What counts
    is what was handed in: a constant that happens to be the quotient (0.0 once r.r is 0) is the quotient; a p.w that
    came from copies is not the fused one, whatever its bits."""
    its, rr = [], scalars[0]
    for item in case.script:
        if item[0] == "spmv":
            its.append({})
            pw, alpha, rr_new, beta = scalars[1 + 4 * (len(its) - 1):5 + 4 * (len(its) - 1)]
        elif item[0] == "dot_copies":
            its[-1]["alpha_ulps"] = 1
        elif item[0] == "calc_xr" and not same_bits(alpha, fdiv(rr, pw)):
            its[-1]["alpha_ulps"] = 1
        elif item[0] == "calc_p":
            if not same_bits(beta, fdiv(rr_new, rr)):
                its[-1]["beta_ulps"] = 1
            rr = rr_new
    return its


def check_counters(case, name, env, res, base):
    cp, cr, dropped, absorbed, flushed, sc, sd = res["counters"]
    tags, its = case.tags, case.iterations
    xin = env.get("ABFT_HIP_X_IN_SPMV") == "1" or (not env and case.mode == "none")
    level = int(env.get("ABFT_HIP_AHEAD", "1")) if xin else 0
    if level == 0 and (cp, cr, dropped) != (0, 0, 0):
        return "run-ahead counters %s with the run-ahead off" % ((cp, cr, dropped),)
    if level == 1 and cr:
        return "committed_r = %d at level 1" % cr
    if not xin and (absorbed, flushed) != (0, 0):
        return "x-in-SpMV counters %s with the switch off" % ((absorbed, flushed),)
    if "ABFT_HIP_SPECULATE" not in env and (sc, sd) != (0, 0):
        return "speculation counters %s with the switch off" % ((sc, sd),)
    more = sum(1 for i in case.script if i[0] == "extra" and i[2] in ("calc_xr_again", "calc_p_other"))
    if max(cp, cr) + dropped > its + more or absorbed + flushed > its + more or sc + sd > its + more:
        return "counters %s exceed the %d iterations (+ %d extra calc_xr / calc_p)" % (res["counters"], its, more)
    if tags["plain_loop"] and env.get("ABFT_HIP_X_IN_SPMV") == "1":
        scalars = [float(v) for v in base["obs"][:1 + 4 * its]]  # rr0, then pw, alpha, rr_new, beta per iteration
        want = expected(as_ahead_script(case, scalars), scalars, level) if level else (0, 0, 0)
        if (cp, cr, dropped) != want:
            return "run-ahead counters %s, the arming rule gives %s" % ((cp, cr, dropped), want)
    if tags["must_commit"]:
        if level >= 1 and cp < 1:
            return "three clean iterations in a row and no calc_p committed"
        if level == 2 and cr < 1:
            return "three clean iterations in a row and no calc_xr committed"
        if xin and absorbed < 1:
            return "three clean iterations in a row and no x update absorbed"
        if "ABFT_HIP_SPECULATE" in env and sc < 1:
            return "three clean iterations in a row and no speculation committed"
    return None


def same_bits(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and ieee_equal(a, b)


def one_case(seed, sums):
    """-> a message, or None"""
    case = fuzz_gen.loop_case(seed)
    what = "seed %d (mode %s, %s, %d iterations)" % (seed, case.mode, [v["spec"] for v in case.solves], case.iterations)
    base = None
    for k, (name, env) in enumerate(CONFIGS):
        p = Player(case, env, model=k == 0)
        try:
            res = p.play()
        except Mismatch as e:
            return "%s, configuration %s: %s; the last calls: %s" % (what, name, e, p.trace[-6:])
        except Exception as e:  # noqa: BLE001
            return "%s, configuration %s: exception %r; the last calls: %s" % (what, name, e, p.trace[-6:])
        finally:
            p.close()
        if k == 0:
            base = res
            if res["events_msg"]:
                return "%s, configuration %s: %s" % (what, name, res["events_msg"])
            if res["fatal"] and not case.tags["event_every_spmv"]:
                return "%s: a fatal event %s" % (what, res["events"][:6])
        else:
            if len(res["obs"]) != len(base["obs"]):
                return "%s, configuration %s: %d values read, %d without the switches" % (what, name, len(res["obs"]), len(base["obs"]))
            for j, (a, b) in enumerate(zip(res["obs"], base["obs"])):
                if not same_bits(a, b):
                    return "%s, configuration %s: value %d read differs from the run without the switches (%s vs %s)" % (
                        what, name, j, np.atleast_1d(a)[:3], np.atleast_1d(b)[:3])
            if res["events"] != base["events"]:
                return "%s, configuration %s: events %s, without the switches %s" % (what, name, res["events"][:6], base["events"][:6])
        msg = check_counters(case, name, env, res, base)
        if msg:
            return "%s, configuration %s: %s" % (what, name, msg)
        sums[name] = [a + b for a, b in zip(sums.get(name, [0] * len(COUNTERS)), res["counters"])]
    return None


TAGS = ["must_commit", "three_lengths", "same_length_pair", "switch_inside", "event_every_spmv", "plain_loop"]


def main():
    if len(sys.argv) != 3:
        sys.exit("usage: python tools/fuzz_loop.py FIRST_SEED COUNT")
    first, count = int(sys.argv[1]), int(sys.argv[2])
    sums, bad = {}, 0
    tagged = {t: 0 for t in TAGS + ["scaled_%d" % e for e in fuzz_gen.LOOP_SCALES] + ["in_flight"]}
    for seed in range(first, first + count):
        msg = one_case(seed, sums)
        if msg:
            bad += 1
            print("FAIL " + msg, flush=True)
        tags = fuzz_gen.loop_case(seed).tags
        for t in TAGS:
            tagged[t] += bool(tags[t])
        for e in tags["scaled"]:
            tagged["scaled_%d" % e] += 1
        tagged["in_flight"] += len(tags["in_flight"])
        if (seed - first + 1) % 500 == 0 and seed + 1 < first + count:
            print("... %d cases, %d failures" % (seed - first + 1, bad), flush=True)
    for name, _ in CONFIGS:
        print("config %s: %s" % (name, " ".join("%s=%d" % kv for kv in zip(COUNTERS, sums.get(name, [0] * len(COUNTERS))))), flush=True)
    print("tags: " + " ".join("%s=%d" % kv for kv in tagged.items()), flush=True)
    zero = [0] * len(COUNTERS)
    reached = dict(dropped_level1=sums.get("ahead1", zero)[2], dropped_level2=sums.get("ahead2", zero)[2],
                   flushed=sums.get("ahead1", zero)[4], spec_dropped=sums.get("speculate", zero)[6])
    print("reached: " + " ".join("%s=%d" % kv for kv in reached.items()), flush=True)
    for k, v in reached.items():
        if not v:
            bad += 1
            print("FAIL no case of %d reached %s" % (count, k), flush=True)
    print("fuzz_loop: %d cases, %d failures" % (count, bad), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
