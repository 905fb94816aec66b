"""Run-ahead of the host-scalar loop (ABFT_HIP_AHEAD; include/abft_hip.h: abft_hip_ahead_stats; DESIGN.md section 4,
"Fifth cross-call fusion"): calc_p is launched before the host has r.r (level 1), calc_r and calc_p before it has
p.w (level 2), with alpha and beta formed on the device; the caller's calls commit them when they hand in the same
quotients, bit for bit, and everything else drops them.  Transparent: every case plays one script at levels 0, 1 and 2
and compares the bit patterns of every scalar handed back, of x, r, p, w (and the spare q) and the drained events.
The counters say which path ran; what they must read follows from the arming rule (`expected` of tests/_ahead.py):

  * an iteration MATCHES when its calc_xr was handed rr / p.w and its calc_p rr_new / rr, neither a NaN, on vectors
    only the library can see into, with nothing between spmv, dot(p, w), calc_xr and calc_p;
  * a matching iteration that ran as written arms; once armed, level 2 launches behind every spmv(A, p, w), level 1
    behind every calc_xr that was handed its quotient;
  * a drop, or an iteration that does not match, disarms.

So the predicted loop of K iterations commits K - 1 calc_p (and K - 1 calc_xr at level 2) and drops nothing: the
first iteration arms.

The cases at the end -- several solves in one context, right-hand sides scaled to the ends of the exponent range -- are
also held against a numpy model (tests/_ahead.py: model_turns_hold), as tools/fuzz_loop.py holds its random ones."""
import numpy as np
import pytest

import _ahead as H
from _ahead import expected

pytestmark = pytest.mark.gpu

MODES = ["none", "constraints", "sed", "sec7", "sec8", "secded"]
K = 9


@pytest.fixture(autouse=True)
def armed_everywhere(monkeypatch):
    monkeypatch.setenv("ABFT_HIP_X_IN_SPMV", "1")
    for name in ("ABFT_HIP_SPECULATE", "ABFT_HIP_FUSE_X", "ABFT_HIP_FUSE_DOT"):
        monkeypatch.delenv(name, raising=False)


def play(monkeypatch, mode, which, script):
    import abft_sparse_cg_amd as amd
    res = H.levels(amd, monkeypatch, mode, H.matrix(which), script)
    for level in (1, 2):
        assert res[level]["ahead"] == expected(script, res[0]["scalars"], level), (level, res[level]["ahead"])
    return res


# ---- the predicted loop ----
@pytest.mark.parametrize("which", ["lap40", "lap37x41", "rand"])
def test_predicted_loop_commits_all_but_the_first_iteration(which, monkeypatch):
    res = play(monkeypatch, "none", which, H.predicted(K))
    assert res[1]["ahead"] == (K - 1, 0, 0) and res[2]["ahead"] == (K - 1, K - 1, 0)
    assert res[0]["xin"] == res[1]["xin"] == res[2]["xin"] == (K - 2, 1)  # the pending x updates go the same way


@pytest.mark.parametrize("which", ["lap3", "one"])
def test_loop_that_converges_on_the_way(which, monkeypatch):
    """N = 9 and N = 1: r.r reaches (nearly) zero inside the loop; with N = 1 alpha becomes 0 / 0, a NaN the device
    and the host need not encode alike: such an iteration is dropped (level 2) or never launched (level 1)"""
    res = play(monkeypatch, "none", which, H.predicted(K))
    assert res[2]["ahead"][0] >= 1 or which == "one"


# ---- a scalar that is not the quotient ----
@pytest.mark.parametrize("key", ["alpha_ulps", "beta_ulps"])
@pytest.mark.parametrize("off", [1, -1])
def test_one_ulp_off_drops_and_disarms_until_a_matching_iteration(key, off, monkeypatch):
    script = H.predicted(K)
    script[3] = {key: off}
    res = play(monkeypatch, "none", "lap40", script)
    # iterations 2, 3 commit; 4 misses; 5 runs as written and arms; 6 .. K commit
    if key == "alpha_ulps":  # known before calc_p could be launched: level 1 launches nothing
        assert res[1]["ahead"] == (K - 3, 0, 0) and res[2]["ahead"] == (K - 3, K - 3, 1)
    else:  # r is committed (level 2), the calc_p behind it dropped
        assert res[1]["ahead"] == (K - 3, 0, 1) and res[2]["ahead"] == (K - 3, K - 2, 1)


# ---- something else comes first ----
EXTRAS = {
    "download p": [("download", "p")],
    "download x": [("download", "x")],
    "upload r": [("upload", "r")],
    "copy r <- q": [("copy", "r", "q")],
    "view of p": [("view", "p")],
    "pointer of r": [("ptr", "r")],
    "graph_begin": [("graph",)],
    "calc_xr again": [("calc_xr",)],
    "calc_p on another p": [("calc_p", "q", "r")],
    "calc_p with another r": [("calc_p", "p", "q")],
    "destroy p": [("destroy", "p")],
    "close": [("close",)],
    "dot(r, r)": [("dot", "r", "r")],
    "drain": [("drain",)],
    "synchronize": [("synchronize",)],
    "residual_gap": [("residual_gap",)],
    "inject": [("inject", 100, (3,))],  # one bit of a value, mode secded: corrected and reported by the next SpMV
    "spmv of q": [("spmv", "q", "s")],
}
MODE_OF = {"inject": "secded"}  # (armed there by the fixture's ABFT_HIP_X_IN_SPMV=1); every other extra call in mode none


# What the counters read with the extra call in iteration 4 of K = 9, (level 1, level 2), from the arming rule.
# Iterations 2 and 3 commit.  After the miss: AGAIN = iteration 5 matches, runs as written and arms, 6 .. 9 commit;
# NEVER = a vector the caller can now see into (a view, its pointer), a capture, or the end of the script.
# Between calc_xr and calc_p the calc_p of iteration 4 is in flight at both levels (level 2 has committed its r).
P_AGAIN, P_NEVER = ((6, 0, 1), (6, 7, 1)), ((2, 0, 1), (2, 3, 1))
BEFORE_P = {
    "download p": P_AGAIN, "download x": P_AGAIN, "upload r": P_AGAIN, "copy r <- q": P_AGAIN,
    "calc_p on another p": P_AGAIN, "calc_p with another r": P_AGAIN,
    "view of p": P_NEVER, "pointer of r": P_NEVER, "graph_begin": P_NEVER, "destroy p": P_NEVER,
    "close": ((2, 0, 0), (2, 3, 0)),  # ends with the kernel in flight: nobody counts a drop
    # the second calc_xr hands back another r.r than the one the caller goes on with: iteration 5 is handed quotients
    # of the first one's and does not match, 6 arms, 7 .. 9 commit
    "calc_xr again": ((5, 0, 1), (5, 6, 1)),
    # every entry point but the loop's own drops what is in flight, and the loop goes on with the scalars it holds:
    # dot(r, r) hands back the bits calc_xr handed back (one reduction tree) and leaves them where r.r is kept
    "dot(r, r)": P_AGAIN, "drain": P_AGAIN, "synchronize": P_AGAIN, "spmv of q": P_AGAIN,
    # the flipped bit is reported by iteration 5's SpMV, when nothing is in flight (5 is the iteration that arms)
    "inject": P_AGAIN,
    # a residual entry point forgets the r.r kept on the device: iteration 5's calc_xr cannot tell whether its alpha is
    # a quotient, 6 arms, 7 .. 9 commit
    "residual_gap": ((5, 0, 1), (5, 6, 1)),
}
# Between spmv / dot(p, w) and calc_xr only level 2 has anything in flight.  A call that leaves the fused p.w valid (a
# download) lets iteration 4's calc_xr match: level 1 never notices, level 2 is armed again by iteration 4 itself.
# upload, copy and calc_p void the fused product: iteration 4 does not match, 5 arms, 6 .. 9 commit.
X_AGAIN, X_NEVER = ((6, 0, 0), (6, 6, 1)), ((2, 0, 0), (2, 2, 1))
BEFORE_XR = {
    "download p": ((8, 0, 0), (7, 7, 1)), "download x": ((8, 0, 0), (7, 7, 1)),
    "upload r": X_AGAIN, "copy r <- q": X_AGAIN, "calc_p on another p": X_AGAIN, "calc_p with another r": X_AGAIN,
    "view of p": X_NEVER, "pointer of r": X_NEVER, "graph_begin": X_NEVER, "destroy p": X_NEVER,
    "close": ((2, 0, 0), (2, 2, 0)),
    # the extra calc_xr is the one that matches (level 1 launches behind it, level 2 commits its r); the second one
    # finds a calc_p in flight and drops it; the caller goes on with the second one's r.r, so iteration 5 arms
    "calc_xr again": ((6, 0, 1), (6, 7, 1)),
    # these leave the fused p.w valid, as a download does (dot(r, r) also re-reads r.r: the same bits)
    "dot(r, r)": ((8, 0, 0), (7, 7, 1)), "drain": ((8, 0, 0), (7, 7, 1)), "synchronize": ((8, 0, 0), (7, 7, 1)),
    # these void it (an SpMV of their own): iteration 4 does not match
    "residual_gap": X_AGAIN, "spmv of q": X_AGAIN,
    # leaves the fused p.w valid, and level 2 is armed again by iteration 4; iteration 5's SpMV reports the corrected bit
    # and the drain behind its dot(p, w) drops what level 2 launched behind that SpMV: 5 arms again, 6 .. 9 commit.
    # Level 1 launches behind calc_xr, after the drain: it never notices
    "inject": ((8, 0, 0), (6, 6, 2)),
}


@pytest.mark.parametrize("what", sorted(EXTRAS))
def test_between_calc_xr_and_calc_p(what, monkeypatch):
    """iteration 4's calc_p is in flight (both levels) when the extra call arrives: dropped, unread"""
    import abft_sparse_cg_amd as amd
    script = H.predicted(K)
    script[3] = {"before_p": EXTRAS[what]}
    res = H.levels(amd, monkeypatch, MODE_OF.get(what, "none"), H.matrix("lap40"), script)
    assert (res[1]["ahead"], res[2]["ahead"]) == BEFORE_P[what]


@pytest.mark.parametrize("what", sorted(EXTRAS))
def test_between_spmv_and_calc_xr(what, monkeypatch):
    """level 2: iteration 4's calc_r and calc_p are in flight behind the SpMV when the extra call arrives"""
    import abft_sparse_cg_amd as amd
    script = H.predicted(K)
    script[3] = {"before_xr": EXTRAS[what]}
    res = H.levels(amd, monkeypatch, MODE_OF.get(what, "none"), H.matrix("lap40"), script)
    assert (res[1]["ahead"], res[2]["ahead"]) == BEFORE_XR[what]


# ---- where it is armed ----
@pytest.mark.parametrize("mode", MODES)
def test_default_commits_in_mode_none_only(mode, monkeypatch):
    import abft_sparse_cg_amd as amd
    monkeypatch.delenv("ABFT_HIP_X_IN_SPMV", raising=False)
    res = H.levels(amd, monkeypatch, mode, H.matrix("lap40"), H.predicted(K))
    assert res[1]["ahead"] == ((K - 1, 0, 0) if mode == "none" else (0, 0, 0))
    assert res[2]["ahead"] == ((K - 1, K - 1, 0) if mode == "none" else (0, 0, 0))


@pytest.mark.parametrize("mode", MODES)
def test_every_mode_with_x_in_spmv_forced(mode, monkeypatch):
    res = play(monkeypatch, mode, "lap40", H.predicted(K))
    assert res[1]["ahead"] == (K - 1, 0, 0) and res[2]["ahead"] == (K - 1, K - 1, 0)


@pytest.mark.parametrize("env,value", [("ABFT_HIP_SPECULATE", "1"), ("ABFT_HIP_FUSE_X", "0"), ("ABFT_HIP_FUSE_DOT", "0"),
                                       ("ABFT_HIP_X_IN_SPMV", "0")])
def test_switches_that_keep_it_off(env, value, monkeypatch):
    import abft_sparse_cg_amd as amd
    monkeypatch.setenv(env, value)
    res = H.levels(amd, monkeypatch, "none", H.matrix("lap40"), H.predicted(K))
    assert res[1]["ahead"] == res[2]["ahead"] == (0, 0, 0)


def test_two_lengths_take_turns(monkeypatch):
    """two solves of different lengths in one context, four iterations each in turn: the first iteration after a switch
    is handed scalars of the other solve's history and never matches; the third and fourth commit"""
    import abft_sparse_cg_amd as amd
    from abft_sparse_cg_amd.context import fdiv
    out = {}
    for level in "012":
        monkeypatch.setenv("ABFT_HIP_AHEAD", level)
        events = []
        ctx = amd.HIPContext("none", "csr", on_event=lambda ev, fatal: events.extend((k, i, b, fatal) for k, i, b in ev))
        sets, scalars = [], []
        for name in ("lap40", "lap37x41"):
            cols, rows, vals, n = H.matrix(name)
            A = ctx.create_matrix(cols, rows, vals, n, len(vals))
            x, r, p, w = (ctx.create_vector(n) for _ in range(4))
            b = np.random.default_rng(3).random(n) + 0.5
            ctx.upload(x, np.zeros(n))
            ctx.upload(r, b)
            ctx.upload(p, b)
            ctx.upload(w, np.zeros(n))
            sets.append([A, (x, r, p, w), ctx.dot(r, r)])
        for turn in range(6):
            A, (x, r, p, w), rr = sets[turn % 2]
            for _ in range(4):
                ctx.spmv(A, p, w)
                pw = ctx.dot(p, w)
                rr_new = ctx.calc_xr(x, r, p, w, fdiv(rr, pw))
                ctx.calc_p(p, r, fdiv(rr_new, rr))
                scalars += [pw, rr_new]
                rr = rr_new
            sets[turn % 2][2] = rr
        got = [ctx.download(u) for _, v, _ in sets for u in v]
        ctx._drain()
        out[level] = (got, scalars, ctx.ahead_stats(), list(events))
        ctx.close()
    assert out["0"][2] == (0, 0, 0)
    # a switch finds nothing in flight (the last calc_p committed) and the other solve's spmv names other vectors: no drop
    assert out["1"][2] == (12, 0, 0) and out["2"][2] == (12, 12, 0)
    for level in "12":
        assert out[level][3] == out["0"][3]
        assert np.array_equal(H.bits(out[level][1]), H.bits(out["0"][1]))
        for a, b in zip(out[level][0], out["0"][0]):
            assert np.array_equal(H.bits(a), H.bits(b))


# ---- several solves in one context, against the numpy model ----
def turns(monkeypatch, names, schedule):
    import abft_sparse_cg_amd as amd
    mats = [H.matrix(name) for name in names]
    res = H.levels(amd, monkeypatch, "none", mats, schedule, run=H.run_turns)
    H.model_turns_hold("none", mats, schedule, res[0])
    return res


def test_three_lengths_take_turns(monkeypatch):
    """three solves of three lengths, four iterations each in turn, twice round: the x update's two buffers and the
    run-ahead's one shadow of r are freed and made again at every switch.  As with two lengths, a turn's first
    iteration never matches, its second arms, its third and fourth commit; the update left pending by a turn's last
    calc_p is applied on its own when the next solve's SpMV comes first"""
    res = turns(monkeypatch, ["lap40", "lap37x41", "rand"], [(k % 3, 16) for k in range(6)])
    assert res[1]["ahead"] == (12, 0, 0) and res[2]["ahead"] == (12, 12, 0)
    assert res[0]["xin"] == res[1]["xin"] == res[2]["xin"] == (12, 6)


@pytest.mark.parametrize("run", [1, 3])
def test_two_solves_of_one_length_take_turns(run, monkeypatch):
    """two solves on lap40 (they share one buffer for the new p), `run` iterations each in turn.  One each: every
    iteration is the first after a switch, nothing ever arms.  Three each: the second arms, the third commits"""
    res = turns(monkeypatch, ["lap40", "lap40"], [(k % 2, 4 * run) for k in range(8)])
    want = 8 * max(0, run - 2)
    assert res[1]["ahead"] == (want, 0, 0) and res[2]["ahead"] == (want, want, 0)
    assert res[0]["xin"] == res[1]["xin"] == res[2]["xin"] == (want, want)


def test_two_solves_alternate_inside_an_iteration(monkeypatch):
    """spmv and dot of one solve, spmv and dot of the other, then calc_xr and calc_p of each: the other solve's SpMV
    has replaced the fused p.w by the time calc_xr comes, and no SpMV directly follows the calc_p of its p"""
    res = turns(monkeypatch, ["lap40", "lap40"], [(0, 2), (1, 2)] * 12)
    for k in range(3):
        assert res[k]["ahead"] == (0, 0, 0) and res[k]["xin"] == (0, 0)


# ---- scalars at the ends of the exponent range ----
@pytest.mark.parametrize("exponent", [480, -480, -530])
@pytest.mark.parametrize("which", ["lap40", "lap3"])
def test_predicted_loop_on_scaled_right_hand_sides(which, exponent, monkeypatch):
    """r.r and p.w near 2^960 and 2^-960, and subnormal (2^-530 squared): the quotients formed on the device are the
    host's in every bit there too, so the counters are the arming rule's; lap3 converges on the way (see above)"""
    import abft_sparse_cg_amd as amd
    scale = 2.0 ** exponent
    script = H.predicted(K)
    res = H.levels(amd, monkeypatch, "none", H.matrix(which), script, scale=scale)
    H.model_holds("none", H.matrix(which), K, res[0], scale)
    for level in (1, 2):
        assert res[level]["ahead"] == expected(script, res[0]["scalars"], level), (level, res[level]["ahead"])
    if which == "lap40":
        assert res[1]["ahead"] == (K - 1, 0, 0) and res[2]["ahead"] == (K - 1, K - 1, 0)


# ---- an event at every SpMV ----
def test_standing_constraints_violation_drops_level_2_at_every_iteration(monkeypatch):
    """Mode constraints, the first column of lap40 lifted to its row successor's before the loop: every SpMV reports
    the order violation (nobody repairs it), so every dot(p, w) is followed by a drain, and a drain is an entry point
    like any other: it drops what level 2 launched behind that SpMV.  The drop disarms, the iteration itself matches
    and arms again: a drop per iteration from the second on, nothing ever committed.  Level 1 launches behind calc_xr,
    after the drain, and calc_xr reports no new event: it commits all but the first iteration.  (No numpy model here:
    the oracle, like the reference, stops at the fatal event.)"""
    import abft_sparse_cg_amd as amd
    script = H.predicted(K)
    script[0] = {"before_spmv": [("inject", 0, (64,))]}
    res = H.levels(amd, monkeypatch, "constraints", H.matrix("lap40"), script)
    assert len(res[0]["events"]) == K and {e[:2] for e in res[0]["events"]} == {(8, 0)}  # (8: column order, element 0)
    assert res[1]["ahead"] == (K - 1, 0, 0) and res[2]["ahead"] == (0, 0, K - 1)
