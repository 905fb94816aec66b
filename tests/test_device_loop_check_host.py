"""CPU-side checks of the residual checks in the device-resident loop (abft_hip_residual_check_dev,
abft_hip_residual_check_reserve, cg_solve_device(check_every=)): the header declares the two
entries and the built library exports them, the new keywords sit behind vector_ecc with cg_solve's defaults, the
batch schedule (_check_batch) never crosses a check position, and the control flow of cg_solve_device with checks --
what is enqueued before which download, what a failed slot makes the host do, when the one eager check runs --
against cg_solve(check_every=) on the numpy stand-in context of test_device_loop_precond_host.py, extended by the
device check.  With check_every=0 the calls are the ones made before the keywords existed.

As there, whatever loads the package runs in a child interpreter."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_device_loop_precond_host import STANDIN as BASE  # noqa: E402
from test_residual_check_host import child  # noqa: E402

NEW = ["abft_hip_residual_check_dev", "abft_hip_residual_check_reserve"]


def test_header_declares_the_device_check():
    from test_capi_symbols import declared_symbols
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s


def test_library_exports_the_device_check():
    out = child("""
import ctypes
from abft_sparse_cg_amd import capi
lib = ctypes.CDLL(capi.LIB_PATH)
missing = [s for s in %r if not hasattr(lib, s) or s not in capi.SIGNATURES]
assert not missing, missing
import abft_sparse_cg_amd as amd
for m in ("residual_check_dev", "residual_check_reserve"):
    assert callable(getattr(amd.HIPContext, m)), m
assert len(capi.SIGNATURES["abft_hip_residual_check_dev"][1]) == 9
assert capi.SIGNATURES["abft_hip_residual_check_dev"][1][-1] is ctypes.c_double
assert len(capi.SIGNATURES["abft_hip_residual_check_reserve"][1]) == 1
print("ok")
""" % (NEW,))
    assert out.strip() == "ok"


def test_new_keywords_follow_vector_ecc_with_cg_solves_defaults():
    out = child("""
import inspect
from abft_sparse_cg_amd.context import cg_solve, cg_solve_device
dev = inspect.signature(cg_solve_device).parameters
names = list(dev)
new = ["check_every", "check_tol", "max_rollbacks", "x_ckpt", "on_check"]
assert names[-6:] == ["vector_ecc"] + new, names
# everything in front of them as it was: positional calls are unchanged
assert names[:-5] == ["ctx", "A", "b", "x", "r", "p", "w", "max_itrs", "conv_threshold", "on_iteration", "stride",
                      "graph", "precond", "vector_ecc"], names
host = inspect.signature(cg_solve).parameters
for k in new:
    assert dev[k].default == host[k].default, k
assert [dev[k].default for k in new] == [0, 1e-7, 3, None, None]
print("ok")
""")
    assert out.strip() == "ok"


def test_the_schedule_never_crosses_a_check_position():
    out = child("""
from abft_sparse_cg_amd.context import _check_batch
for stride in (1, 3, 4, 16):
    for ce in (1, 4, 5, 16, 50):
        for max_itrs in (0, 1, 37, 100):
            done, batches = 0, []
            while done < max_itrs:
                m, check = _check_batch(done, max_itrs, stride, ce)
                assert 1 <= m <= stride, (stride, ce, max_itrs, done, m)
                # no check position strictly inside the batch
                assert not any((i + 1) % ce == 0 for i in range(done, done + m - 1)), (stride, ce, done, m)
                # a check follows exactly the iterations i with (i + 1) % ce == 0
                assert check == ((done + m) % ce == 0), (stride, ce, done, m, check)
                batches.append((m, check))
                done += m
            assert done == max_itrs == sum(m for m, _ in batches)
            checked = [sum(m for m, _ in batches[:k + 1]) - 1 for k, (_, c) in enumerate(batches) if c]
            assert checked == [i for i in range(max_itrs) if (i + 1) % ce == 0], (stride, ce, max_itrs)
            # at most two shapes recur: anything else is the run-up to max_itrs, once, at the end
            recurring = {(stride, False), ((ce - 1) % stride + 1, True)}
            odd = [k for k, s in enumerate(batches) if s not in recurring]
            assert odd in ([], [len(batches) - 1]), (stride, ce, max_itrs, batches)
            assert len(set(batches) & recurring) <= 2
# after a rollback at a count that is no multiple of check_every: on to the next multiple, then periodic again
assert _check_batch(13, 100, 4, 5) == (2, True) and _check_batch(15, 100, 4, 5) == (4, False)
assert _check_batch(13, 14, 4, 5) == (1, False)
print("ok")
""")
    assert out.strip() == "ok"


# the stand-in with the device check: the numpy operations of Single.residual_gap, the verdict by the host's rule and
# the copy it commands, all behind do() -- recorded under capture, run otherwise -- and a call list that shows every
# download and upload in its place
STANDIN = BASE + r'''
from abft_sparse_cg_amd.context import _check_batch

class CSingle(PSingle):
    def __init__(self, A):
        super().__init__(A)
        self.eager_checks, self.captures = 0, 0
    def cg_iteration_until_dev(self, A, vec, x, r, p, w, sc, rr_at, pw_at, new_at, thr):
        self.calls.append(("until", rr_at, pw_at, new_at))
        super().cg_iteration_until_dev(A, vec, x, r, p, w, sc, rr_at, pw_at, new_at, thr)
    def download(self, v):
        self.calls.append(("download", v.a.size))
        return super().download(v)
    def upload(self, v, a):
        self.calls.append(("upload", v.a.size))
        super().upload(v, a)
    def graph_begin(self):
        self.captures += 1
        super().graph_begin()
    def graph_launch(self, g):
        self.calls.append(("launch",))
        super().graph_launch(g)
    def residual_check_reserve(self):
        assert self.rec is None              # it allocates: never under capture
        self.calls.append(("reserve",))
    def sums(self, b, x, r, w):
        w.a[:] = self.A @ x.a
        t = b.a - w.a
        g = t - r.a
        return float(np.sum(g * g)), float(np.sum(t * t))
    def residual_check_dev(self, A, b, x, r, w, x_ckpt, trail, chk_at, limit):
        self.calls.append(("check", chk_at))
        if self.rec is None:
            self.eager_checks += 1
        def f():
            gap2, tt2 = self.sums(b, x, r, w)
            ok = (gap2 <= limit) and math.isfinite(gap2) and math.isfinite(tt2)
            trail.a[chk_at:chk_at + 4] = (gap2, tt2, 1.0 if ok else 2.0, 0.0)
            if ok:
                x_ckpt.a[:] = x.a
            else:
                x.a[:] = x_ckpt.a
        self.do(f)

def cdevice(A, b, max_itrs, conv, stride, graph=True, flips=(), check_flips=(), cls=CSingle, dinv=None, **kw):
    """-> (itr, rr, x, history, checks, ctx); flips: (iteration, name, index, bits) from on_iteration, check_flips:
    (iteration the check follows, name, index, bits) from on_check"""
    s = cls(A)
    n = len(b)
    vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
    vecs = {"x": vx, "r": vr, "p": vp}
    hist, checks = [], []
    def on_it(i, v):
        assert s.rec is None
        hist.append(v)
        for fi, name, idx, bits in flips:
            if fi == i:
                s.flip_vector(vecs[name], idx, bits)
    def on_ck(*c):
        checks.append(c)
        for fi, name, idx, bits in check_flips:
            if fi == c[0]:
                s.flip_vector(vecs[name], idx, bits)
    if dinv is not None:
        kw["precond"] = V(dinv.copy())
    it, rr = cg_solve_device(s, None, vb, vx, vr, vp, vw, max_itrs, conv, on_iteration=on_it, stride=stride,
                             graph=graph, on_check=on_ck, **kw)
    return it, rr, vx.a, hist, checks, s

def host(A, b, max_itrs, conv, flips=(), check_flips=(), cls=Single, dinv=None, **kw):
    s = cls(A)
    n = len(b)
    vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
    vecs = {"x": vx, "r": vr, "p": vp}
    hist, checks = [], []
    def on_it(i, v):
        hist.append(v)
        for fi, name, idx, bits in flips:
            if fi == i:
                s.flip_vector(vecs[name], idx, bits)
    def on_ck(*c):
        checks.append(c)
        for fi, name, idx, bits in check_flips:
            if fi == c[0]:
                s.flip_vector(vecs[name], idx, bits)
    if dinv is not None:
        kw["precond"] = V(dinv.copy())
    it, rr = cg_solve(s, None, vb, vx, vr, vp, vw, max_itrs, conv, on_iteration=on_it, on_check=on_ck, **kw)
    return it, rr, vx.a, hist, checks, s

def same(dev, ref):
    """count, rr, x, history and check records (gap included) bit for bit"""
    assert dev[0] == ref[0], (dev[0], ref[0])
    assert np.array_equal(bits([dev[1]]), bits([ref[1]]))
    assert np.array_equal(bits(dev[2]), bits(ref[2]))
    assert np.array_equal(bits(dev[3]), bits(ref[3]))
    assert len(dev[4]) == len(ref[4]), (dev[4], ref[4])
    for c, d in zip(dev[4], ref[4]):
        assert (c[0], c[2], c[3]) == (d[0], d[2], d[3]), (dev[4], ref[4])
        assert np.array_equal(bits([c[1]]), bits([d[1]])), (c, d)

def batches_of(calls):
    """the call list cut after every download -> per look, the calls in front of it"""
    out, cur = [], []
    for c in calls:
        cur.append(c)
        if c[0] == "download":
            out.append(cur)
            cur = []
    return out, cur
'''


def test_check_every_0_makes_the_calls_made_without_the_keywords():
    out = child(STANDIN + r'''
for graph in (True, False):
    for stride in (1, 3, 16):
        for dinv in (None, pdinv):
            M, rhs_ = (A, b) if dinv is None else (PA, pb)
            runs = []
            for kw in ({}, {"check_every": 0}, {"check_every": 0, "check_tol": 1e-3, "max_rollbacks": 0}):
                it, rr, x, h, checks, s = cdevice(M, rhs_, 23, 1e-20, stride, graph, dinv=dinv, **kw)
                assert checks == [] and s.eager_checks == 0
                assert not any(c[0] in ("check", "reserve", "restart") for c in s.calls)
                assert [c[0] for c in s.calls].count("upload") == 1          # the trail's seed, nothing reseeded
                runs.append((it, rr, x.tobytes(), tuple(h), s.calls, s.downloads, s.launches, s.eager))
            assert runs[0] == runs[1] == runs[2], (graph, stride)
# written out: two copies and a dot, the trail's upload, then per batch one copy, m guarded iterations over pairs at
# 2 k with p.w at 2 (stride + 1), and the download
it, rr, x, h, checks, s = cdevice(A, b, 7, 1e-20, 3, False, check_every=0)
want = [("copy",), ("copy",), ("dot",), ("upload", 10)]
for m in (3, 3, 1):
    want += [("copy",)] + [("until", 2 * k, 8, 2 * k + 2) for k in range(m)] + [("download", 10)]
want += [("destroy",)] * 3
assert it == 7 and s.calls == want, s.calls
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_clean_runs_are_cg_solve_with_checks_call_by_call():
    out = child(STANDIN + r'''
plain = cdevice(A, b, 1000, 1e-20, 4)
need = plain[0]
assert 23 < need < 1000
for stride in (1, 3, 4, 16):
    for ce in (1, 4, 5, 16, 50):
        for graph in (True, False):
            for max_itrs in (1000, 37, need):
                ref = host(A, b, max_itrs, 1e-20, check_every=ce)
                dev = cdevice(A, b, max_itrs, 1e-20, stride, graph, check_every=ce)
                same(dev, ref)
                assert dev[4] and all(c[2] for c in dev[4])
                s = dev[5]
                # the rr history and x are those of the loop without checks
                if max_itrs == 1000:
                    assert np.array_equal(bits(dev[2]), bits(plain[2])) and dev[3] == plain[3]
                looks, rest = batches_of(s.calls)
                # every check is enqueued in front of the download that brings its slot, behind the iterations
                for look in looks:
                    # (a captured batch shows its calls once, in front of its first launch; a replay only the launch)
                    kinds = [c[0] for c in look if c[0] not in ("launch", "reserve")]
                    assert kinds.count("check") <= 1 and kinds[-1] == "download"
                    if "check" in kinds:
                        assert kinds.index("check") == len(kinds) - 2, kinds
                assert not any(c[0] in ("check", "until", "launch") for c in rest)
                # the eager final check only when the last batch carried none: then one look at the four words alone
                it = dev[0]
                lone = [look for look in looks if look[-1] == ("download", 4)]
                assert all([c[0] for c in look] == ["check", "download"] for look in lone)
                assert s.eager_checks >= len(lone)
                assert len(lone) <= 1
                if it % ce == 0:
                    assert lone == [], (stride, ce, max_itrs)
                # graphs: at most the two recurring shapes, each captured once behind the reserve call
                assert s.captures <= (2 if graph else 0)
                assert s.calls.count(("reserve",)) == s.captures
                if not graph:
                    assert s.launches == 0
                assert not any(c[0] in ("restart", "gap", "spmv", "calc_xr") for c in s.calls)
# written out for stride 4, check_every 5, 12 iterations allowed, eager: the trail has 2 * 5 + 2 + 4 doubles; a
# batch of m iterations uses the pairs 4 - m .. 4; the check's slot starts at 12
it, rr, x, h, checks, s = cdevice(A, b, 12, 1e-20, 4, False, check_every=5)
want = [("copy",), ("copy",), ("dot",), ("copy",), ("upload", 16)]
full = [("copy",)] + [("until", 2 * k, 10, 2 * k + 2) for k in range(4)] + [("download", 16)]
one = [("copy",), ("until", 6, 10, 8), ("check", 12), ("download", 16)]
two = [("copy",), ("until", 4, 10, 6), ("until", 6, 10, 8), ("download", 16)]
want += full + one + full + one + two + [("check", 12), ("download", 4)]
assert it == 12 and [c for c in s.calls if c[0] != "destroy"] == want, s.calls
assert [(c[0], c[2], c[3]) for c in checks] == [(4, True, None), (9, True, None), (11, True, None)]
assert s.calls.count(("destroy",)) == 7      # three first-record views, last, the slot, the trail, the checkpoint
# 10 allowed: the last batch carries the check, nothing eager
it, rr, x, h, checks, s = cdevice(A, b, 10, 1e-20, 4, True, check_every=5)
assert it == 10 and s.eager_checks == 0 and s.captures == 2 and s.downloads == 4 and s.launches == 4
assert [c[0] for c in checks] == [4, 9]
# a caller's checkpoint vector is used and kept
ck = V(np.zeros(n))
s0 = cdevice(A, b, 10, 1e-20, 4, True, check_every=5, x_ckpt=ck)
assert np.array_equal(bits(ck.a), bits(s0[2])) and s0[5].calls.count(("destroy",)) == 5
# nothing to iterate: the start is checked, as cg_solve does it
for max_itrs, conv, rhs_ in ((0, 1e-20, b), (1000, 1e9, b), (1000, 1e-3, np.zeros(n))):
    ref = host(A, rhs_, max_itrs, conv, check_every=5)
    dev = cdevice(A, rhs_, max_itrs, conv, 4, True, check_every=5)
    same(dev, ref)
    assert [c[0] for c in dev[4]] == [-1] and dev[5].eager_checks == 1 and dev[5].live == 0
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_a_failed_slot_restarts_reseeds_and_goes_on_as_cg_solve():
    out = child(STANDIN + r'''
def ends_plain_batch(itr, stride, ce):
    """is iteration itr the last of a batch that carries no check (the schedule function names them)?"""
    done = 0
    while done <= itr:
        m, check = _check_batch(done, 10 ** 6, stride, ce)
        done += m
        if done == itr + 1:
            return not check
    return False

assert ends_plain_batch(13, 4, 5) and ends_plain_batch(13, 1, 5)
assert not ends_plain_batch(13, 3, 5) and not ends_plain_batch(14, 4, 5)
clean = host(A, b, 1000, 1e-20)
i = int(np.argmax(np.abs(clean[2])))
for stride, graph in ((4, True), (4, False), (3, True), (16, False), (1, True)):
    for bit in (62, 55, 52, 45):
        for name in ("x", "r"):
            # from on_iteration at iteration 13 -- with stride 4 the last of a batch without a check -- and from
            # on_check behind the check-carrying batch
            for kw in ({"flips": [(13, name, i, [bit])]}, {"check_flips": [(9, name, i, [bit])]}):
                if "flips" in kw and not ends_plain_batch(13, stride, 5):
                    continue                  # on_iteration(13) would run behind later iterations of its batch
                ref = host(A, b, 1000, 1e-20, check_every=5, **kw)
                dev = cdevice(A, b, 1000, 1e-20, stride, graph, check_every=5, **kw)
                same(dev, ref)
                fails = [c for c in dev[4] if not c[2]]
                assert len(fails) == 1 and fails[0][3] == 9, (stride, bit, name, dev[4])
                assert true_res(A, b, dev[2]) <= 10 * true_res(A, b, clean[2])
                s = dev[5]
                k = s.calls.index(("restart",))
                # the failed slot came with a download; then restart, and the reseeding of record `stride`
                assert s.calls[k - 1][0] == "download" and s.calls[k + 1] == ("upload", 2), s.calls[k - 2:k + 3]
                assert s.calls.count(("restart",)) == 1
assert _check_batch(10, 1000, 4, 5) == (4, False)     # iterations 10 .. 13: 13 is the last of a batch without a check
# with precond: precond_start on the restarted r, the record of four doubles reseeded
for stride, graph, kw in ((4, True, {"flips": [(13, "x", 5, [55])]}), (16, False, {"check_flips": [(9, "x", 5, [55])]})):
    ref = host(PA, pb, 1000, 1e-20, cls=PSingle, dinv=pdinv, check_every=5, **kw)
    dev = cdevice(PA, pb, 1000, 1e-20, stride, graph, dinv=pdinv, check_every=5, **kw)
    same(dev, ref)
    assert [(c[0], c[3]) for c in dev[4] if not c[2]] == [(14, 9)]
    s = dev[5]
    k = s.calls.index(("restart",))
    assert s.calls[k - 1][0] == "download" and s.calls[k + 1:k + 3] == [("precond_start",), ("upload", 4)]
    clean_p = cdevice(PA, pb, 1000, 1e-20, stride, graph, dinv=pdinv)
    with_checks = cdevice(PA, pb, 1000, 1e-20, stride, graph, dinv=pdinv, check_every=5)
    assert np.array_equal(bits(clean_p[2]), bits(with_checks[2])) and clean_p[3] == with_checks[3]
# an r flip that drives r.r to a non-number: the loop freezes, the check on that final state fails, the solve restarts
# -- on its own (eager) when the batch that froze carried no check, else the check behind that batch
for stride, graph, ce, at, eager in ((1, True, 5, 7, 1), (4, True, 16, 3, 1), (4, False, 16, 3, 1), (4, True, 7, 3, 0)):
    assert ends_plain_batch(at, stride, ce)
    hs = Single(A)
    vb, vx, vr_, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
    cg_solve(hs, None, vb, vx, vr_, vp, vw, at + 1, 0.0)   # the state after iteration `at`
    j = int(np.argmax(np.abs(vr_.a)))
    ex = int(vr_.a[j:j + 1].view(np.uint64)[0] >> np.uint64(52)) & 0x7FF
    allones = [52 + t for t in range(11) if not (ex >> t) & 1]   # exponent all ones: inf or NaN
    ref = host(A, b, 1000, 1e-20, check_every=ce, flips=[(at, "r", j, allones)])
    fails = [(c[0], c[3]) for c in ref[4] if not c[2]]
    assert len(fails) == 1 and (fails[0][0] + 1) % ce != 0, ref[4]      # a check of the final state, not a periodic one
    dev = cdevice(A, b, 1000, 1e-20, stride, graph, check_every=ce, flips=[(at, "r", j, allones)])
    same(dev, ref)
    assert dev[5].eager_checks >= eager and (dev[5].frozen > 0 or stride == 1)
    lone = [look for look in batches_of(dev[5].calls)[0] if look[-1] == ("download", 4)]
    assert len(lone) >= eager and (eager or len(lone) <= 1)
    assert np.all(np.isfinite(dev[2])) and true_res(A, b, dev[2]) <= 10 * true_res(A, b, clean[2])
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_failures_that_repeat_raise_as_cg_solve_does():
    out = child(STANDIN + r'''
class Broken(Single):
    def residual_gap(self, *a):
        g2, t2 = Single.residual_gap(self, *a)
        return float("nan"), t2
class DBroken(CSingle):
    def sums(self, *a):
        g2, t2 = CSingle.sums(self, *a)
        return float("nan"), t2              # NaN must fail the rule on the device too
for m in (0, 1, 3):
    for stride, graph in ((4, True), (3, False), (16, True)):
        got = []
        for run, cls in ((host, Broken), (lambda *a, **k: cdevice(*a, stride, graph, **k), DBroken)):
            try:
                run(A, b, 1000, 1e-20, cls=cls, check_every=4, max_rollbacks=m)
            except ResidualCheckFailed as e:
                got.append((str(e), [(c[0], c[2], c[3]) for c in e.checks]))
            else:
                raise AssertionError(m)
        assert got[0] == got[1], got
        assert len(got[1][1]) == m + 1 and [c[0] for c in got[1][1]] == [4 * t + 3 for t in range(m + 1)]
        assert "after %d rollbacks" % m in got[1][0]
# a failure at max_itrs: rolled back and raised, x the last checkpoint that passed
it0 = host(A, b, 1000, 1e-20)[0]
ce = next(c for c in range(5, 12) if it0 % c >= 4)
last = (it0 // ce) * ce - 1
for stride, graph in ((1, True), (1, False), (4, True), (16, False)):
    msgs = []
    for run in (host, lambda *a, **k: cdevice(*a, stride, graph, **k)):
        try:
            run(A, b, it0, 1e-20, check_every=ce, flips=[(last + 2, "x", 3, [55])])
        except ResidualCheckFailed as e:
            assert [(c[0], c[2], c[3]) for c in e.checks][-1] == (it0 - 1, False, last), e.checks
            msgs.append(str(e))
        else:
            raise AssertionError("no ResidualCheckFailed at max_itrs")
    assert all("max_itrs" in m for m in msgs)
    if stride == 1:                           # every callback in cg_solve's place: the same gap, the same text
        assert msgs[0] == msgs[1], msgs
# x then holds the checkpoint
ck = V(np.zeros(n))
s = DBroken(A)
vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
vx.a[:] = 0.25
try:
    cg_solve_device(s, None, vb, vx, vr, vp, vw, 1000, 1e-20, stride=4, check_every=4, max_rollbacks=1, x_ckpt=ck)
except ResidualCheckFailed:
    assert np.all(vx.a == 0.25) and np.all(ck.a == 0.25)
else:
    raise AssertionError
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_refusals_come_before_anything_runs():
    out = child(STANDIN + r'''
def refused(**kw):
    s = CSingle(A)
    vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
    try:
        cg_solve_device(s, None, vb, vx, vr, vp, vw, 10, 1e-3, **kw)
    except ValueError as e:
        assert s.calls == [], s.calls
        return str(e)
    raise AssertionError(kw)
assert "vector_ecc with check_every" in refused(vector_ecc=True, check_every=5)
for kw in ({"check_every": -1}, {"check_every": 2.5}, {"check_every": 5, "check_tol": 0.0},
           {"check_every": 5, "check_tol": float("inf")}, {"check_every": 5, "check_tol": float("nan")},
           {"check_every": 5, "max_rollbacks": -1}, {"check_tol": -1.0}):
    refused(**kw)
print("ok")
''')
    assert out.strip().endswith("ok"), out
