"""The protected block trail (TrailBlock<K> in abft_sparse_cg_amd/csrc/trail_ecc.h) without a GPU:
tests/host/trail_block_play.cpp compiles the header -- the text the kernels compile -- for the host, with
AddressSanitizer and UBSan, as a program of its own, and plays an iteration through TrailBlock's own rules.

  * TrailBlock<K> against the model of guard_protocol.h: test_guard_protocol_host.py's block cases for K = 1, 3, 8,
    plain and preconditioned, every mask and threshold, each with a flipped bit in one or more of the slots a launch
    reads -- every bit 0..127 of an r.r slot, an r.z slot, a live P.W slot and a live next-r.z slot, alone and
    together with flips in other slots; the mask, the alphas and betas, the all-frozen hand-on (NaN payloads and -0.0
    kept), the partial publication and the repair count;
  * what is read and what is not: two flips in a slot read stop the half that reads it, two flips in a frozen
    column's P.W slot (or next r.z, or the events word) stop nothing;
  * planted mistakes, each caught;
  * the library's surface, and cg_solve_block_device(trail_ecc=True) on a stand-in context (that of
    test_device_loop_block_host.py, extended by the protected iteration on slots)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_guard_protocol_host as G  # noqa: E402
from test_device_loop_block_host import STANDIN as BASE, child  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "abft_sparse_cg_amd", "csrc")
HEADERS = ["trail_ecc.h", "struct_ecc.h", "ecc_device.h", "guard_protocol.h"]
NEW = ["abft_hip_cg_block_trail_iteration_until_dev", "abft_hip_cg_block_vecc_trail_iteration_until_dev",
       "abft_hip_block_trail_inject_at"]
START, PW, NEXT = 0, 1, 2
KINDS = ("rr", "rz", "pw", "next")


def build(include_dir, out_dir):
    exe = os.path.join(str(out_dir), "trail_block_play")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-Wno-unknown-pragmas", "-I", str(include_dir), os.path.join(HERE, "host", "trail_block_play.cpp"), "-o", exe],
                   check=True)
    return exe


def run(exe, tmp, text):
    path = os.path.join(str(tmp), "requests.txt")
    with open(path, "w") as f:
        f.write(text)
    # (the leak check at exit needs ptrace rights a sandbox may withhold; the program frees through destructors)
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    return p.returncode, p.stdout.splitlines(), p.stderr


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(CSRC, tmp_path_factory.mktemp("trail_block"))


# ---- the requests: a block case of test_guard_protocol_host.py with a list of damages ----

def live_columns(k, case):
    return [j for j in range(k) if (G.expect_block(k, 0, case)[0] >> j) & 1]


def slot_of(kind, k, j):
    return {"rr": (START, j), "rz": (START, k + j), "pw": (PW, j), "next": (NEXT, k + j)}[kind]


def with_flips(blocks):
    """-> [(k, precond, case, flips, kinds)]: every case twice.  First with ONE flipped bit in one slot -- the kind of
    slot goes round, and each kind counts its own bits up, so every bit of every kind is reached alone; then with a
    flipped bit in one slot of every kind at once (P.W and next r.z: of a live column, when there is one)."""
    out = []
    count = {kind: 0 for kind in KINDS}
    turn = 0
    for k, precond, cases in blocks:
        for case in cases:
            live = live_columns(k, case)
            kind = KINDS[turn % 4]
            turn += 1
            if kind in ("pw", "next") and not live:
                kind = KINDS[turn % 2]
            c = count[kind]
            count[kind] += 1
            j = live[c % len(live)] if kind in ("pw", "next") else c % k
            out.append((k, precond, case, [slot_of(kind, k, j) + (c % 128,)], (kind,)))
    start = {"rr": 0, "rz": 37, "pw": 71, "next": 101}
    count = dict(start)
    for k, precond, cases in blocks:
        for case in cases:
            live = live_columns(k, case)
            flips, kinds = [], []
            for kind in KINDS:
                if kind in ("pw", "next") and not live:
                    continue
                c = count[kind]
                count[kind] += 1
                j = live[(c // 3) % len(live)] if kind in ("pw", "next") else (c // 5) % k
                flips.append(slot_of(kind, k, j) + (c % 128,))
                kinds.append(kind)
            out.append((k, precond, case, flips, tuple(kinds)))
    return out


def line_of(k, precond, case, flips):
    t, nev, _, rec_in, pw, rec_out, tot = case
    words = " ".join("%x" % w for w in rec_in + pw + rec_out + tot)
    damage = "".join(" %d %d %d" % f for f in flips)
    return "tblock %d %d %x %x %s %d%s" % (k, precond, t, nev, words, len(flips), damage)


def expect(k, precond, case):
    """G.expect_block's words -- the mask, alpha[k], beta[k], the hand-on, the publication -- as a protected launch
    gives them: a frozen column's alpha and beta are +0.0, its P.W slot is not read"""
    want = G.expect_block(k, precond, case)
    mask = want[0]
    for j in range(k):
        if not (mask >> j) & 1:
            want[1 + j] = want[1 + k + j] = 0
    return want


def mismatches(exe, tmp, requests):
    rc, lines, err = run(exe, tmp, "\n".join(line_of(k, p, c, f) for k, p, c, f, _ in requests) + "\n")
    if rc != 0:
        return [("program", rc, err[-500:])]
    assert len(lines) == len(requests)
    bad = []
    for i, ((k, precond, case, flips, _), line) in enumerate(zip(requests, lines)):
        w = line.split()
        if w[0] != "b":
            bad.append(("fatal", (k, precond), i))
            continue
        got = [int(w[1])] + [int(t, 16) for t in w[2:-1]]
        if got != expect(k, precond, case):
            bad.append(("block", (k, precond), i))
        if int(w[-1]) != len(flips):
            bad.append(("repairs", (k, precond), i))
    return bad


@pytest.fixture(scope="module")
def blocks():
    return [(k, precond, G.block_cases(k, precond)) for k in (1, 3, 8) for precond in (0, 1)]


def test_protected_block_records_give_guard_protocols_bits(exe, blocks, tmp_path):
    requests = with_flips(blocks)
    assert len(requests) == 2 * sum(len(c) for _, _, c in blocks) == 2 * 3360
    bad = mismatches(exe, tmp_path, requests)
    assert not bad, (len(bad), bad[:10])
    # what the requests reach: every bit of every kind of slot, alone and together with flips in other slots
    alone = {kind: set() for kind in KINDS}
    together = {kind: set() for kind in KINDS}
    for k, _, _, flips, kinds in requests:
        for (_, _, bit), kind in zip(flips, kinds):
            (alone if len(flips) == 1 else together)[kind].add(bit)
    for kind in KINDS:
        assert alone[kind] == set(range(128)) and together[kind] == set(range(128)), kind
    assert any(len(f) == 4 for _, _, _, f, _ in requests)
    # ... on both verdicts, partial masks, and frozen words that a double's arithmetic would change
    masks = {(k, G.expect_block(k, 0, c)[0]) for k, _, c, _, _ in requests}
    assert {(3, m) for m in range(8)} <= masks and (8, 0xFF) in masks and (8, 0) in masks and (8, 0xFE) in masks
    frozen = set()
    for k, _, c, _, _ in requests:
        m = G.expect_block(k, 0, c)[0]
        frozen |= {c[3][j] for j in range(k) if not (m >> j) & 1} | {c[3][k + j] for j in range(k) if not (m >> j) & 1}
    assert {G.QNAN, G.NEG_NAN, G.SNAN, int(G.b64(-0.0))} <= frozen


def special_requests(precond):
    """K = 3, columns 0 and 2 live, column 1 frozen: [(case, flips, the line expected: None the clean one)]"""
    thr = int(G.b64(1e-3))
    case = next(c for c in G.block_cases(3, precond) if c[0] == thr and G.expect_block(3, precond, c)[0] == 0b101)
    k = 3
    return case, [
        ([(PW, 1, 3), (PW, 1, 77)], None),                 # two flips in the frozen column's P.W: not read
        ([(PW, 1, 50)], None),                             # one: not read, not repaired, not counted
        ([(NEXT, k + 1, 9), (NEXT, k + 1, 100)], None),    # the frozen column's next r.z: not read
        ([(START, 2 * k, 1), (START, 2 * k, 2)], None),    # the events word: the host's decode covers it
        ([(START, 2 * k + 1, 64), (START, 2 * k + 1, 65)], None),
        ([(PW, k, 0), (PW, k, 127)], None),                # the tail's events word
        ([(START, 1, 5), (START, 1, 90)], "f 0 1 0"),      # r.r of the frozen column: read by every launch
        ([(START, k, 24), (START, k, 25)], "f 0 1 0"),     # r.z of a live column
        ([(START, 0, 70), (START, k + 1, 24), (START, k + 1, 31)], "f 0 1 1"),  # a repair on the way is kept
        ([(PW, 2, 33), (PW, 2, 34)], "f 1 1 0"),           # P.W of a live column: the r half stops
        ([(PW, 0, 12), (NEXT, k + 0, 66), (NEXT, k + 0, 67)], "f 2 1 1"),  # next r.z of a live column: the x / p half
        ([(START, 1, 1000)], "f 0 1 0"),                   # r.r[0]'s codeword in r.r[1]'s place
        ([(NEXT, k + 2, 1000 + k)], "f 2 1 0"),            # r.z[0]'s codeword of the next record in r.z[2]'s place
        ([(PW, 0, 1002)], "f 1 1 0"),
    ]


def special_bad(exe, tmp, precond):
    case, specials = special_requests(precond)
    rc, lines, err = run(exe, tmp, "\n".join(line_of(3, precond, case, f) for f, _ in specials) + "\n")
    if rc != 0:
        return [("program", rc, err[-500:])]
    clean = expect(3, precond, case)
    bad = []
    for i, ((flips, want), line) in enumerate(zip(specials, lines)):
        w = line.split()
        if want is None:
            ok = w[0] == "b" and [int(w[1])] + [int(t, 16) for t in w[2:-1]] == clean and w[-1] == "0"
        else:
            ok = line == want
        if not ok:
            bad.append((i, flips, line[:40]))
    return bad


@pytest.mark.parametrize("precond", [0, 1])
def test_what_a_launch_reads_and_what_it_does_not(exe, tmp_path, precond):
    assert not special_bad(exe, tmp_path, precond)


MISTAKES = {
    "a frozen column is handed on through + 0.0":
        ("trail_ecc.h", "const uint64_t word = guard_word(plain_out, i);",
         "const uint64_t word = (uint64_t)__double_as_longlong(plain_out[i] + 0.0);"),
    "r.z is published from r.r under PRECOND":
        ("guard_protocol.h", "const uint64_t rz_new = PRECOND ? (uint64_t)__double_as_longlong(tot[2 * j]) : rr_new;",
         "const uint64_t rz_new = rr_new;"),
    "the ordinal of RZ + j is encoded as j":
        ("trail_ecc.h", "      trail_put(out, i, word);\n",
         "      { uint32_t w[4]; trail_encode(word, (uint32_t)(i >= RZ && i < EV ? i - RZ : i), w); trail_store(out, i, w); }\n"),
    "a frozen column's P.W double flip is fatal":
        ("trail_ecc.h", "      if (ok && ((active >> j) & 1u)) {\n        const auto pw = get(ABFT_TRAIL_PW, j);",
         "      if (ok) {\n        const auto pw = get(ABFT_TRAIL_PW, j);"),
    "the mask is taken from r.z":
        ("trail_ecc.h", "    return G::live_mask(rec, threshold);", "    return G::live_mask(rec + RZ, threshold);"),
    "beta divides by the next record's word":
        ("trail_ecc.h", "    for (int i = 0; i < LEN; i++) guard_put(out, i, next_rz);\n    return G::beta(in, out, j);",
         "    for (int i = 0; i < LEN; i++) guard_put(out, i, next_rz);\n    return G::beta(out, in, j);"),
    "the raw hand-on leaves the last word out":
        ("trail_ecc.h", "    for (int i = 0; i < DOUBLES; i++) guard_put(out, i, guard_word(in, i));",
         "    for (int i = 0; i + 1 < DOUBLES; i++) guard_put(out, i, guard_word(in, i));"),
}


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_a_planted_mistake_is_caught(blocks, tmp_path, mistake):
    """the comparisons can fail: a private copy of the headers with one mistake planted"""
    where, old, new = MISTAKES[mistake]
    inc = tmp_path / "inc"
    inc.mkdir()
    for h in HEADERS:
        with open(os.path.join(CSRC, h)) as f:
            text = f.read()
        if h == where:
            assert text.count(old) == 1, (h, text.count(old))
            text = text.replace(old, new)
        (inc / h).write_text(text)
    bad_exe = build(inc, tmp_path)
    some = [(k, p, c) for k, p, c in blocks if k == 3]
    bad = mismatches(bad_exe, tmp_path, with_flips(some)) + special_bad(bad_exe, tmp_path, 0) + special_bad(bad_exe, tmp_path, 1)
    assert bad, mistake


# ---- the header and the library's surface ----

def test_header_keeps_its_includes_and_covers_the_block_record():
    with open(os.path.join(CSRC, "trail_ecc.h")) as f:
        text = f.read()
    assert re.findall(r"#include\s*[\"<]([^\">]+)", text) == ["stdint.h", "guard_protocol.h", "struct_ecc.h"]
    assert not re.search(r"\bhip[A-Z]\w*\(|threadIdx|blockIdx|__global__|__shared__", text)
    assert "template <int K> struct TrailBlock" in text and "out of scope" not in text


def test_header_capi_library_and_methods_agree():
    from test_capi_symbols import declared_symbols
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s
    out = child("""
import ctypes, inspect
from abft_sparse_cg_amd import capi
lib = ctypes.CDLL(capi.LIB_PATH)
missing = [s for s in %r if not hasattr(lib, s) or s not in capi.SIGNATURES]
assert not missing, missing
import abft_sparse_cg_amd as amd
for m in ("cg_block_trail_iteration_until_dev", "cg_block_vecc_trail_iteration_until_dev", "block_trail_inject_at"):
    assert callable(getattr(amd.HIPContext, m)), m
f = amd.cg_solve_block_device
assert f.__kwdefaults__ == {"trail_ecc": False, "on_batch": None}
assert list(inspect.signature(f).parameters)[-2:] == ["precond", "vector_ecc"]
assert "trail_ecc=False, on_batch=None" in f.__doc__
try:
    f(*([None] * 14), True)
except TypeError:
    pass
else:
    raise AssertionError("a fifteenth positional argument was taken")
print("ok")
""" % (NEW,))
    assert out.strip() == "ok"


# ---- cg_solve_block_device(trail_ecc=True) on the stand-in ----
# The protected iteration of the stand-in keeps its scalars as slots through the library's own host functions
# (abft_hip_trail_encode / abft_hip_trail_decode need no GPU) and computes what DRec.cg_block_iteration_until_dev does.
STANDIN = BASE + r'''
from abft_sparse_cg_amd import capi

L = capi.load()

def enc(values, first=0):
    v = np.ascontiguousarray(values, dtype=np.float64)
    out = np.zeros(2 * len(v))
    capi.check(L.abft_hip_trail_encode(v.ctypes.data_as(capi.f64p), len(v), first, out.ctypes.data_as(capi.f64p)))
    return out

def dec(slots):
    s = np.ascontiguousarray(slots, dtype=np.float64)
    n = len(s) // 2
    v, st, b = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
    capi.check(L.abft_hip_trail_decode(s.ctypes.data_as(capi.f64p), n, v.ctypes.data_as(capi.f64p),
                                       st.ctypes.data_as(capi.i32p), b.ctypes.data_as(capi.i32p)))
    return v, st, b

class TRec(DRec):
    def __init__(self, A):
        super().__init__(A)
        self.reported, self.trail_calls, self.repaired = [], 0, []
    def encode_trail(self, values, first_ordinal=0):
        self.calls.append(("encode_trail", len(values)))
        return enc(values, first_ordinal)
    def report_trail(self, slots, rec, stride):
        v, st, b = dec(slots)
        assert len(v) == rec * (stride + 1) + (rec - 2) // 2 + 1      # the records and the tail of k + 1 words
        self.reported += [(int(j), int(st[j]), int(b[j])) for j in np.flatnonzero(st)]
        return v
    def flip_trail(self, trail, slot, bits):
        w = trail.a.view(np.uint32)
        for bit in bits:
            w[4 * slot + (bit >> 5)] ^= np.uint32(1 << (bit & 31))
    def cg_block_trail_iteration_until_dev(self, A, X, R, P, W, k, sc, in_at, pw_at, out_at, thr, dinv=None):
        # the same name in the call list: the lists of a protected and an unprotected solve are compared
        self.calls.append(("block_until", in_at // 2, pw_at // 2, out_at // 2, dinv is not None))
        assert in_at % 2 == 0 and pw_at % 2 == 0 and out_at % 2 == 0
        self.trail_calls += 1
        if self.rec is None:
            self.eager += 1
        else:
            assert self.reserved
        def f():
            rec = 2 * k + 2
            vals, st, b = dec(sc.a[in_at:in_at + 4 * k])          # the 2k value slots: all read by every launch
            assert (st >= 0).all()
            for o in np.flatnonzero(st):                          # repaired in place
                sc.a[in_at + 2 * o:in_at + 2 * o + 2] = enc(vals[o:o + 1], int(o))
                self.repaired.append((int(o), int(b[o])))
            u = vals.view(np.uint64)
            active = sum(1 << j for j in range(k) if vals[j] > thr)
            self._mm(P, W, k)
            pw = sums(P, W, k)
            sc.a[pw_at:pw_at + 2 * (k + 1)] = enc(np.concatenate([pw, [0.0]]), 0)
            if not active:
                sc.a[out_at:out_at + 2 * rec] = enc(np.concatenate([vals, [0.0, 0.0]]), 0)
                self.frozen += 1
                return
            self.live += 1
            on = [(active >> j) & 1 for j in range(k)]
            num = vals[k:2 * k].copy()
            alpha = [fdiv(num[j], pw[j]) if on[j] else 0.0 for j in range(k)]
            got = self._r(R, W, k, alpha, active, dinv)
            rz_new, rr_new = (got, got) if dinv is None else got
            beta = [fdiv(rz_new[j], num[j]) if on[j] else 0.0 for j in range(k)]
            self._x(X, P, k, alpha, active); self._p(P, R, k, beta, active, dinv)
            new = np.concatenate([rr_new, rz_new]).view(np.uint64)
            keep = np.array(on + on, dtype=bool)
            words = np.where(keep, new, u).view(np.float64)       # frozen words: moved as integers
            sc.a[out_at:out_at + 2 * rec] = enc(np.concatenate([words, [0.0, 0.0]]), 0)
        self.do(f)

def tdevice(A, B, pre, max_itrs, conv, stride, graph=True, on_batch=None, cls=None):
    s = (cls or TRec)(A)
    v = vecs(B)
    s.x = v[1]
    hist = []
    def cb(i, r, a):
        assert s.rec is None
        hist.append((i, r, a, s.downloads))
    itrs, rr = cg_solve_block_device(s, None, *v, max_itrs, conv, on_iteration=cb, stride=stride, graph=graph,
                                     precond=dinv_of(A, pre), trail_ecc=True, on_batch=on_batch)
    return list(itrs), rr, v[1].a, hist, s

def same_history(h, h0):
    return ([(i, a, d) for i, _, a, d in h] == [(i, a, d) for i, _, a, d in h0]
            and all(np.array_equal(bits(r), bits(r0)) for (_, r, _, _), (_, r0, _, _) in zip(h, h0)))
'''


def test_protected_block_loop_is_the_block_device_loop_on_the_standin():
    out = child(STANDIN + r'''
for pre in (False, True):
    for max_itrs, conv in ((1000, 1e-20), (23, 1e-20), (1000, 1e-3), (0, 1e-20)):
        for stride in (1, 5, 16):
            for graph in (True, False):
                it0, rr0, x0, h0, s0 = device(PA, PB, pre, max_itrs, conv, stride, graph)
                it, rr, x, h, s = tdevice(PA, PB, pre, max_itrs, conv, stride, graph)
                assert it == it0 and np.array_equal(bits(rr), bits(rr0)) and np.array_equal(bits(x), bits(x0)), stride
                assert same_history(h, h0), stride
                # the same batches, downloads, launches and eager calls; the guarded calls are the protected ones
                assert (s.downloads, s.launches, s.eager, s.live, s.frozen, s.reserved) == \
                       (s0.downloads, s0.launches, s0.eager, s0.live, s0.frozen, s0.reserved)
                assert not s.reported and not s.repaired
                # the same call list, offsets doubled, but for the three encodes of the trail's start
                assert [c for c in s.calls if c[0] != "encode_trail"] == s0.calls
                n_enc = sum(1 for c in s.calls if c[0] == "encode_trail")
                assert n_enc == (3 if s0.downloads else 0), (n_enc, s0.downloads)
    assert len(set(device(PA, PB, pre, 1000, 1e-20, 5)[0])) >= 3          # columns stop at different iterations
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_on_batch_flips_reach_the_next_batch_and_the_host_decode():
    out = child(STANDIN + r'''
k = PB.shape[1]
rec = 2 * k + 2
it0, rr0, x0, h0, s0 = tdevice(PA, PB, False, 1000, 1e-20, 3)
seen, box = [], []
class Probe(TRec):
    def __init__(self, A):
        super().__init__(A)
        box.append(self)
def on_batch(done, trail):
    seen.append(done)
    assert trail.a.size == 2 * (rec * 4 + k + 1)
    if done == 3:
        box[0].flip_trail(trail, rec * 3 + k + 1, [70])     # r.z[1] of record `stride`: the next iteration repairs it
    if done == 6:
        box[0].flip_trail(trail, rec * 3 + 2 * k, [5])      # its events word: nobody reads it before the host does
it, rr, x, h, s = tdevice(PA, PB, False, 1000, 1e-20, 3, on_batch=on_batch, cls=Probe)
assert it == it0 and same_history(h, h0) and np.array_equal(bits(x), bits(x0))
assert seen[:3] == [3, 6, 9] and seen == sorted(seen) and len(seen) == s.downloads
assert s.repaired == [(k + 1, 70)], s.repaired             # reached the next batch, there once
# record 0's events word (the batch's first copy took it there), once; the r.z flip never reaches the host
assert s.reported == [(2 * k, 1, 5)], s.reported
# on_batch without the keyword: the unprotected loop, the same callbacks
calls = []
sp = DRec(PA)
v = vecs(PB)
sp.x = v[1]
cg_solve_block_device(sp, None, *v, 1000, 1e-20, stride=3, on_batch=lambda done, trail: calls.append((done, trail.a.size)))
assert [d for d, _ in calls] == seen and all(n == rec * 4 + k + 1 for _, n in calls)
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_the_default_path_makes_todays_calls_on_a_context_without_the_new_methods():
    out = child(STANDIN + r'''
class Old(DRec):
    def __getattr__(self, name):
        raise AssertionError("a new context method was called: " + name)
def solve(**kw):
    s = Old(PA)
    v = vecs(PB)
    s.x = v[1]
    out = cg_solve_block_device(s, None, *v, 1000, 1e-20, stride=3, **kw)
    return out, s.calls, s.downloads, s.launches, bits(v[1].a)
base, kw = solve(), solve(trail_ecc=False, on_batch=None)
assert base[0][0] == kw[0][0] and np.array_equal(bits(base[0][1]), bits(kw[0][1]))
assert base[1:4] == kw[1:4] and np.array_equal(base[4], kw[4])
assert not any(c[0] == "encode_trail" for c in base[1])
print("ok")
''')
    assert out.strip().endswith("ok"), out
