"""The protected scalar trail (abft_sparse_cg_amd/csrc/trail_ecc.h) without a GPU:
tests/host/trail_ecc_play.cpp compiles the header -- the text the kernels compile -- for the host, with
AddressSanitizer and UBSan, as a program of its own.

  * the slot code against the oracle's COO secded element (tests/_structecc.py's blk_words model): +-0.0, denormals,
    +-inf, NaNs with payloads, ordinary values, under every ordinal of a record; a codeword of another ordinal (or
    with word 1 set) told from one in its place; all 128 single flips repaired with the right bit, all 8128 double
    flips detected and the words left as they are;
  * TrailSingle<QUAD> against the model of guard_protocol.h: the inputs are test_guard_protocol_host.py's single cases
    (pair and quad, its five thresholds), every one with a flipped bit in one or more of the slots a launch reads;
    live, alpha, beta, the frozen hand-on (NaN payloads and -0.0 kept) and the publication, bit for bit;
  * planted mistakes, each caught;
  * cg_solve_device(trail_ecc=True) on a stand-in context (that of test_device_loop_host.py, extended by the protected
    iteration on slots): the call sequences, the check_every refusal, and the default path making today's calls."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _structecc as S  # noqa: E402
import test_guard_protocol_host as G  # noqa: E402
from test_device_loop_host import STANDIN as BASE, child  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "abft_sparse_cg_amd", "csrc")
U = np.uint64
HEADERS = ["trail_ecc.h", "struct_ecc.h", "ecc_device.h", "guard_protocol.h"]
NEW = ["abft_hip_cg_trail_iteration_until_dev", "abft_hip_pcg_trail_iteration_until_dev",
       "abft_hip_cg_vecc_trail_iteration_until_dev", "abft_hip_pcg_vecc_trail_iteration_until_dev",
       "abft_hip_trail_encode", "abft_hip_trail_decode", "abft_hip_trail_flip", "abft_hip_trail_inject_at"]


def build(include_dir, out_dir):
    exe = os.path.join(str(out_dir), "trail_ecc_play")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-Wno-unknown-pragmas", "-I", str(include_dir), os.path.join(HERE, "host", "trail_ecc_play.cpp"), "-o", exe],
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
    return build(CSRC, tmp_path_factory.mktemp("trail_ecc"))


def test_header_needs_no_gpu():
    with open(os.path.join(CSRC, "trail_ecc.h")) as f:
        text = f.read()
    assert re.findall(r"#include\s*[\"<]([^\">]+)", text) == ["stdint.h", "guard_protocol.h", "struct_ecc.h"]
    assert not re.search(r"\bhip[A-Z]\w*\(|threadIdx|blockIdx|__global__|__shared__", text)
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert re.search(r"^HDRS\s*=.*\btrail_ecc\.h\b", f.read(), re.M)


def test_header_and_library_have_the_entries():
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
for m in ("cg_trail_iteration_until_dev", "pcg_trail_iteration_until_dev", "cg_vecc_trail_iteration_until_dev",
          "pcg_vecc_trail_iteration_until_dev", "flip_trail", "trail_inject_at", "encode_trail", "decode_trail"):
    assert callable(getattr(amd.HIPContext, m)), m
# keyword-only, behind every positional parameter: positional calls are unchanged, and so is the list of those
# (test_device_loop_check_host.py pins it through inspect.signature, which follows the wrapper to that list)
assert amd.cg_solve_device.__kwdefaults__ == {"trail_ecc": False, "on_batch": None}
assert list(inspect.signature(amd.cg_solve_device).parameters)[-1] == "on_check"
assert "trail_ecc=False, on_batch=None" in amd.cg_solve_device.__doc__
try:
    amd.cg_solve_device(*([None] * 19), True)
except TypeError:
    pass
else:
    raise AssertionError("a twentieth positional argument was taken")
assert capi.is_fatal(capi.EV_TRAIL_DOUBLE) and not capi.is_fatal(capi.EV_TRAIL_CORRECTED)
assert capi.format_event(14, 2, 77 | (1 << 8), 0) == "[ECC] corrected bit 77 of trail word 2 (p.w pair)\\n"
assert capi.format_event(14, 0, 24, 0) == "[ECC] corrected bit 24 of trail word 0 (start record)\\n"
assert capi.format_event(15, 2, 2 << 8, 0) == "[ECC] double-bit error detected in trail word 2 (next record)\\n"
print("ok")
""" % (NEW,))
    assert out.strip() == "ok"


# ---- the slot code against the oracle ----

def slot_values():
    f = lambda v: int(np.float64(v).view(U))
    vals = [f(0.0), f(-0.0), 1, 0x000FFFFFFFFFFFFF, 0x8000000000000001, f(np.inf), f(-np.inf), G.QNAN, G.NEG_NAN, G.SNAN,
            0x7FF8DEADBEEF1234, f(1.0), f(-1.5), f(1e-3), f(1.7976931348623157e308), f(2.2250738585072014e-308),
            f(3.0), f(16.0), 0xFFFFFFFFFFFFFFFF, 0x5555555555555555]
    rng = np.random.default_rng(11)
    vals += [int(v) for v in rng.integers(0, 1 << 63, 12, dtype=np.uint64)]
    return vals


def test_slots_are_the_oracles_coo_secded_elements(exe, tmp_path):
    cases = [(o, v) for v in slot_values() for o in (0, 1, 2, 3)] + [((1 << 24) - 1, 5), (0x123456, G.QNAN)]
    rc, lines, err = run(exe, tmp_path, "".join("slot %d %x\n" % c for c in cases))
    assert rc == 0, err[-3000:]
    assert len(lines) == len(cases) * 130
    want = S.blk_words([(o, 0, v & 0xFFFFFFFF, v >> 32) for o, v in cases])
    for k, (o, v) in enumerate(cases):
        block = [line.split() for line in lines[130 * k:130 * k + 130]]
        got = [int(t, 16) for t in block[0][1:5]]
        assert block[0][0] == "slot" and block[0][5] == "0"
        assert got == [int(w) for w in want[k]], (o, hex(v), got, want[k])
        # words 2 and 3 the double, every bit; word 1 zero; the ordinal in bits 0..23 of word 0
        assert got[2] | (got[3] << 32) == v and got[1] == 0 and got[0] & 0xFFFFFF == o
        for b in range(128):  # every single flip: repaired, the right bit named
            s = block[1 + b]
            assert s[0] == "s" and int(s[1]) == b and int(s[2]) == 1, (o, hex(v), s)
            assert int(s[3], 16) == v and [int(t, 16) for t in s[4:8]] == got and int(s[8]) == b, (o, hex(v), s)
        assert block[129] == ["d", "8128", "8128"], (o, hex(v), block[129])  # every double flip: fatal, words kept


# ---- TrailSingle<QUAD> against the model of guard_protocol.h ----

def flips_for(n, quad):
    """a flipped bit for the slots of r.r, r.z, p.w and the next record's r.z of each of n cases (128: none): every
    bit of every slot is reached, alone and together with flips in the other slots"""
    i = np.arange(n)
    frr, frz, fpw, fnew = i % 129, (i // 3) % 129, (i // 7 + 64) % 129, (i // 11 + 100) % 129
    if not quad:
        frz = np.full(n, 128)
    return frr, frz, fpw, fnew


def text_of(single):
    lines = []
    for quad, c in single:
        n = len(c["thr"])
        cols = [c["thr"], c["nev"], c["rr"], c["rz"], c["pw"], c["new"]] + list(flips_for(n, quad))
        fmt = "single %d" % quad + " %x" * 6 + " %d" * 4
        lines += [fmt % row for row in zip(*(np.asarray(col).tolist() for col in cols))]
    return "\n".join(lines) + "\n"


def expect(quad, c):
    """rows of words: live, alpha, beta, the frozen hand-on, the publication -- G.expect_single, the model of
    guard_protocol.h, and behind it the record a live r half publishes: {new, events, new, +0.0}"""
    base = G.expect_single(quad, c)
    events = G.b64(c["nev"].astype(np.float64))
    published = [c["new"], events] + ([c["new"], np.zeros_like(events)] if quad else [])
    return np.concatenate([base, np.stack(published, axis=1)], axis=1)


def mismatches(exe, tmp, single):
    rc, lines, err = run(exe, tmp, text_of(single))
    if rc != 0:
        return [("program", rc, err[-500:])]
    bad, at = [], 0
    for quad, c in single:
        want = expect(quad, c)
        got = lines[at:at + len(want)]
        at += len(want)
        words = np.array([[int(w, 16) for w in g.split()[1:-1]] for g in got], dtype=U)
        repairs = np.array([int(g.split()[-1]) for g in got])
        assert all(g.startswith("s ") for g in got) and words.shape == want.shape, (quad, words.shape, want.shape)
        f = np.stack(flips_for(len(want), quad), axis=1)
        bad += [("single", quad, int(i)) for i in np.flatnonzero((words != want).any(axis=1))]
        bad += [("repairs", quad, int(i)) for i in np.flatnonzero(repairs != (f < 128).sum(axis=1))]
    assert at == len(lines)
    return bad


@pytest.fixture(scope="module")
def cases():
    return [(0, G.single_cases(False)), (1, G.single_cases(True))]


def test_protected_records_give_guard_protocols_bits(exe, cases, tmp_path):
    bad = mismatches(exe, tmp_path, cases)
    assert not bad, (len(bad), bad[:10])
    assert sum(len(c["thr"]) for _, c in cases) == 8640 + 103680
    for quad, c in cases:  # what the cases reach: both verdicts, special values frozen, every bit of every slot flipped
        with np.errstate(all="ignore"):
            live = G.f64(c["rr"]) > G.f64(c["thr"])
        assert live.any() and (~live).any()
        frozen = set(c["rr"][~live].tolist())
        assert {G.QNAN, G.NEG_NAN, G.SNAN, int(G.b64(-0.0))} <= frozen  # payloads and -0.0 through the hand-on
        for f in flips_for(len(live), quad)[:1 + 3 * quad] + flips_for(len(live), quad)[2:]:
            assert set(range(129)) <= set(np.asarray(f).tolist())


MISTAKES = {
    "the ordinal is left out of the code":
        ("trail_ecc.h", "  blk_encode(w);\n}", "  { const uint32_t o = w[0]; w[0] = 0u; blk_encode(w); w[0] |= o; }\n}"),
    "the value is read from the unrepaired words":
        ("trail_ecc.h", "t.bits = trail_bits(t.w);", "t.bits = trail_bits(w);"),
    "the frozen hand-on goes through a double add":
        ("trail_ecc.h", "trail_put(out, i, guard_word(plain_out, i));", "trail_put_value(out, i, plain_out[i] + 0.0);"),
    "the publication swaps r.z and r.r":
        ("trail_ecc.h", "trail_put_value(out, RZ, rz_new);", "trail_put_value(out, RZ, rr_new + 1.0);"),
    "the ordinal is not compared with the place":
        ("trail_ecc.h", "return ((w[0] ^ ordinal) & ABFT_TRAIL_ORDINAL_MASK) | w[1];", "(void)ordinal; return w[1];"),
    "a repair flips the wrong word":
        ("struct_ecc.h", "if ((bit >> 5) == (uint32_t)k) o.w[k] ^= 1u << (bit & 31u);",
         "if ((bit >> 5) == (uint32_t)k) o.w[k ^ 1] ^= 1u << (bit & 31u);"),
}


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_a_planted_mistake_is_caught(cases, tmp_path, mistake):
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
    # the slot requests: the program's own checks, or the comparison with the oracle
    slots = [(o, v) for v in slot_values()[:6] for o in (0, 1, 2, 3)]
    rc, lines, _ = run(bad_exe, tmp_path, "".join("slot %d %x\n" % c for c in slots))
    slot_bad = rc != 0
    if rc == 0:
        want = S.blk_words([(o, 0, v & 0xFFFFFFFF, v >> 32) for o, v in slots])
        for k, (o, v) in enumerate(slots):
            block = [line.split() for line in lines[130 * k:130 * k + 130]]
            slot_bad |= [int(t, 16) for t in block[0][1:5]] != [int(w) for w in want[k]]
            slot_bad |= any(int(s[2]) != 1 or int(s[3], 16) != v for s in block[1:129])
    quad = {k: v[:4000] for k, v in cases[1][1].items()}
    pair = {k: v[:4000] for k, v in cases[0][1].items()}
    single_bad = mismatches(bad_exe, tmp_path, [(0, pair), (1, quad)])
    assert slot_bad or single_bad, mistake
    if "hand-on" in mistake or "publication" in mistake or "unrepaired" in mistake:
        assert single_bad and not slot_bad or "unrepaired" in mistake


# ---- cg_solve_device(trail_ecc=True) on the stand-in ----
# The protected iteration of the stand-in keeps its scalars as slots through the library's own host functions
# (abft_hip_trail_encode / abft_hip_trail_decode need no GPU) and computes what DSingle.cg_iteration_until_dev computes.
STANDIN = BASE + r'''
import ctypes as C
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

class TSingle(DSingle):
    def __init__(self, A):
        super().__init__(A)
        self.reported, self.trail_calls = [], 0
    def encode_trail(self, values, first_ordinal=0):
        self.calls.append(("encode_trail", len(values)))
        return enc(values, first_ordinal)
    def report_trail(self, slots, rec, stride):
        assert len(slots) == 2 * (rec * (stride + 1) + 2)
        v, st, b = dec(slots)
        self.reported += [(int(j), int(st[j]), int(b[j])) for j in np.flatnonzero(st)]
        return v
    def flip_trail(self, trail, slot, bits):
        w = trail.a.view(np.uint32)
        for bit in bits:
            w[4 * slot + (bit >> 5)] ^= np.uint32(1 << (bit & 31))
    def cg_trail_iteration_until_dev(self, A, vec, x, r, p, w, sc, rr_at, pw_at, new_at, thr):
        assert vec is p and rr_at % 2 == 0 and pw_at % 2 == 0 and new_at % 2 == 0
        self.trail_calls += 1
        if self.rec is None:
            self.eager += 1
        def f():
            (rr, _), st, _ = dec(sc.a[rr_at:rr_at + 4])
            assert st[0] >= 0
            if st[0]:
                sc.a[rr_at:rr_at + 2] = enc([rr], 0)          # repaired in place
            rr = float(rr)
            if not (rr > thr):
                sc.a[new_at:new_at + 4] = enc([rr, 0.0], 0)
                self.frozen += 1
                return
            self.live += 1
            w.a[:] = self.A @ vec.a
            pw = float(np.sum(vec.a * w.a))
            sc.a[pw_at:pw_at + 4] = enc([pw, 0.0], 0)
            alpha = fdiv(rr, pw)
            x.a[:] = x.a + alpha * p.a; r.a[:] = r.a - alpha * w.a
            rr_new = float(np.sum(r.a * r.a))
            sc.a[new_at:new_at + 4] = enc([rr_new, 0.0], 0)
            p.a[:] = r.a + fdiv(rr_new, rr) * p.a
        self.do(f)

def trail_device(A, b, max_itrs, conv, stride, graph=True, on_batch=None, **kw):
    s = TSingle(A)
    n = len(b)
    vb, vx, vr, vp, vw = V(b.copy()), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n)), V(np.zeros(n))
    hist = []
    it, rr = cg_solve_device(s, None, vb, vx, vr, vp, vw, max_itrs, conv,
                             on_iteration=lambda i, v: hist.append((i, v)), stride=stride, graph=graph, trail_ecc=True,
                             on_batch=on_batch, **kw)
    return it, rr, vx.a, hist, s
'''


def test_protected_loop_is_the_device_loop_bit_for_bit_on_the_standin():
    out = child(STANDIN + r'''
for max_itrs, conv in ((1000, 1e-20), (23, 1e-20), (1000, 1e-3), (0, 1e-20)):
    for stride in (1, 3, 16):
        for graph in (True, False):
            it0, rr0, x0, h0, s0 = device(A, b, max_itrs, conv, stride, graph)
            it, rr, x, h, s = trail_device(A, b, max_itrs, conv, stride, graph)
            assert it == it0 and np.array_equal(bits([rr]), bits([rr0])), (stride, it, it0)
            assert h == h0 and np.array_equal(bits(x), bits(x0)), stride
            # the same batches, downloads, launches and eager calls; the guarded calls are the protected ones
            assert (s.downloads, s.launches, s.eager, s.live, s.frozen) == (s0.downloads, s0.launches, s0.eager, s0.live, s0.frozen)
            assert s.trail_calls == (s.eager + (stride if s.launches else 0)) and not s.reported
            names0 = [c[0] for c in s0.calls]
            names = [c[0] for c in s.calls]
            assert [c for c in names if c != "encode_trail"] == names0
            # the whole trail is encoded at the start: a record of +0.0, the pair, the seed record
            assert names.count("encode_trail") == (3 if it0 or (max_itrs and rr0 > conv) else 0)
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_on_batch_flips_reach_the_next_batch_and_the_host_decode():
    out = child(STANDIN + r'''
it0, rr0, x0, h0, _ = trail_device(A, b, 1000, 1e-20, 3)
seen = []
def on_batch(done, trail):
    seen.append(done)
    if done == 3:
        s_ref[0].flip_trail(trail, 2 * 3 + 0, [70])     # r.r of record `stride`: the iteration repairs it
    if done == 6:
        s_ref[0].flip_trail(trail, 2 * 3 + 1, [5])      # its events word: nobody reads it before the host does
s_ref = [None]
class Probe(TSingle):
    def __init__(self, A):
        super().__init__(A)
        s_ref[0] = self
TSingle_, TSingle = TSingle, Probe
it, rr, x, h, s = trail_device(A, b, 1000, 1e-20, 3, on_batch=on_batch)
assert (it, h) == (it0, h0) and np.array_equal(bits(x), bits(x0))
assert seen[:3] == [3, 6, 9] and seen == sorted(seen)
assert s.reported == [(1, 1, 5)], s.reported            # record 0's events word, once; the r.r flip never reaches the host
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_check_every_is_refused_and_the_default_path_makes_todays_calls():
    out = child(STANDIN + r'''
s = TSingle(A)
v = [V(b.copy())] + [V(np.zeros(n)) for _ in range(4)]
try:
    cg_solve_device(s, None, *v, 100, 1e-3, check_every=5, trail_ecc=True)
except ValueError as e:
    assert "check_every" in str(e) and "trail_ecc" in str(e)
else:
    raise AssertionError("not refused")
assert s.calls == [] and s.downloads == 0                # before anything runs
# trail_ecc=False: a context without one of the new methods is enough, and the calls are those of a call without it
class Old(DSingle):
    def __getattr__(self, name):
        raise AssertionError("a new context method was called: " + name)
def solve(**kw):
    s = Old(A)
    v = [V(b.copy())] + [V(np.zeros(n)) for _ in range(4)]
    out = cg_solve_device(s, None, *v, 1000, 1e-20, stride=3, **kw)
    return out, s.calls, s.downloads, s.launches, bits(v[1].a)
base, kw = solve(), solve(trail_ecc=False, on_batch=None)
assert base[:4] == kw[:4] and np.array_equal(base[4], kw[4])
print("ok")
''')
    assert out.strip().endswith("ok"), out


def test_on_batch_runs_with_residual_checks_too():
    """on_batch is not the protected trail's alone: with check_every > 0 (and trail_ecc off) it runs behind every
    batch of the checked loop, behind that batch's on_check"""
    from test_device_loop_check_host import STANDIN as CHECKED
    out = child(CHECKED + r'''
it0, rr0, x0, h0, c0, s0 = cdevice(A, b, 40, 1e-20, 4, check_every=5)
order = []
it, rr, x, h, c, s = cdevice(A, b, 40, 1e-20, 4, check_every=5, on_batch=lambda done, trail: order.append((done, trail.a.size)))
assert (it, h, c) == (it0, h0, c0) and np.array_equal(x, x0) and s.calls == s0.calls
dones = [d for d, _ in order]
assert dones == sorted(dones) and dones[-1] == it
assert len(dones) == sum(1 for k in s.calls if k[0] == "download" and k[1] == 2 * 5 + 4 + 2)   # once per downloaded trail
assert all(size == 2 * 5 + 4 + 2 for _, size in order)   # the trail of pairs with the pair and the check's four words
print("ok")
''')
    assert out.strip().endswith("ok"), out
