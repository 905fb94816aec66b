"""The stop-test protocol of the guarded CG kernels (abft_sparse_cg_amd/csrc/guard_protocol.h) without a GPU:
tests/host/guard_protocol_play.cpp compiles the header -- the text the kernels compile -- for the host, with
AddressSanitizer and UBSan, and prints what its functions leave; everything is compared bit for bit with the numpy
model below, which is written from DESIGN.md sections 5f, 5g and 5h, not from the header.

116 160 cases.  Pair and quad records: the cross product of 5 thresholds (0.0, -0.0, 1e-3, +inf, NaN) and 12 values
(the threshold and its two neighbours, +-0.0, the smallest subnormal, a normal, +-inf, a quiet NaN with a payload, a
negative NaN, a signalling NaN) for each of r.r, p.w and the new sum (8 640 pair cases) and for r.r, r.z, p.w and the
new r.z (103 680 quad cases).  Block records (3 840 cases): K = 1, 2, 3 with every mask and K = 8 with the all-live,
all-frozen, single-live and single-frozen masks at each column, plain and PRECOND, at every threshold, the 12 values
rotated through the columns' r.r, r.z, P.W, new sums and totals in 12 rotations (a threshold nothing is above reaches
the empty mask only, whatever was planned)."""
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "abft_sparse_cg_amd", "csrc")
U = np.uint64
POISON = 0x7FF4DEAD0000BEEF


def f64(bits):
    return np.array(bits, dtype=U).view(np.float64)


def b64(x):
    return np.asarray(x, dtype=np.float64).view(U)


THRESHOLDS = [0.0, -0.0, 1e-3, np.inf, float(f64(0x7FF8000000000000))]
QNAN, NEG_NAN, SNAN = 0x7FF8000000001234, 0xFFF8000000000ABC, 0x7FF0000000000001
NEVS = [0, 1, 7, 0xFFFFFFFF]


def values(t):
    """the 12 values of a threshold, as bits"""
    t = np.float64(t)
    with np.errstate(all="ignore"):
        near = [t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf)]
    return [int(b64(v)) for v in near + [0.0, -0.0, 5e-324, 1.5, np.inf, -np.inf]] + [QNAN, NEG_NAN, SNAN]


def div(a, b):
    """the IEEE quotient of two arrays of bits, as bits"""
    with np.errstate(all="ignore"):
        return b64(f64(a) / f64(b))


# ---- the cases: dicts of uint64 arrays, one row a case ----

def single_cases(quad):
    rows = []
    for ti, t in enumerate(THRESHOLDS):
        v = values(t)
        for c in itertools.product(v, repeat=4 if quad else 3):
            rr, rz, pw, new = c if quad else (c[0], c[0], c[1], c[2])
            rows.append((int(b64(t)), NEVS[(len(rows) + ti) % 4], rr, rz, pw, new))
    a = np.array(rows, dtype=U)
    return dict(thr=a[:, 0], nev=a[:, 1], rr=a[:, 2], rz=a[:, 3], pw=a[:, 4], new=a[:, 5])


def masks(k):
    if k <= 3:
        return list(range(1 << k))
    full = (1 << k) - 1
    return [full, 0] + [1 << j for j in range(k)] + [full ^ (1 << j) for j in range(k)]


def block_cases(k, precond):
    """-> [(threshold bits, nev, the mask planned, in[2k+2], pw[k+1], out[2k+2], tot[S])], words as ints"""
    cases = []
    s_len = 2 * k if precond else k
    for t in THRESHOLDS:
        v = values(t)
        with np.errstate(all="ignore"):
            above = [x for x in v if float(f64(x)) > t]
        below = [x for x in v if x not in above]
        for mask in masks(k):
            for rot in range(len(v)):
                pick = lambda salt, j: v[(rot + salt * j + salt) % len(v)]
                rr = [(above[(rot + j) % len(above)] if (mask >> j) & 1 and above else below[(rot + j) % len(below)])
                      for j in range(k)]
                rec_in = rr + [pick(5, j) for j in range(k)] + [int(b64(3.0)), int(b64(-7.0))]
                rec_out = [pick(7, j) for j in range(k)] + [pick(11, j) for j in range(k)] + [QNAN, int(b64(9.0))]
                pw = [pick(1, j) for j in range(k)] + [int(b64(2.0))]
                tot = [v[(rot + 3 * i + 2) % len(v)] for i in range(s_len)]
                cases.append((int(b64(t)), NEVS[len(cases) % 4], mask if above else 0, rec_in, pw, rec_out, tot))
    return cases


def text_of(single, blocks):
    """the input of the program: single: [(quad, cases)], blocks: [(k, precond, cases)]"""
    lines = []
    for quad, c in single:
        n = len(c["thr"])
        rec_in = [c["rr"], np.full(n, b64(5.0)), c["rz"], np.full(n, b64(-3.0))]  # the events and trailing words: not moved
        rec_out = [c["new"], np.full(n, b64(6.0)), c["new"], np.full(n, b64(8.0))]
        cols = [c["thr"], c["nev"]] + rec_in + [c["pw"]] + rec_out
        fmt = "single %d" % quad + " %x" * len(cols)
        lines += [fmt % row for row in zip(*(col.tolist() for col in cols))]
    for k, precond, cases in blocks:
        for t, nev, _, rec_in, pw, rec_out, tot in cases:
            lines.append("block %d %d %x %x " % (k, precond, t, nev) + " ".join("%x" % w for w in rec_in + pw + rec_out + tot))
    return "\n".join(lines) + "\n"


# ---- the model ----

def expect_single(quad, c):
    """-> rows of words: live, alpha, beta, the record a frozen r half hands on"""
    with np.errstate(all="ignore"):
        live = (f64(c["rr"]) > f64(c["thr"])).astype(U)  # false for NaN, as `while (rr > conv)`
    num = c["rz"] if quad else c["rr"]
    events = b64(c["nev"].astype(np.float64))
    handed = [c["rr"], events] + ([c["rz"], np.zeros_like(events)] if quad else [])  # the words themselves; +0.0 behind
    return np.stack([live, div(num, c["pw"]), div(c["new"], num)] + handed, axis=1)


def expect_block(k, precond, case):
    t, nev, _, rec_in, pw, rec_out, tot = case
    a = lambda words: np.array(words, dtype=U)
    with np.errstate(all="ignore"):
        live = f64(a(rec_in[:k])) > float(f64(t))
    mask = sum(1 << j for j in range(k) if live[j])
    alpha = div(a(rec_in[k:2 * k]), a(pw[:k]))
    beta = div(a(rec_out[k:2 * k]), a(rec_in[k:2 * k]))
    tail = [int(b64(float(nev))), 0]  # the queued-event count as a double, +0.0
    handed = rec_in[:2 * k] + tail
    new_rr = [tot[2 * j + 1] if precond else tot[j] for j in range(k)]
    new_rz = [tot[2 * j] if precond else tot[j] for j in range(k)]
    published = ([new_rr[j] if live[j] else rec_in[j] for j in range(k)]
                 + [new_rz[j] if live[j] else rec_in[k + j] for j in range(k)] + tail)
    return [mask] + alpha.tolist() + beta.tolist() + handed + published


# ---- building, running, comparing ----

def build(include_dir, out_dir):
    exe = os.path.join(str(out_dir), "guard_protocol_play")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-I", str(include_dir), os.path.join(HERE, "host", "guard_protocol_play.cpp"), "-o", exe], check=True)
    return exe


def mismatches(exe, tmp, single, blocks):
    """run every case -> [(kind, parameters, case index)] of the cases whose output is not the model's, word for word"""
    path = os.path.join(str(tmp), "cases.txt")
    with open(path, "w") as f:
        f.write(text_of(single, blocks))
    # (the leak check at exit needs ptrace rights a sandbox may withhold; the program frees through destructors)
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    bad, at = [], 0
    for quad, c in single:
        want = expect_single(quad, c)
        got = lines[at:at + len(want)]
        at += len(want)
        assert all(g.startswith("s ") for g in got)
        got = np.array([[int(w, 16) for w in g.split()[1:]] for g in got], dtype=U)
        assert got.shape == want.shape, (quad, got.shape, want.shape)
        bad += [("single", quad, int(i)) for i in np.flatnonzero((got != want).any(axis=1))]
    for k, precond, cases in blocks:
        for i, case in enumerate(cases):
            w = lines[at].split()
            at += 1
            got = [int(w[1])] + [int(t, 16) for t in w[2:]]
            if w[0] != "b" or got != expect_block(k, precond, case):
                bad.append(("block", (k, precond), i))
    assert at == len(lines)
    return bad


@pytest.fixture(scope="module")
def all_cases():
    single = [(0, single_cases(False)), (1, single_cases(True))]
    blocks = [(k, precond, block_cases(k, precond)) for k in (1, 2, 3, 8) for precond in (0, 1)]
    return single, blocks


def test_every_case_has_the_models_bits(all_cases, tmp_path):
    single, blocks = all_cases
    exe = build(CSRC, tmp_path)
    bad = mismatches(exe, tmp_path, single, blocks)
    assert not bad, (len(bad), bad[:10])
    n = sum(len(c["thr"]) for _, c in single) + sum(len(c) for _, _, c in blocks)
    print("%d cases" % n)
    assert n == 116160


def test_the_cases_cover_what_they_claim(all_cases):
    single, blocks = all_cases
    for quad, c in single:
        with np.errstate(all="ignore"):
            live = f64(c["rr"]) > f64(c["thr"])
        assert live.any() and (~live).any()
        assert (c["rr"] == c["thr"]).any()  # r.r at the threshold itself: frozen
        assert not live[c["rr"] == c["thr"]].any()
        for special in (QNAN, NEG_NAN, SNAN, int(b64(-0.0)), int(b64(5e-324))):
            assert (c["rr"] == U(special)).any() and (c["pw"] == U(special)).any() and (c["new"] == U(special)).any()
        zero = int(b64(0.0))
        assert ((c["rz"] == U(zero)) & (c["pw"] == U(zero))).any()  # 0 / 0
        inf = int(b64(np.inf))
        assert ((c["rz"] == U(inf)) & (c["pw"] == U(inf))).any()  # inf / inf
        assert ((c["rz"] == b64(1.5)) & (c["pw"] == U(zero))).any()  # x / 0
        assert set(c["nev"].tolist()) == set(NEVS)
    for k, precond, cases in blocks:
        for t in THRESHOLDS[:3]:  # the thresholds something is above
            reached = {expect_block(k, precond, c)[0] for c in cases if c[0] == int(b64(t))}
            assert reached == set(masks(k)), (k, precond, t)
            assert all(expect_block(k, precond, c)[0] == c[2] for c in cases if c[0] == int(b64(t)))
        for t in THRESHOLDS[3:]:  # +inf, NaN: nothing is live
            assert {expect_block(k, precond, c)[0] for c in cases if c[0] == int(b64(t))} == {0}
        frozen_rr = {c[3][j] for c in cases for j in range(k)}
        assert {QNAN, NEG_NAN, SNAN, int(b64(-0.0))} <= frozen_rr  # special values reach the columns' r.r
    assert POISON not in {w for _, _, cases in blocks for c in cases for part in c[3:] for w in part}


MISTAKES = {
    "the comparison admits equality":
        ("return rr > threshold;", "return rr >= threshold;"),
    "a frozen word goes through a double add":
        ("rec[i] = __longlong_as_double((long long)w);", "rec[i] = __longlong_as_double((long long)w) + 0.0;"),
    "the two words of a PRECOND column are swapped":
        ("(PRECOND ? tot[2 * j + 1] : tot[j])", "(PRECOND ? tot[2 * j] : tot[j])"),
}


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_a_planted_mistake_is_caught(all_cases, tmp_path, mistake):
    """the comparison can fail: a private copy of the header with one mistake planted, over the pair and block cases"""
    old, new = MISTAKES[mistake]
    with open(os.path.join(CSRC, "guard_protocol.h")) as f:
        text = f.read()
    assert text.count(old) == 1
    inc = tmp_path / "inc"
    inc.mkdir()
    (inc / "guard_protocol.h").write_text(text.replace(old, new))
    single, blocks = all_cases
    bad = mismatches(build(inc, tmp_path), tmp_path, single[:1], blocks)
    assert bad
    kinds = {b[0] for b in bad}
    assert kinds == ({"block"} if "PRECOND" in mistake else {"single", "block"}), kinds
