"""The matrix digest (abft_sparse_cg_amd/csrc/matrix_digest.h) without a GPU: tests/host/matrix_digest_play.cpp compiles
the header -- the text the kernels and the C ABI's host code compile -- for the host, with AddressSanitizer and UBSan,
and runs as a program of its own.  The header's digest is held against the numpy model of tests/_digest.py on segments
of every byte length that takes another path (no byte, a short last word, a tail behind the last 16-byte group), the
detection argument the header states is checked exhaustively on a 64-word segment -- all 2 048 single and all
2 096 128 double flips --, and the limit, the names and the library's event text are pinned."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _digest as D

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "abft_sparse_cg_amd", "csrc")
LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 4096 + 2]


@pytest.fixture(scope="module")
def play(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("matrix_digest") / "matrix_digest_play")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-I", CSRC, os.path.join(HERE, "host", "matrix_digest_play.cpp"), "-o", exe], check=True)
    # (the leak check at exit needs ptrace rights a sandbox may withhold; the program frees what it allocates)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")

    def run(text):
        p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, p.stderr[-3000:]
        return [line.split() for line in p.stdout.splitlines()]
    return run


def hexed(b):
    return bytes(b).hex() if len(b) else "-"


def test_header_needs_no_gpu():
    with open(os.path.join(CSRC, "matrix_digest.h")) as f:
        text = f.read()
    assert re.findall(r"#include\s*[\"<]([^\">]+)", text) == ["stddef.h", "stdint.h"]
    code = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"\bhip[A-Z]\w*\(|threadIdx|blockIdx|__global__|__shared__|atomic", code)
    # the argument is stated where the definition is
    assert "2^b (2 i + 1)" in text and "the same bit of the same word" in text


def test_model_of_the_model():
    rng = np.random.default_rng(5)
    for n in LENGTHS[:-1] + [61]:
        b = rng.integers(0, 256, n, dtype=np.uint8)
        assert D.digest(b) == D.digest_exact(b), n
    assert D.digest(b"") == 0
    assert D.digest(bytes([1])) == 1 and D.digest(bytes([0, 0, 0, 0, 2])) == 6
    # wrap-around: the largest words at the largest weights of a small segment still agree with exact arithmetic
    assert D.digest(np.full(4000, 0xFF, np.uint8)) == D.digest_exact(np.full(4000, 0xFF, np.uint8))


def test_header_equals_the_model(play):
    rng = np.random.default_rng(2024)
    segs = []
    for n in LENGTHS:
        for _ in range(4):
            segs.append(rng.integers(0, 256, n, dtype=np.uint8))
        segs.append(np.full(n, 0xFF, np.uint8))
        segs.append(np.zeros(n, np.uint8))
    lines = play("".join("digest %s\n" % hexed(s) for s in segs))
    assert len(lines) == len(segs)
    for s, line in zip(segs, lines):
        assert line[0] == "digest"
        want = D.digest(s)
        assert int(line[1], 16) == want, (len(s), line)
        assert int(line[2], 16) == want, ("the kernel's cut", len(s), line)  # groups in another order, the tail apart


def test_every_single_and_every_double_flip_changes_the_digest(play):
    rng = np.random.default_rng(64)
    seg = rng.integers(0, 256, 256, dtype=np.uint8)  # 64 words
    seg[:4] = 0            # a zero word
    seg[4:8] = 0xFF        # and a full one
    line = play("flips %s\n" % hexed(seg))[0]
    assert line == ["flips", "2048", "2048", "2096128", "2096128"], line
    # the model on all single flips and on a seeded sample of the double ones
    d0 = D.digest(seg)
    for bit in range(2048):
        f = seg.copy()
        f[bit >> 3] ^= 1 << (bit & 7)
        assert D.digest(f) != d0, bit
    for a, b in rng.integers(0, 2048, (2000, 2)):
        if a == b:
            continue
        f = seg.copy()
        f[a >> 3] ^= 1 << (a & 7)
        f[b >> 3] ^= 1 << (b & 7)
        assert D.digest(f) != d0, (a, b)
    # a short last word: its flips count too (9 bytes: 72 singles, 2556 doubles)
    line = play("flips %s\n" % hexed(seg[:9]))[0]
    assert line == ["flips", "72", "72", "2556", "2556"], line


def test_swapping_two_unequal_words_changes_the_digest(play):
    rng = np.random.default_rng(8)
    seg = rng.integers(0, 256, 256, dtype=np.uint8)
    seg[8:12] = seg[100:104]  # one equal pair: not a swap
    line = play("swaps %s\n" % hexed(seg))[0]
    w = D.words(seg)
    pairs = sum(1 for i in range(64) for j in range(i + 1, 64) if w[i] != w[j])
    assert pairs == 2016 - 1
    assert line == ["swaps", str(pairs), str(pairs)], line
    f = seg.copy()
    f[0:4], f[252:256] = seg[252:256], seg[0:4]
    assert D.digest(f) != D.digest(seg)


def test_limit(play, monkeypatch):
    ask = [0, 1, 4, (1 << 33) - 3, 1 << 33, (1 << 33) + 1, 1 << 40]
    got = [(int(line[1]), int(line[2])) for line in play("".join("limit %d\n" % a for a in ask))]
    assert got == [(0, 0), (0, 1), (0, 1), (0, 1 << 31), (0, 1 << 31), (-4, (1 << 31) + 1), (-4, 1 << 38)]  # -4: ABFT_ERR_RANGE
    # the model refuses by the same rule (shown at a limit a test can allocate)
    monkeypatch.setattr(D, "MAX_WORDS", 4)
    assert D.digest(bytes(16)) == 0
    with pytest.raises(OverflowError):
        D.digest(bytes(17))


def test_every_kind_has_a_distinct_name(play):
    lines = play("names\n")
    kinds = [int(line[1]) for line in lines]
    names = [line[2] for line in lines]
    assert kinds == list(range(len(lines))) and names[-1] == "?" and "?" not in names[:-1]
    real = names[:-1]
    assert len(set(real)) == len(real) and real[0] == "none"
    # the issue's list: every array abft_internal.h shows a kernel reading
    for s in ["cols", "vals", "rowptr", "blk", "orig_index", "pos_of_orig", "gidx", "cols16", "cbase", "code16", "pdesc", "pal",
              "fast", "rowext", "sblk", "seg_base", "seg_ptr", "wbase", "counts", "sub", "rid", "elems", "grp_ptr", "coo_blk",
              "as_created"]:
        assert s in real, s
    # ... and none of the buffers kernels write
    for s in ["pace", "debug", "moved", "fuse_partials"]:
        assert s not in real, s
    # the header's enum and the names agree with what the library hands Python
    with open(os.path.join(CSRC, "matrix_digest.h")) as f:
        enum = dict((m.group(1).lower(), int(m.group(2))) for m in re.finditer(r"ABFT_SEG_(\w+) = (\d+)", f.read()))
    assert enum.pop("count") == len(real)
    assert sorted(enum.values()) == list(range(len(real)))
    for name, kind in enum.items():
        assert real[kind] == name, (name, kind)


def child(code):
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_library_event_text_names_and_keywords(play):
    names = [line[2] for line in play("names\n")][:-1]
    out = child("""
import inspect
import abft_sparse_cg_amd as amd
from abft_sparse_cg_amd import capi
assert capi.segment_names() == %r
assert capi.EV_MATRIX_DIGEST == 16 and capi.is_fatal(16) and capi.load().abft_event_is_fatal(16) == 1
for k, s in enumerate(capi.segment_names()):
    assert capi.format_event(16, k, 0, 0) == "[ABFT] matrix digest mismatch in segment %%s\\n" %% s
    assert capi.format_event(16, k, 0, 1) == "[ABFT] matrix digest mismatch in segment %%s\\n" %% s
assert capi.segment_kind("pal") == capi.segment_names().index("pal")
try:
    capi.segment_kind("none")
    raise SystemExit("none is no segment")
except ValueError:
    pass
for m in ("matrix_segments", "matrix_digest", "arm_matrix", "verify_matrix", "verify_matrix_dev", "read_segment", "flip_segment"):
    assert callable(getattr(amd.HIPContext, m)), m
# keyword-only and off by default; the positional lists are what they were
for f in (amd.cg_solve, amd.cg_solve_block, amd.cg_solve_device, amd.cg_solve_block_device):
    assert "matrix_check_every" not in inspect.signature(f).parameters
    assert "matrix_check_every=0" in f.__doc__.split("\\n\\n")[0], f.__name__
# the refusal of the device loop with both keywords comes before anything runs: no context is touched
try:
    amd.cg_solve_device(None, None, None, None, None, None, None, check_every=10, matrix_check_every=4)
    raise SystemExit("not refused")
except ValueError as e:
    assert "matrix_check_every" in str(e) and "check_every" in str(e)
for bad in (-1, 2.5):
    try:
        amd.cg_solve_device(None, None, None, None, None, None, None, matrix_check_every=bad)
        raise SystemExit("not refused")
    except ValueError:
        pass
print("ok")
""" % (names,))
    assert out.strip() == "ok"


def test_the_schedule_of_the_device_loops():
    """which batches carry a verification: those whose end count reaches or passes the next multiple of M; with the
    final one, a flip is seen at most M + stride - 1 iterations after it happened"""
    out = child("""
import types
from abft_sparse_cg_amd.context import _MatrixWatch
class W(_MatrixWatch):
    def __init__(self, every):
        self.every, self.fresh = every, False
        self.ctx = types.SimpleNamespace(matrix_verifications=0)
for M in (1, 7, 16, 50):
    for stride in (1, 3, 16):
        for max_itrs in (1, 15, 16, 17, 60):
            w, done, seen = W(M), 0, []
            while done < max_itrs:
                m = min(stride, max_itrs - done)
                v = w.due(done, m)
                assert v == any((i + 1) % M == 0 for i in range(done, done + m)), (M, stride, done)
                done += m
                if v:
                    w.enqueued()
                    seen.append(done)
            assert w.fresh == (bool(seen) and seen[-1] == done)
            assert w.ctx.matrix_verifications == len(seen)  # counted per batch, captured into a graph or not
            if not w.fresh:
                seen.append(done)  # final_dev
            for c in range(max_itrs + 1):  # a flip behind iteration count c
                assert min(s for s in seen if s >= c) - c <= M + stride - 1, (M, stride, max_itrs, c)
print("ok")
""")
    assert out.strip() == "ok"
