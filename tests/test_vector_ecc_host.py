"""Protected vectors, the parts that need no GPU: the numpy model of the
(64, 57) code against the constants and known answers of the specification, its decode rule on
single and double flips, the NaN rule, the refusals of cg_solve and of the command line, and the
texts of the two vector events."""
import os
import sys

import numpy as np
import pytest

import _vecc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MASKS = [0xaaaaaaab5556ad82, 0xcccccccd999b3684, 0xf0f0f0f1e1e3c708, 0xff00ff01fe03f810, 0xffff0001fffc0020,
         0xfffffffe00000040]
KNOWN = [(0x3ff0000000000000, 0x3ff0000000000003), (0xc004000000000000, 0xc004000000000067), (0x0, 0x0),
         (0x000012688b70e62b, 0x000012688b70e66e), (0x7ff0000000000000, 0x7ff000000000007f),
         (0x400921fb54442d18, 0x400921fb54442d7c)]


def test_model_reproduces_the_masks_and_known_answers():
    assert [int(m) for m in _vecc.MASKS] == MASKS
    clean = np.array([c for c, _ in KNOWN], np.uint64).view(np.float64)
    assert [int(w) for w in _vecc.encode(clean)] == [s for _, s in KNOWN]
    # a codeword: every check and the overall parity even; its value is the double cut to 57 bits
    w = _vecc.encode(clean)
    assert not _vecc.syndrome(w).any() and not _vecc.parity(w).any()
    assert np.array_equal(_vecc.strip(w).view(np.uint64), clean.view(np.uint64) & ~np.uint64(0x7F))


def test_single_flips_are_repaired_and_double_flips_classed():
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 1 << 63, 50, dtype=np.uint64) | (rng.integers(0, 2, 50, dtype=np.uint64) << np.uint64(63))
    good = _vecc.encode(raw.view(np.float64))
    w, status, _ = _vecc.decode(good)
    assert np.array_equal(w, good) and not status.any()
    for b in range(64):
        w, status, bit = _vecc.decode(good ^ np.uint64(1 << b))
        assert np.array_equal(w, good) and (status == 1).all() and (bit == b).all(), b
    for _ in range(40):  # sampled pairs of distinct bits, the same pair in all 50 words
        i, j = rng.choice(64, 2, replace=False)
        bad = good ^ np.uint64((1 << int(i)) | (1 << int(j)))
        w, status, bit = _vecc.decode(bad)
        assert np.array_equal(w, bad) and (status == 2).all() and (bit == -1).all(), (i, j)


def test_nan_rule():
    nans = np.array([0x7FF0000000000041, 0xFFF000000000007F, 0x7FF8000000000000, 0x7FF0000000000080,
                     0x7FF4000000000001], np.uint64)
    w = _vecc.encode(nans.view(np.float64))
    assert np.isnan(_vecc.strip(w)).all()
    # payload only in the cut bits: bit 51 set; a payload that survives the cut: kept as it is
    assert [int(x) & ~0x7F for x in w] == [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000000,
                                           0x7FF0000000000080, 0x7FF4000000000000]
    inf = _vecc.encode(np.array([np.inf, -np.inf]))
    assert np.array_equal(_vecc.strip(inf), [np.inf, -np.inf])


def test_cg_solve_refuses_what_writes_unencoded_vectors():
    sys.path.insert(0, ROOT)
    from abft_sparse_cg_amd.context import cg_solve

    class Ctx:
        calls = []

        def vecc_supported(self, A):
            return A.ok

        def matrix_info(self, A):
            return ("sweep", 1)

        def __getattr__(self, name):  # any call into the library is a failure of the test
            raise AssertionError("cg_solve called %s before refusing" % name)

    class Mat:
        fmt, ok = 0, True

    ctx, A, bad = Ctx(), Mat(), Mat()
    bad.ok = False
    v = object()
    with pytest.raises(ValueError, match="check_every"):
        cg_solve(ctx, A, v, v, v, v, v, vector_ecc=True, check_every=5)
    with pytest.raises(ValueError, match="precond"):
        cg_solve(ctx, A, v, v, v, v, v, vector_ecc=True, precond=v)
    with pytest.raises(ValueError, match="streaming layout"):
        cg_solve(ctx, bad, v, v, v, v, v, vector_ecc=True)


def test_command_line_refusals(capsys):
    sys.path.insert(0, ROOT)
    from abft_sparse_cg_amd import cg
    o = cg.parse(["cg"])
    assert o["vector_ecc"] == "none"
    o = cg.parse(["cg", "--vector-ecc", "secded", "--flip-vector", "10:w:7:55", "--flip-vector", "2:b:0:40"])
    assert o["vector_ecc"] == "secded" and [f[1] for f in o["flip_vector"]] == ["w", "b"]
    for extra, word in ((["--rhs", "2"], "--rhs"), (["--precond", "jacobi"], "--precond"),
                        (["--check-every", "5"], "--check-every"), (["--format", "coo"], "coo")):
        with pytest.raises(SystemExit) as e:
            cg.parse(["cg", "--vector-ecc", "secded"] + extra)
        assert e.value.code == 1
        assert word in capsys.readouterr().out
    for args in (["--vector-ecc"], ["--vector-ecc", "sed"], ["--flip-vector", "1:w:0:3"], ["--flip-vector", "1:b:0:3"],
                 ["--vector-ecc", "secded", "--flip-vector", "1:q:0:3"]):
        with pytest.raises(SystemExit) as e:
            cg.parse(["cg"] + args)
        assert e.value.code == 1, args
        capsys.readouterr()


def test_event_texts_and_fatality():
    sys.path.insert(0, ROOT)
    from abft_sparse_cg_amd import capi
    assert capi.format_event(10, 777, 55 | (2 << 8), 2) == "[ECC] corrected bit 55 of vector operand 2 at index 777\n"
    assert capi.format_event(11, 12, 1 << 8, 2) == "[ECC] double-bit error detected in vector operand 1 at index 12\n"
    assert not capi.is_fatal(10) and capi.is_fatal(11)
    lib = capi.load()
    assert lib.abft_event_is_fatal(10) == 0 and lib.abft_event_is_fatal(11) == 1
    for kind in range(1, 10):  # the existing kinds keep their rule
        assert bool(lib.abft_event_is_fatal(kind)) == capi.is_fatal(kind) == (kind in (1, 4, 5, 6, 7, 8, 9))
