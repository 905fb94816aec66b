"""The protected CSR row structure (abft_sparse_cg_amd/csrc/struct_ecc.h) without a GPU: tests/host/
struct_ecc_play.cpp compiles the header and ecc_device.h -- the text the kernels compile -- for the host, with
AddressSanitizer and UBSan, and runs every encode and every cold decode.  Row extent words are held against the model
of tests/_vecc.py applied to the packed integer, row-block descriptors against the oracle's COO secded element
(tests/_oracle.py, pinned to the reference).  Every comparison is bit for bit; no word, bit or pair of bits is left
out.  The last tests prove, through layout_plan.h, that the matrices of tests/test_gpu_structure_ecc.py reach every
branch of the protected kernel."""
import os
import re
import subprocess

import numpy as np
import pytest

import _layout_cases as LC
import _structecc as S
import _vecc as V
from _oracle import COO, Oracle
from _structecc import matrix

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "abft_sparse_cg_amd", "csrc")
U = np.uint64
M28 = (1 << 28) - 1
GEO = LC.geometry(CSRC)
BLOCK, TILE = GEO[0], GEO[1]
PLANNED = S.NAMES


def extents():
    rng = np.random.default_rng(2024)
    out = [(0, 0), (0, M28), (M28, M28), (M28, 0), (1, 2), (5, 5)]
    out += [tuple(int(v) for v in rng.integers(0, 1 << 28, 2)) for _ in range(300)]
    out += [(a, a + int(d)) for a, d in zip(rng.integers(0, 1 << 27, 60).tolist(), rng.integers(0, 2000, 60))]
    return out


def descriptors():
    """{first row, end row | flag, first element, end element} as a plan holds them, and a few that use every field's width"""
    rng = np.random.default_rng(7)
    out = [(0, 0, 0, 0), (0, 1, 0, 1), ((1 << 24) - 1, (1 << 24) | (1 << 31), M28, M28), (0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)]
    for _ in range(40):
        r0 = int(rng.integers(0, 1 << 24))
        r1 = min(r0 + int(rng.integers(1, 1025)), 1 << 24) | (int(rng.integers(0, 2)) << 31)
        e0 = int(rng.integers(0, 1 << 28))
        out.append((r0, r1, e0, min(e0 + int(rng.integers(0, 1025)), M28)))
    return out


def _define(name, where="abft_internal.h"):
    with open(os.path.join(CSRC, where)) as f:
        return "-D%s=%s" % (name, re.search(r"#define\s+%s\s+(\w+)" % name, f.read()).group(1))


@pytest.fixture(scope="module")
def play(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("struct_ecc") / "struct_ecc_play")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    _define("ABFT_PAL_ENTRIES"), _define("ABFT_CBASE_WIDE"), _define("ABFT_PAL_SPARE", "abft_hip.hip"), "-I", CSRC,
                    os.path.join(HERE, "host", "struct_ecc_play.cpp"), "-o", exe], check=True)
    # (the leak check at exit needs ptrace rights a sandbox may withhold; the program frees through destructors)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")

    def run(text):
        p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, p.stderr[-3000:]
        return [line.split() for line in p.stdout.splitlines()]
    return run


def pack(rs, re_):
    return (rs << 7) | (re_ << 35)


def test_header_needs_no_gpu():
    with open(os.path.join(CSRC, "struct_ecc.h")) as f:
        text = f.read()
    assert re.findall(r"#include\s*[\"<]([^\">]+)", text) == ["stdint.h", "ecc_device.h"]
    assert not re.search(r"\bhip[A-Z]\w*\(|threadIdx|blockIdx|__global__|__shared__", text)


def test_row_words(play):
    ext = extents()
    lines = play("".join("row %d %d\n" % e for e in ext))
    assert len(lines) == len(ext) * 66
    packed = np.array([pack(*e) for e in ext], dtype=U)
    # the model of the protected vectors on the packed integer, seen through a float64 view (bits 0..6 are clear, so
    # even where the pattern is a NaN's the model cuts no payload off and sets no bit 51)
    model = V.encode(packed.view(np.float64))
    assert np.array_equal(model & ~V.CODE, packed)
    for k, e in enumerate(ext):
        blockl = lines[66 * k:66 * k + 66]
        assert blockl[0][0] == "row"
        w = int(blockl[0][1], 16)
        assert w & ~0x7F == pack(*e) and w >> 63 == 0, e
        assert w == int(model[k]), (e, hex(w), hex(int(model[k])))
        # ... and by the model's own parity rule, whatever the pattern: a codeword
        assert V.decode(np.array([w], dtype=U))[1][0] == 0, e
        singles = blockl[1:65]
        assert [int(s[1]) for s in singles] == list(range(64))
        flipped = np.array([w ^ (1 << b) for b in range(64)], dtype=U)
        rep, status, bit = V.decode(flipped)
        for b, s in enumerate(singles):
            assert s[0] == "s" and int(s[2]) == 1 and int(s[3], 16) == w and int(s[4]) == b, (e, s)
            assert status[b] == 1 and int(rep[b]) == w and int(bit[b]) == b
        assert blockl[65] == ["d", "2016", "2016"], (e, blockl[65])
    # all 2016 double flips by the model as well: fatal, the word left as it is
    a, b = np.triu_indices(64, 1)
    for e in ext[:8]:
        w = int(play("row %d %d\n" % e)[0][1], 16)
        both = np.array([w ^ (1 << int(i)) ^ (1 << int(j)) for i, j in zip(a, b)], dtype=U)
        rep, status, _ = V.decode(both)
        assert len(both) == 2016 and np.all(status == 2) and np.array_equal(rep, both)


def test_descriptors(play):
    descs = descriptors()
    lines = play("".join("blk %d %d %d %d\n" % d for d in descs))
    assert len(lines) == len(descs) * 130
    for k, d in enumerate(descs):
        blockl = lines[130 * k:130 * k + 130]
        got = [int(t, 16) for t in blockl[0][1:5]]
        want = Oracle.encode(COO, "secded", [d[0] & 0x00FFFFFF, d[1], d[2], d[3]])
        assert got == [int(v) for v in want], (d, got, want)
        assert blockl[0][5] == "0"
        assert got[0] & 0x00FFFFFF == d[0] & 0x00FFFFFF and got[1:] == list(d[1:])  # data untouched: the flag is data
        for b in range(128):
            s = blockl[1 + b]
            f = list(got)
            f[b >> 5] ^= 1 << (b & 31)
            assert s[0] == "s" and int(s[1]) == b and int(s[2]) == 1, (d, s)
            assert [int(t, 16) for t in s[3:7]] == got, (d, s)
            # the bit the oracle names: its syndrome's Hamming position -> bit, the parity bit when the syndrome is clear
            syn = Oracle.syndrome(COO, f)
            assert Oracle.parity(COO, f) == 1
            named = Oracle.flipped_bit(COO, syn) if syn else 24
            assert named == b and int(s[7]) == b, (d, b, named, s)
        assert blockl[129] == ["d", "8128", "8128"], (d, blockl[129])
    # the double flips by the oracle as well, on one descriptor: even parity and a set syndrome, all 8128
    got = [int(t, 16) for t in lines[0][1:5]]
    n = 0
    for a in range(128):
        for b in range(a + 1, 128):
            f = list(got)
            f[a >> 5] ^= 1 << (a & 31)
            f[b >> 5] ^= 1 << (b & 31)
            assert Oracle.parity(COO, f) == 0 and Oracle.syndrome(COO, f) != 0
            n += 1
    assert n == 8128


def test_limits(play):
    ask = [(1, (1 << 28) - 1), (1, 1 << 28), (1 << 24, 1), ((1 << 24) + 1, 1), (10_000_000, 105_000_000), (0, 0)]
    got = [int(line[1]) for line in play("".join("limit %d %d\n" % a for a in ask))]
    assert got == [0, 1, 0, 2, 0, 0]


@pytest.fixture(scope="module")
def plans(play):
    out = {}
    for name in PLANNED:
        cols, rows, vals, n = matrix(name)
        text = "plan %s %d %d %s %s\n" % (" ".join(str(g) for g in GEO), n, len(rows), " ".join(str(int(r)) for r in rows),
                                          " ".join(str(int(c)) for c in cols))
        line = play(text)[0]
        assert line[0] == "plan"
        blk = np.array([int(t) for t in line[2:]], dtype=np.int64).reshape(int(line[1]), 4)
        out[name] = (blk, S.rowptr_of(rows, n), n)
    return out


def test_plans_tile_the_rows(plans):
    for name, (blk, ptr, n) in plans.items():
        r0, r1, flag = blk[:, 0], blk[:, 1] & 0x7FFFFFFF, blk[:, 1] >> 31
        assert r0[0] == 0 and r1[-1] == n and np.array_equal(r0[1:], r1[:-1]), name
        assert np.array_equal(blk[:, 2], ptr[r0]) and np.array_equal(blk[:, 3], ptr[r1]), name
        for t in np.flatnonzero(flag):
            assert len(set(np.diff(ptr[r0[t]:r1[t] + 1]).tolist())) == 1, (name, t)
        assert n <= 3001 and ptr[-1] < 1 << 28


def one_tile(b):
    return b[3] >= b[2] and b[3] - (b[2] & ~1) <= TILE


def test_inputs_reach_every_branch(plans):
    flag = {name: plans[name][0][:, 1] >> 31 for name in plans}
    assert not flag["rand"].any()  # row words are read in every block
    # lap40 (the issue's name for it) has no uniform block: its rows change length every 40 rows.  wide5 has both kinds.
    assert not flag["lap40"].any()
    assert flag["wide5"].any() and not flag["wide5"].all()
    blk = plans["diag23"][0]
    rows = (blk[:, 1] & 0x7FFFFFFF) - blk[:, 0]
    # more rows than threads and no uniform flag: the row loop's `row != r` trips read row words (a third trip too)
    assert np.any((rows > 2 * BLOCK) & (flag["diag23"] == 0) & np.array([one_tile(b) for b in blk]))
    blk = plans["arrow"][0]
    assert not one_tile(blk[0]) and blk[0][0] == 0 and (blk[0][1] & 0x7FFFFFFF) == 1  # row 0 alone, longer than a tile
    blk, ptr, n = plans["holes"]
    assert np.any(np.diff(ptr) == 0) and not flag["holes"].all()
    assert len(plans["one"][0]) == 1 and len(plans["lap3"][0]) == 1
