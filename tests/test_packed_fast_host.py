"""The fast words of packed row blocks (abft_sparse_cg_amd/csrc/layout_plan.h, packed_fast_word) without a GPU:
tests/host/packed_fast_play.cpp, built here with AddressSanitizer and UBSan and run as a program of its own, plans
seeded matrices at the library's geometry and at the toy one and checks every block's word against its conditions and
against what the SpMV skips on its strength (a broken expectation, or a sanitizer report, ends the program with a
non-zero status).  Here: that the cases reached what they were made for."""
import os
import re
import subprocess

import pytest

import _layout_cases as LC

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "abft_sparse_cg_amd", "csrc")
GEO = LC.geometry(CSRC)
FIELDS = ("blocks", "packed", "stage", "row", "window_fails", "alloc_only", "replanned")


def _define(name, where="abft_internal.h"):
    with open(os.path.join(CSRC, where)) as f:
        return "-D%s=%s" % (name, re.search(r"#define\s+%s\s+(\w+)" % name, f.read()).group(1))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("packed_fast") / "packed_fast_play")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    _define("ABFT_PAL_ENTRIES"), _define("ABFT_CBASE_WIDE"), _define("ABFT_PAL_SPARE", "abft_hip.hip"), "-I", CSRC,
                    os.path.join(HERE, "host", "packed_fast_play.cpp"), "-o", path], check=True)
    return path


def _play(exe, block, tile):
    # (the leak check at exit needs ptrace rights a sandbox may withhold; the program frees through destructors)
    p = subprocess.run([exe, str(block), str(tile)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0, p.stderr[-3000:]
    got = {}
    for line in p.stdout.splitlines():
        w = line.split()
        got[w[0]] = dict(zip(FIELDS, map(int, w[1:])))
    return got


@pytest.fixture(scope="module", params=["library", "toy"])
def answers(request, exe):
    block, tile = (GEO[0], GEO[1]) if request.param == "library" else (LC.TOY_GEOMETRY[0], LC.TOY_GEOMETRY[1])
    return request.param, _play(exe, block, tile)


def test_every_block_checked_and_every_case_reached(answers):
    tag, got = answers
    assert len(got) == 5 + 18 + (40 if tag == "toy" else 12)
    assert all(a["stage"] <= a["packed"] <= a["blocks"] and a["row"] <= a["stage"] for a in got.values())
    assert sum(a["replanned"] for a in got.values()) > 200


def test_window_fails_for_the_last_blocks_only(answers):
    a = answers[1]["band2.last_blocks"]
    assert a["packed"] == a["blocks"] and 0 < a["stage"] < a["packed"]
    assert a["window_fails"] == a["packed"] - a["stage"] and a["alloc_only"] == 0


def test_small_columns_in_the_last_rows_fail_on_the_allocation_alone(answers):
    tag, got = answers
    a = got["small_columns_last"]
    # (at the toy geometry the padding behind the codes is as long as a quarter tile: the last window still fits)
    assert (a["alloc_only"] > 0 or tag == "toy") and a["stage"] > 0 and a["window_fails"] == 0
    assert a["stage"] == a["packed"] - a["alloc_only"]


def test_no_word_where_the_vector_is_shorter_than_a_window(answers):
    tag, got = answers
    for name in ("short_vector", "short_vector.4095"):
        assert got[name]["packed"] > 0 and got[name]["stage"] == 0, name
    # at exactly one window: every block that starts at column 0 (library: all but the last, whose tile ends past the codes)
    assert got["vector.4096"]["stage"] == (got["vector.4096"]["packed"] - 1 if tag == "library" else 0)


def test_row_lengths(answers):
    tag, got = answers
    band = lambda n, odd: got["band16.len%d%s" % (n, odd)]  # noqa: E731
    for odd in ("", ".odd"):
        for n in (9, 16):
            assert band(n, odd)["row"] == 0
        if tag == "toy":  # a tile of 8 elements and 4 threads: two rows of 2, 3 or 4 elements make a uniform block
            assert all(band(n, odd)["row"] > 0 for n in (2, 3)) and band(1, odd)["row"] == 0 and band(4, "")["row"] > 0
            continue
        for n in (4, 5, 7, 8):
            assert 0 < band(n, odd)["row"] <= band(n, odd)["stage"], (n, odd)
        for n in (9, 16):
            assert band(n, odd)["stage"] > 0, (n, odd)
        for n in (1, 2, 3):  # a block of such rows has more rows than threads: no uniform flag, the general row phase
            assert band(n, odd)["stage"] > 0 and band(n, odd)["row"] == 0, (n, odd)
