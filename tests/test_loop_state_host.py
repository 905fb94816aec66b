"""The decisions of the host-scalar CG loop's cross-call fusions (abft_sparse_cg_amd/csrc/loop_state.h) without a GPU:
tests/host/loop_state_play.cpp, built here with AddressSanitizer and UBSan, stands where abft_hip.hip stands and plays
scripts from stdin -- every launch succeeds, the scalars come from the script.  Held: the arming rule of the run-ahead
(tests/_loop_scripts.py: expected), the counters the library itself counted on a GPU before the state moved into that
header (tests/golden/loop_state_counters.json), and what follows from the switches alone."""
import ast
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import _loop_scripts as LS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "abft_sparse_cg_amd", "csrc")
NAN = float("nan")
IN_FLIGHT_NONE = 0


def _define(name):
    with open(os.path.join(CSRC, "abft_internal.h")) as f:
        return "-D%s=%s" % (name, re.search(r"#define\s+%s\s+(\w+)" % name, f.read()).group(1))


@pytest.fixture(scope="module")
def player(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("loop_state") / "loop_state_play")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    _define("ABFT_AHEAD_DEFAULT"), _define("ABFT_X_IN_SPMV_MODES"), "-I", CSRC,
                    os.path.join(HERE, "host", "loop_state_play.cpp"), "-o", exe], check=True)
    # (the program never touches the heap; the leak check at exit needs ptrace rights a sandbox may withhold)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")

    def play(text):
        """-> one row of eight integers per `show` / `end`: the seven counters and what is in flight"""
        p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        return [[int(v) for v in line.split()] for line in p.stdout.splitlines()]
    return play


def hexbits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def begin(env):
    """the `begin` line of a configuration of tools/fuzz_loop.py"""
    return "begin %s %s %s" % (env.get("ABFT_HIP_X_IN_SPMV", "-"), env.get("ABFT_HIP_AHEAD", "-"), env.get("ABFT_HIP_SPECULATE", "0"))


def lines_of(word, variant="", seed=0):
    """The steps of a script, one list per call, and its scalars as `expected` wants them.  Letters: c, a, b as in
    _loop_scripts.KINDS; n: the p.w handed back is a NaN, so alpha = rr / p.w is that NaN on both sides of the
    comparison, bit for bit, and only the NaN exclusion tells.  The scalars are invented (nothing is computed from
    vectors here; the decisions compare bits): finite, and finite again behind an n."""
    rng = np.random.default_rng(seed)
    rr = float(rng.random() + 0.5)
    steps, scalars = [["dot r r " + hexbits(rr)]], [rr]
    for j, kind in enumerate(word):
        last = j == len(word) - 1
        pw = NAN if kind == "n" else float(rng.random() + 0.5)
        with np.errstate(all="ignore"):
            alpha = float(np.float64(rr) / np.float64(pw))
        alpha = LS.ulps(alpha, 1 if kind == "a" else 0)
        rr_new = float(rr * (rng.random() * 0.5 + 0.25))
        beta = LS.ulps(rr_new / rr, 1 if kind == "b" else 0)
        steps += [["spmv"], ["dot p w " + hexbits(pw)]]
        if last and variant == "+dot_rr":
            steps.append(["dot r r " + hexbits(rr)])  # (the same vector summed again: the same bits)
        steps.append(["xr %s %s" % (hexbits(alpha), hexbits(rr_new))])
        if last and variant == "+download":
            steps.append(["other"])
        steps.append(["p " + hexbits(beta)])
        scalars += [pw, alpha, rr_new, beta]
        rr = rr_new
    return steps, scalars


def text_of(env, steps):
    return "\n".join([begin(env)] + [s for step in steps for s in step] + ["end"]) + "\n"


def test_configurations_are_those_of_the_fuzzer():
    with open(os.path.join(ROOT, "tools", "fuzz_loop.py")) as f:
        tree = ast.parse(f.read())
    found = {t.id: ast.literal_eval(n.value) for n in tree.body if isinstance(n, ast.Assign) for t in n.targets
             if isinstance(t, ast.Name) and t.id in ("CONFIGS", "COUNTERS", "SWITCHES")}
    assert found == dict(CONFIGS=LS.CONFIGS, COUNTERS=LS.COUNTERS, SWITCHES=LS.SWITCHES)


def test_header_needs_no_gpu():
    with open(os.path.join(CSRC, "loop_state.h")) as f:
        text = f.read()
    assert not re.search(r"#include\s*[<\"][^>\"]*(hip|abft_internal)", text)
    assert not re.search(r"\bhip[A-Z]\w*\(|\blaunch_\w+\(", text)


def test_arming_rule(player):
    """every script of 1 to 5 iterations over {clean, alpha one ulp off, beta one ulp off, alpha NaN} at levels 0, 1, 2"""
    words = list(LS.words("cabn", 5))
    assert len(words) == 1364
    cases = []
    for level in (0, 1, 2):
        env = {"ABFT_HIP_X_IN_SPMV": "1", "ABFT_HIP_AHEAD": str(level)}
        for k, word in enumerate(words):
            steps, scalars = lines_of(word, seed=k)
            script = [dict(LS.KINDS.get(c, {})) for c in word]
            cases.append((word, level, text_of(env, steps), LS.expected(script, scalars, level)))
    rows = player("".join(c[2] for c in cases))
    assert len(rows) == len(cases)
    for (word, level, _, want), row in zip(cases, rows):
        assert tuple(row[:3]) == want, (word, level, row)
        assert row[5:7] == [0, 0], (word, level, row)
        assert level or row[:3] == [0, 0, 0]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "loop_state_counters.json")) as f:
        doc = json.load(f)
    assert doc["configs"] == [n for n, _ in LS.CONFIGS] and doc["counters"] == LS.COUNTERS
    assert (doc["matrix"], doc["mode"]) == (LS.GOLDEN_MATRIX, LS.GOLDEN_MODE)
    assert sorted(doc["scripts"]) == sorted(LS.golden_names()) and len(doc["scripts"]) == 360
    return doc


def test_counters_of_the_library(player, golden):
    """what the library counted on the GPU, script by script and configuration by configuration"""
    cases = []
    for k, name in enumerate(LS.golden_names()):
        word, plus, variant = name.partition("+")
        steps, _ = lines_of(word, plus + variant, seed=k)
        steps.append(["other"])  # (_ahead.run downloads the vectors before it reads the counters)
        for j, (_, env) in enumerate(LS.CONFIGS):
            cases.append((name, j, text_of(env, steps)))
    rows = player("".join(c[2] for c in cases))
    assert len(rows) == len(cases)
    bad = [(name, LS.CONFIGS[j][0], row[:7], golden["scripts"][name][j]) for (name, j, _), row in zip(cases, rows)
           if row[:7] != golden["scripts"][name][j]]
    assert not bad, (len(bad), bad[:8])


def test_fixture_reaches_every_counter(golden):
    """(a fixture of zeros would hold anything to nothing)"""
    sums = np.array([golden["scripts"][n] for n in LS.golden_names()]).sum(axis=0)  # [configuration][counter]
    by = dict(zip(golden["configs"], sums.tolist()))
    assert by["x_in_spmv_off"] == [0] * 7
    assert by["ahead0"][:3] == [0, 0, 0] and by["ahead0"][3] > 0 and by["ahead0"][4] > 0
    assert by["ahead1"][0] > 0 and by["ahead1"][1] == 0 and by["ahead1"][2] > 0
    assert all(v > 0 for v in by["ahead2"][:5])
    assert by["unset"] == by["ahead1"]  # (mode none: on by default, at the default level)
    assert by["speculate"][:5] == [0] * 5 and by["speculate"][5] > 0 and by["speculate"][6] > 0


def test_switches_alone(player):
    """speculation on: nothing of the run-ahead or of x-in-SpMV ever counts; x-in-SpMV off: nothing counts at all"""
    words = list(LS.words("cabn", 4))
    spec = [text_of({"ABFT_HIP_SPECULATE": "1", "ABFT_HIP_AHEAD": a, **x}, lines_of(w, v, seed=k)[0])
            for k, w in enumerate(words) for v in LS.VARIANTS for a in "12" for x in ({}, {"ABFT_HIP_X_IN_SPMV": "1"})]
    rows = player("".join(spec))
    assert len(rows) == len(spec) and all(row[:5] == [0] * 5 for row in rows)
    assert any(row[5] for row in rows) and any(row[6] for row in rows)
    off = [text_of({"ABFT_HIP_X_IN_SPMV": "0", "ABFT_HIP_AHEAD": a}, lines_of(w, v, seed=k)[0])
           for k, w in enumerate(words) for v in LS.VARIANTS for a in "012"]
    rows = player("".join(off))
    assert len(rows) == len(off) and all(row == [0] * 7 + [IN_FLIGHT_NONE] for row in rows)


def test_other_entry_drops_what_is_in_flight(player):
    """an entry point with default flags, wherever something is in flight: exactly one item dropped, nothing left"""
    seen = set()
    for name, env in LS.CONFIGS[2:4] + LS.CONFIGS[5:]:
        steps, _ = lines_of("ccccc")
        watched = player("\n".join([begin(env)] + [s for step in steps for s in step + ["show"]]) + "\n")
        assert len(watched) == len(steps)
        for k, row in enumerate(watched):
            if row[7] == IN_FLIGHT_NONE:
                continue
            seen.add(row[7])
            (after,) = player("\n".join([begin(env)] + [s for step in steps[:k + 1] for s in step] + ["other", "end"]) + "\n")
            assert after[7] == IN_FLIGHT_NONE, (name, k, after)
            assert after[2] + after[6] == row[2] + row[6] + 1, (name, k, row, after)  # dropped + spec_drops
            assert after[:2] + after[5:6] == row[:2] + row[5:6], (name, k, row, after)  # no commit
    assert seen == {1, 2, 3, 4}  # every value of InFlight but None
