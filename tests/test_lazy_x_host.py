"""The queue of x updates (ABFT_HIP_LAZY_X; abft_sparse_cg_amd/csrc/loop_state.h, LazyUpdates) without a GPU:
tests/host/lazy_x_play.cpp, built here with AddressSanitizer and UBSan, stands where abft_hip.hip stands and holds every
decision against a first-in first-out model of the updates owed to x.  The program itself ends with status 3 when
  - an update is applied twice, never, out of arrival order or with another alpha or buffer than it arrived with,
  - a calc_p -- as written or run ahead -- is told to write a buffer a queued update still reads,
  - more than depth + 1 buffers of p's length are live, or one sits in two places of the ring,
  - depth 1 ever touches the queue, or an entry that does not keep the queue leaves it filled;
this file feeds it the scripts and compares the counters between the depths."""
import itertools
import os
import re
import subprocess

import pytest

import _loop_scripts as LS
from test_loop_state_host import hexbits, lines_of  # the script vocabulary of the older fusions

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "abft_sparse_cg_amd", "csrc")
DEPTHS = (1, 2, 4)
CONFIGS = [dict(xin="1", ahead="0"), dict(xin="1", ahead="1"), dict(xin="1", ahead="2"), dict(xin="-", ahead="-")]
# what may come between two calls of the loop; every one of them must find and leave the queue as the rules say
EXTRAS = {"other": ["other"], "dot_rr": None, "spmv_q": ["spmv_q"], "p_again": ["p " + hexbits(0.25)],
          "xr_q": ["xr_q %s %s" % (hexbits(0.5), hexbits(0.125))], "spmv_again": ["spmv"]}


def _define(name):
    with open(os.path.join(CSRC, "abft_internal.h")) as f:
        return "-D%s=%s" % (name, re.search(r"#define\s+%s\s+(\w+)" % name, f.read()).group(1))


@pytest.fixture(scope="module")
def player(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lazy_x") / "lazy_x_play")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    _define("ABFT_AHEAD_DEFAULT"), _define("ABFT_X_IN_SPMV_MODES"), "-I", CSRC,
                    os.path.join(HERE, "host", "lazy_x_play.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")

    def play(text):
        """-> one row of twelve integers per `show` / `end`"""
        p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, env=env)
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        return [[int(v) for v in line.split()] for line in p.stdout.splitlines()]
    return play


def text_of(cfg, depth, steps, spec="0"):
    head = "begin %s %s %s %d" % (cfg["xin"], cfg["ahead"], spec, depth)
    return "\n".join([head] + [s for step in steps for s in step] + ["end"]) + "\n"


def with_extra(steps, at, what, rr_bits):
    extra = EXTRAS[what] or ["dot r r " + rr_bits]
    return steps[:at] + [extra] + steps[at:]


def test_header_still_needs_no_gpu():
    with open(os.path.join(CSRC, "loop_state.h")) as f:
        text = f.read()
    assert not re.search(r"#include\s*[<\"][^>\"]*(hip|abft_internal)", text)
    assert not re.search(r"\bhip[A-Z]\w*\(|\blaunch_\w+\(", text)


def test_predicted_loop_counts(player):
    """L clean iterations: L - 2 updates taken over by their SpMV at every depth, every d-th of those SpMVs a burst, the
    rest of the queue applied by the shutdown, the last pending update flushed"""
    texts, want = [], []
    for cfg in CONFIGS[:3]:
        for depth in DEPTHS:
            for L in range(3, 2 * depth + 8):
                steps, _ = lines_of("c" * L, seed=L)
                texts.append(text_of(cfg, depth, steps))
                bursts = (L - 2) // depth if depth > 1 else 0
                want.append([L - 2, 1, bursts, bursts * depth, (L - 2) % depth if depth > 1 else 0, depth])
    rows = player("".join(texts))
    assert [r[3:5] + r[8:12] for r in rows] == want


def test_every_script_at_every_depth_against_depth_1(player):
    """every script of up to 5 iterations over {clean, alpha off, beta off, alpha NaN}, and the clean six-iteration
    loop with each extra call at each place: the model holds (the program's own checks), and the counters of the older
    fusions are those of depth 1"""
    scripts = []
    for word in LS.words("cabn", 5):
        scripts.append(lines_of(word, seed=len(scripts))[0])
    base, _ = lines_of("c" * 7, seed=5)
    rr_bits = base[0][0].split()[-1]
    for what in sorted(EXTRAS):
        for at in range(1, len(base) + 1):
            scripts.append(with_extra(base, at, what, rr_bits))
    for (w1, a1), (w2, a2) in itertools.product(itertools.product(sorted(EXTRAS), (14, 15, 16, 17)), repeat=2):
        if a1 < a2:
            scripts.append(with_extra(with_extra(base, a2, w2, rr_bits), a1, w1, rr_bits))
    for cfg in CONFIGS:
        rows = {d: player("".join(text_of(cfg, d, s) for s in scripts)) for d in DEPTHS}
        assert len(rows[1]) == len(scripts)
        for d in (2, 4):
            assert [r[:8] for r in rows[d]] == [r[:8] for r in rows[1]]
        assert all(r[8:11] == [0, 0, 0] and r[11] == 1 for r in rows[1])
        if cfg["xin"] == "1":
            assert any(r[8] for r in rows[4]) and any(r[10] for r in rows[4])


def test_switches_that_force_depth_1(player):
    steps, _ = lines_of("c" * 8)
    for cfg, spec in [(dict(xin="0", ahead="-"), "0"), (dict(xin="1", ahead="1"), "1")]:
        row, = player(text_of(cfg, 4, steps, spec=spec))
        assert row[8:12] == [0, 0, 0, 1]


@pytest.mark.parametrize("fits,depth", [(0, 1), (1, 2), (2, 2), (3, 4)])
def test_spares_that_do_not_fit_lower_the_depth(player, fits, depth):
    steps, _ = lines_of("c" * 9)
    text = text_of(CONFIGS[1], 4, [["nomem %d" % fits]] + steps)
    row, = player(text)
    assert row[11] == depth and row[3:5] == [7, 1]
    assert row[8] == (7 // depth if depth > 1 else 0)
