"""What the host-scalar CG loop's scripts are made of, without the library: the arming rule of the run-ahead
(`expected`), the one-ulp nudge (`ulps`), the scripts that tests/golden/loop_state_counters.json records and the six
configurations of tools/fuzz_loop.py.  Nothing here loads libabft_hip.so or the oracle, so a test without a GPU can
import it; tests/_ahead.py re-exports `predicted`, `ulps` and `expected` (a script is what _ahead.py says it is)."""
import contextlib
import itertools
import math
import os

import numpy as np


def predicted(k):
    return [{} for _ in range(k)]


def ulps(v, k):
    for _ in range(abs(k)):
        v = float(np.nextafter(v, np.inf if k > 0 else -np.inf))
    return v


def expected(script, scalars, level):
    """(committed_p, committed_r, dropped) of a script without extra steps, from the arming rule and the alpha and beta
    the run handed in (scalars: rr0, then pw, alpha, rr_new, beta per iteration)"""
    armed, cp, cr, dropped = False, 0, 0, 0
    for j, it in enumerate(script):
        alpha, beta = scalars[1 + 4 * j + 1], scalars[1 + 4 * j + 3]
        ok_a = not it.get("alpha_ulps") and not math.isnan(alpha)
        ok_b = ok_a and not it.get("beta_ulps") and not math.isnan(beta)
        p_ahead = False
        if level == 2 and armed:  # calc_r and calc_p behind the SpMV
            if ok_a:
                cr += 1
                p_ahead = True
            else:
                dropped += 1
                armed = False
        elif level >= 1 and armed and ok_a:  # calc_p behind calc_r
            p_ahead = True
        elif not ok_a:
            armed = False
        if p_ahead:
            if ok_b:
                cp += 1
            else:
                dropped += 1
                armed = False
        else:
            armed = ok_b
    return cp, cr, dropped


# ---- the scripts of the loop-state tests (test_loop_state_host.py, test_gpu_loop_state.py) ----

SWITCHES = ["ABFT_HIP_X_IN_SPMV", "ABFT_HIP_AHEAD", "ABFT_HIP_SPECULATE"]
# as tools/fuzz_loop.py has them (test_loop_state_host.py holds the two lists together)
CONFIGS = [("x_in_spmv_off", {"ABFT_HIP_X_IN_SPMV": "0"}),
           ("ahead0", {"ABFT_HIP_X_IN_SPMV": "1", "ABFT_HIP_AHEAD": "0"}),
           ("ahead1", {"ABFT_HIP_X_IN_SPMV": "1", "ABFT_HIP_AHEAD": "1"}),
           ("ahead2", {"ABFT_HIP_X_IN_SPMV": "1", "ABFT_HIP_AHEAD": "2"}),
           ("unset", {}),
           ("speculate", {"ABFT_HIP_SPECULATE": "1"})]
COUNTERS = ["committed_p", "committed_r", "dropped", "absorbed", "flushed", "spec_commits", "spec_drops"]

# one letter per iteration: c clean, a alpha one ulp off, b beta one ulp off, n alpha NaN (the CPU scripts only: a run
# on the GPU takes its scalars from the vectors)
KINDS = {"c": {}, "a": {"alpha_ulps": 1}, "b": {"beta_ulps": 1}}
# the matrix and mode the fixture was recorded on.  tests/_matrices.py also has "one" (1 x 1), but CG on it is done after
# one iteration and every later alpha is 0 / 0: lap3 (N = 9) is the smallest on which four iterations keep finite scalars
GOLDEN_MATRIX, GOLDEN_MODE = "lap3", "none"
# the extra step of a variant goes into the script's last iteration: x downloaded between calc_xr and calc_p, r.r
# asked for again between the SpMV (and its dot(p, w)) and calc_xr
VARIANTS = {"": None, "+download": ("before_p", ("download", "x")), "+dot_rr": ("before_xr", ("dot", "r", "r"))}


def words(letters, longest):
    for k in range(1, longest + 1):
        for w in itertools.product(letters, repeat=k):
            yield "".join(w)


def script_of(name):
    """'cab+download' -> the script as tests/_ahead.py plays it"""
    word, plus, variant = name.partition("+")
    script = [dict(KINDS[c]) for c in word]
    extra = VARIANTS[plus + variant]
    if extra:
        script[-1][extra[0]] = [extra[1]]
    return script


def golden_names():
    """every script of up to 4 iterations over {clean, alpha_ulps=1, beta_ulps=1}, plain and in its two variants"""
    return [w + v for w in words("cab", 4) for v in VARIANTS]


def plain_scalars(name, scalars):
    """the scalars `_ahead.run` collected, without what the variant's extra step added: rr0, then pw, alpha, rr_new,
    beta per iteration"""
    word, plus, variant = name.partition("+")
    flat = [s for s in scalars if not isinstance(s, np.ndarray)]  # (a download is kept as the array)
    if variant == "dot_rr":
        del flat[1 + 4 * (len(word) - 1) + 2]  # behind the last iteration's pw and alpha
    assert len(flat) == 1 + 4 * len(word)
    return flat


@contextlib.contextmanager
def switched(env):
    """the environment of one configuration (the library reads the switches when a context is made)"""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
