"""The scripts of tests/golden/loop_state_counters.json (tests/_loop_scripts.py: golden_names) through the built library:
the seven counters equal the recorded ones in each of the six configurations of tools/fuzz_loop.py, what a caller can
see is the same bits in all six, and the first configuration is held against the numpy model (tests/_ahead.py:
model_holds).  The matrix is the small one the fixture was recorded on: the arming rule does not depend on n, and the
kernels' own length edges are held by test_gpu_devloop.py and test_gpu_special_values.py.  The same fixture is held
without a GPU by tests/test_loop_state_host.py."""
import json
import os

import pytest

import _ahead as H
import _loop_scripts as LS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# scripts of this many iterations, those of four split by their first iteration: every case a few seconds
CASES = [(1, ""), (2, ""), (3, ""), (4, "c"), (4, "a"), (4, "b")]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "loop_state_counters.json")) as f:
        doc = json.load(f)
    assert doc["configs"] == [n for n, _ in LS.CONFIGS] and doc["counters"] == LS.COUNTERS
    assert (doc["matrix"], doc["mode"]) == (LS.GOLDEN_MATRIX, LS.GOLDEN_MODE)
    return doc["scripts"]


def test_cases_cover_the_fixture(golden):
    names = [n for n in LS.golden_names() for length, first in CASES if len(n.partition("+")[0]) == length and n.startswith(first)]
    assert sorted(names) == sorted(golden) and len(names) == 360


@pytest.mark.parametrize("length,first", CASES)
def test_counters_and_bits(length, first, golden):
    import abft_sparse_cg_amd as amd
    mat = H.matrix(LS.GOLDEN_MATRIX)
    names = [n for n in LS.golden_names() if len(n.partition("+")[0]) == length and n.startswith(first)]
    assert len(names) == (3 * 3 ** length if not first else 3 ** length)
    for name in names:
        script = LS.script_of(name)
        base = None
        for j, (config, env) in enumerate(LS.CONFIGS):
            with LS.switched(env):
                res = H.run(amd, LS.GOLDEN_MODE, mat, script)
            got = list(res["ahead"]) + list(res["xin"]) + list(res["spec"])
            assert got == golden[name][j], (name, config, got, golden[name][j])
            if base is None:
                base = res
                plain = dict(scalars=LS.plain_scalars(name, res["scalars"]), vectors=res["vectors"])
                H.model_holds(LS.GOLDEN_MODE, mat, length, plain)
            else:
                H.same(res, base)
