#!/usr/bin/env python3
"""Record the counters of the host-scalar CG loop's cross-call fusions, as the built library counts them on a GPU:

    python tests/golden/make_loop_state_golden.py [OUT.json]      (default: tests/golden/loop_state_counters.json)

Every script of tests/_loop_scripts.py (golden_names: up to 4 iterations over {clean, alpha one ulp off, beta one ulp
off}, plain, with x downloaded between calc_xr and calc_p, and with dot(r, r) between the SpMV and calc_xr) is played
through tests/_ahead.py: run on the matrix GOLDEN_MATRIX in each of the six configurations of tools/fuzz_loop.py.
Written: committed_p, committed_r, dropped, absorbed, flushed, spec_commits, spec_drops per script and configuration.
Only data is written.  The file in the repository was recorded with the library as it stood BEFORE the loop's state
moved into csrc/loop_state.h; tests/test_loop_state_host.py holds the header's decisions to it without a GPU,
tests/test_gpu_loop_state.py the library built from it."""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _loop_scripts as LS  # noqa: E402


def record():
    import abft_sparse_cg_amd as amd
    import _ahead
    mat = _ahead.matrix(LS.GOLDEN_MATRIX)
    counters = {}
    for name in LS.golden_names():
        rows = []
        for _, env in LS.CONFIGS:
            with LS.switched(env):
                res = _ahead.run(amd, LS.GOLDEN_MODE, mat, LS.script_of(name))
            # what the replay without a GPU relies on: no NaN anywhere, and r.r asked for twice is the same bits
            flat = LS.plain_scalars(name, res["scalars"])
            assert all(math.isfinite(s) and s != 0.0 for s in flat), (name, flat)
            assert not res["events"], (name, res["events"])
            if name.endswith("+dot_rr"):
                k = len(flat) // 4
                again = [s for s in res["scalars"] if isinstance(s, float)][1 + 4 * (k - 1) + 2]
                assert again.hex() == flat[1 + 4 * (k - 2) + 2 if k > 1 else 0].hex(), (name, again)
            rows.append(list(res["ahead"]) + list(res["xin"]) + list(res["spec"]))
        counters[name] = rows
    return dict(matrix=LS.GOLDEN_MATRIX, mode=LS.GOLDEN_MODE, configs=[n for n, _ in LS.CONFIGS], counters=LS.COUNTERS,
                scripts=counters)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "loop_state_counters.json")
    doc = record()
    with open(out, "w") as f:
        f.write("{\n")
        for k in ("matrix", "mode", "configs", "counters"):
            f.write(" %s: %s,\n" % (json.dumps(k), json.dumps(doc[k])))
        f.write(' "scripts": {\n')
        names = list(doc["scripts"])
        for j, name in enumerate(names):
            f.write("  %s: %s%s\n" % (json.dumps(name), json.dumps(doc["scripts"][name]), "," if j + 1 < len(names) else ""))
        f.write(" }\n}\n")
    print("%d scripts x %d configurations -> %s" % (len(doc["scripts"]), len(doc["configs"]), out))


if __name__ == "__main__":
    main()
