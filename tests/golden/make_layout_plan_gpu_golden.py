#!/usr/bin/env python3
"""Record what the built library reports of the matrices of tests/test_gpu_layout_plan.py, on a GPU:

    python tests/golden/make_layout_plan_gpu_golden.py NOTE [OUT.json]   (default: tests/golden/layout_plan_gpu.json)

Per format, ABFT_HIP_LAYOUT and mode: abft_hip_matrix_info, abft_hip_matrix_panels, the compact and the packed
statistics.  Only data is written.  The file in the repository was recorded with the library as it stood BEFORE the
layout planner moved into csrc/layout_plan.h (ABFT_HIP_LIB pointing at the parent commit's build; NOTE, kept in the
file, says so); tests/test_gpu_layout_plan.py holds the library built from the header to it."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_layout_plan as T  # noqa: E402


def main():
    note = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "layout_plan_gpu.json")
    import abft_sparse_cg_amd as amd
    cases = {}
    for fmt, layout in T.LAYOUTS:
        for mode in T.MODES:
            os.environ.update(T.ENV, ABFT_HIP_LAYOUT=layout)
            cases[T.key(fmt, layout, mode)], _ = T.observe(amd, fmt, mode, *T.matrix())
    with open(out, "w") as f:
        f.write("{\n %s: %s,\n" % (json.dumps("note"), json.dumps(note)))
        f.write(' "cases": {\n')
        for j, (k, v) in enumerate(cases.items()):
            f.write("  %s: %s%s\n" % (json.dumps(k), json.dumps(v), "," if j + 1 < len(cases) else ""))
        f.write(" }\n}\n")
    print("%d cases -> %s" % (len(cases), out))


if __name__ == "__main__":
    main()
