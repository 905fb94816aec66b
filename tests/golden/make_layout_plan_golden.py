#!/usr/bin/env python3
"""Record what a planner answers on the fixed cases of tests/_layout_cases.py (golden_cases):

    python tests/golden/make_layout_plan_golden.py PLAYER NOTE [OUT.json]   (default: tests/golden/layout_plan.json)

PLAYER is a program that reads the cases of tests/host/layout_plan_io.h on stdin and prints one line per case, as
tests/host/layout_plan_play.cpp does.  Only data is written: per case the chosen layout, the scalars and a digest of
every array.  The file in the repository was recorded from the planner as it stood in abft_hip.hip BEFORE it moved
into csrc/layout_plan.h (NOTE, kept in the file, says from which commit and how); tests/test_layout_plan_host.py
holds the header to it."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _layout_cases as LC  # noqa: E402


def main():
    player, note = sys.argv[1], sys.argv[2]
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(HERE, "layout_plan.json")
    geo = LC.geometry(os.path.join(ROOT, "abft_sparse_cg_amd", "csrc"))
    cases = LC.golden_cases()
    p = subprocess.run([player], input=LC.text_of(cases, geo), capture_output=True, text=True, check=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    answers = dict(LC.parse(line) for line in p.stdout.splitlines())
    assert list(answers) == [c["name"] for c in cases]
    with open(out, "w") as f:
        f.write("{\n %s: %s,\n %s: %s,\n" % (json.dumps("note"), json.dumps(note), json.dumps("geometry"), json.dumps(list(geo))))
        f.write(' "cases": {\n')
        for j, c in enumerate(cases):
            f.write("  %s: %s%s\n" % (json.dumps(c["name"]), json.dumps(answers[c["name"]]), "," if j + 1 < len(cases) else ""))
        f.write(" }\n}\n")
    print("%d cases -> %s" % (len(cases), out))


if __name__ == "__main__":
    main()
