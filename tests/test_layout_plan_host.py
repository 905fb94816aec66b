"""The matrix layout planner (abft_sparse_cg_amd/csrc/layout_plan.h) without a GPU: tests/host/layout_plan_play.cpp,
built here with AddressSanitizer and UBSan, stands where abft_hip.hip's create functions stand, plans the cases of
tests/_layout_cases.py and checks every plan against what a kernel relies on when it indexes these tables unchecked
(a broken invariant, or a sanitizer report, ends the program with a non-zero status).  Held besides: the answers the
planner gave before it moved into that header (tests/golden/layout_plan.json, recorded from the parent commit's text),
and the knob table in the header's comment."""
import json
import os
import re
import subprocess

import pytest

import _layout_cases as LC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "abft_sparse_cg_amd", "csrc")

GEO = LC.geometry(CSRC)


def _define(name, where="abft_internal.h"):
    with open(os.path.join(CSRC, where)) as f:
        return "-D%s=%s" % (name, re.search(r"#define\s+%s\s+(\w+)" % name, f.read()).group(1))


@pytest.fixture(scope="module")
def player(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("layout_plan") / "layout_plan_play")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    _define("ABFT_PAL_ENTRIES"), _define("ABFT_CBASE_WIDE"), _define("ABFT_PAL_SPARE", "abft_hip.hip"), "-I", CSRC,
                    os.path.join(HERE, "host", "layout_plan_play.cpp"), "-o", exe], check=True)
    # (the leak check at exit needs ptrace rights a sandbox may withhold; the program frees through destructors)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")

    def play(cases):
        """-> {case name: {key: value}}, in the order of the cases"""
        p = subprocess.run([exe], input=LC.text_of(cases, GEO), capture_output=True, text=True, timeout=300, env=env)
        assert p.returncode == 0, p.stderr[-3000:]
        got = dict(LC.parse(line) for line in p.stdout.splitlines())
        assert list(got) == [c["name"] for c in cases]
        return got
    return play


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "layout_plan.json")) as f:
        doc = json.load(f)
    assert tuple(doc["geometry"]) == GEO, "recorded at another geometry: record again (tests/golden/make_layout_plan_golden.py)"
    return doc


@pytest.fixture(scope="module")
def answers(player):
    """the fixed list, planned once (every plan has passed the invariants)"""
    return player(LC.golden_cases())


def test_header_needs_no_gpu_and_asks_no_environment():
    with open(os.path.join(CSRC, "layout_plan.h")) as f:
        text = f.read()
    assert not re.search(r"#include\s*\"", text) and not re.search(r"#include\s*<[^>]*(hip|\.h>)", text)
    assert "getenv" not in text and not re.search(r"\bhip[A-Z]\w*\(|\blaunch_\w+\(", text)
    with open(os.path.join(CSRC, "abft_hip.hip")) as f:
        hip = f.read()
    # the layout knobs are read in one function
    knob = re.compile(r"ABFT_HIP_(LAYOUT|PANEL_\w+|SWEEP_(RPT|LAG|DEBUG)|SLICE_(ROWS|LAG)|COO_PC|COO_LEAN|COMPACT_COLS|PACKED)\b")
    assert not [ln for ln in hip.splitlines() if "getenv" in ln and knob.search(ln)]
    assert len(re.findall(r"\bread_knobs\(", hip)) == 1


def test_same_answers_as_the_parent(answers, golden):
    assert list(golden["cases"]) == list(answers)
    bad = [(name, {k: (v, answers[name].get(k)) for k, v in want.items() if answers[name].get(k) != v})
           for name, want in golden["cases"].items() if answers[name] != want]
    assert not bad, (len(bad), bad[:4])


def test_issue_table_of_the_parent(golden):
    """600 x 600, 7 per row, ABFT_HIP_PANEL_WIDTH=16, as the parent's planners answered one by one: `sweep` takes the
    sweep layout (and panels would take it too), `panels` panels, `slice` the slice layout"""
    layout = {k: golden["cases"]["table.small.csr.0.%s" % k]["layout"] for k in ("panels", "sweep", "slice")}
    assert layout == dict(panels="1", sweep="2", slice="3")


def test_fixture_reaches_every_path(golden):
    """(a fixture in which nothing packs, or everything streams, would hold the planner to little)"""
    c = golden["cases"]
    count = lambda key, value: sum(1 for a in c.values() if a.get(key) == value)  # noqa: E731
    assert all(count("layout", str(k)) >= 20 for k in range(4))
    assert count("compact", "1") >= 20 and count("compact", "0") >= 10 and count("packed", "1") >= 20 and count("packed", "0") >= 10
    assert {a["rpt"] for a in c.values() if "rpt" in a} == {"2", "4", "8", "16"}
    assert {a["coo_kernel"] for a in c.values() if "coo_kernel" in a} == {"0", "1", "2"}
    assert len({a["panel_lag"] for a in c.values() if "panel_lag" in a}) >= 4
    assert len({a["panel_chunk"] for a in c.values() if "panel_chunk" in a}) >= 4
    assert len({a["rows_log2"] for a in c.values() if "rows_log2" in a}) >= 4
    # the edges by name: compact at 65535 but not 65536; packed at 16 values, not 17, and on each side of every shift
    assert (c["span.65535"]["compact"], c["span.65536"]["compact"]) == ("1", "0")
    assert c["vals.16.4095"]["packed"] == "1" and c["vals.17.100"]["packed"] == "0"
    for nv, shift in ((1, 16), (2, 15), (3, 14), (4, 14), (5, 13), (8, 13), (9, 12), (16, 12)):
        assert (c["vals.%d.%d" % (nv, (1 << shift) - 1)]["packed"], c["vals.%d.%d" % (nv, 1 << shift)]["packed"]) == ("1", "0")
    assert (c["count.255"]["layout"], c["count.256"]["layout"]) == ("2", "1")  # one-byte counts: the forced panels instead
    assert (c["segment.65500"]["layout"], c["segment.65600"]["layout"]) == ("1", "0")  # 16-bit offsets in a segment
    assert all(c["descending.%s" % k]["layout"] == "0" for k in ("panels", "sweep", "slice", "coo", "coo.constraints"))
    assert (c["gate.8MiB.csr"]["layout"], c["gate.8MiB.coo"]["layout"], c["gate.tables.coo"]["layout"]) == ("0", "0", "0")
    assert (c["gate.square.3"]["layout"], c["gate.square.1"]["layout"]) == ("2", "0")
    assert c["long_row.1025.unset"]["layout"] == "0" and c["long_row.1025.unset"]["blk"] != c["long_row.1024.unset"]["blk"]


def test_knob_table(answers):
    """every row of the table in layout_plan.h, every format and mode, where the size gates decline and where they pass"""
    cases = LC.table_cases()
    assert len(cases) == 2 * 2 * len(LC.LAYOUTS) * 2 + 2 * len(LC.LAYOUTS)
    bad = [(c["name"], answers[c["name"]]["layout"], LC.table_expectation(c["name"])) for c in cases
           if int(answers[c["name"]]["layout"]) != LC.table_expectation(c["name"])]
    assert not bad, bad


def test_table_in_the_header_is_the_table_tested():
    """the comment's rows, read back: what it says is tried and forced is what table_expectation expects"""
    with open(os.path.join(CSRC, "layout_plan.h")) as f:
        rows = re.findall(r"^//   ([a-z, ]+?)\s+\| (.+?)\s+\| (.+?)\s+\| (.+?)\s*$", f.read(), re.M)
    rows = {r[0]: r[1:] for r in rows if r[0] != "ABFT_HIP_LAYOUT"}
    assert set(rows) == {"unset, auto", "stream", "panels", "sweep", "slice", "any other string"}
    for key, cells in rows.items():
        for layout in {"unset, auto": ("unset", "auto"), "any other string": ("bogus",)}.get(key, (key,)):
            for (fmt, mode), cell in zip((("csr", 0), ("csr", 1), ("coo", 0)), cells):
                tried = [w.split()[0] for w in cell.split(",")] if cell != "-" else []
                forced = [w.split()[0] for w in cell.split(",") if w.strip().endswith("forced") or w.strip() == "slice"]
                order = [k for k in ("slice", "sweep", "panels") if k in tried]
                number = dict(slice=LC.SLICE, sweep=LC.SWEEP, panels=LC.PANELS)
                wide = number[order[0]] if order else LC.STREAM
                small = number[[k for k in order if k in forced][0]] if [k for k in order if k in forced] else LC.STREAM
                assert LC.table_expectation("table.wide.%s.%d.%s" % (fmt, mode, layout)) == wide, (key, fmt, mode)
                assert LC.table_expectation("table.small.%s.%d.%s" % (fmt, mode, layout)) == small, (key, fmt, mode)


@pytest.mark.parametrize("tag,geo", [("library", None), ("toy", LC.TOY_GEOMETRY)])
def test_invariants_on_random_small_matrices(player, tag, geo):
    got = player(LC.random_cases(geo, 420, tag))
    seen = {a["layout"] for a in got.values()}
    assert seen == {"0", "1", "2", "3"}
    if geo:  # at a tile of 8 elements and blocks of 4 rows the planner cuts, flags, packs and declines on a dozen elements
        assert sum(1 for a in got.values() if a.get("packed") == "1") > 20 and sum(1 for a in got.values() if a.get("compact") == "1") > 20


def test_fixed_list_at_the_toy_geometry(player):
    """the fixed list's small inputs again with a tile of 8 elements: a row of 7 is most of a tile, one of 1025 is 129 tiles"""
    cases = [dict(c, name="toy." + c["name"], geo=LC.TOY_GEOMETRY) for c in LC.golden_cases()
             if not c["name"].startswith(("table.wide", "table.force_stream", "gate.", "segment."))]
    assert len(cases) > 250
    got = player(cases)
    assert {a["layout"] for a in got.values()} == {"0", "1", "2", "3"}
