"""The cases tests/host/layout_plan_play.cpp is fed (tests/host/layout_plan_io.h has the format): the fixed list whose
answers tests/golden/layout_plan.json records from the parent commit's planner, the knob table of layout_plan.h, and
the seeded small matrices the invariants run on at the library's geometry and at a toy one."""
import re

LIBRARY_GEOMETRY = None  # filled by geometry(): block, CSR tile, COO tile, panel rows, sweep elements per thread, segments per block
TOY_GEOMETRY = (4, 8, 8, 4, 8, 16)

NONE, CONSTRAINTS, SECDED = 0, 1, 5
LAYOUTS = (None, "auto", "stream", "panels", "sweep", "slice", "bogus")  # ABFT_HIP_LAYOUT (None: unset; "bogus": any other string)
STREAM, PANELS, SWEEP, SLICE = 0, 1, 2, 3  # what abft_hip_matrix_info reports

# 600 x 600, 7 ascending random columns per row, three distinct values; with 16-entry panels every layout takes it
SMALL = "rand 600 600 7 1 3"
W16 = {"ABFT_HIP_PANEL_WIDTH": "16"}
# the gathered vector just over 8 MiB (2^20 + 1 entries), scattered: what the `auto` gates let through
WIDE = {"csr": "rand 4096 1048577 40 5 3", "coo": "rand 1048577 4096 1 5 3 -1 8"}
GROUPS3 = "rand 5000 5000 5 2 3"  # three output groups in the panel layout


def geometry(csrc):
    """the sizes abft_hip.hip hands the planner, from abft_internal.h"""
    with open(csrc + "/abft_internal.h") as f:
        text = f.read()

    def macro(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    block = int(re.search(r"constexpr int ABFT_BLOCK = (\d+);", text).group(1))
    return (block, block * macro("ABFT_CFG_CSR_EPT"), block * macro("ABFT_CFG_COO_EPT"), 256 * macro("ABFT_CFG_PANEL_RPT"),
            macro("ABFT_CFG_SWEEP_EPT"), 4 * block)


def case(name, gen, fmt="csr", mode=NONE, env=None, layout=None, stream=False, cus=256, geo=None):
    env = dict(env or {})
    if layout is not None:
        env["ABFT_HIP_LAYOUT"] = layout
    return dict(name=name, gen=gen, fmt=fmt, mode=mode, env=env, stream=stream, cus=cus, geo=geo)


def text_of(cases, library_geometry):
    out = []
    for c in cases:
        out.append("case %s" % c["name"])
        out.append("geo " + " ".join(str(v) for v in (c["geo"] or library_geometry)))
        out.append("fmt %s" % c["fmt"])
        out.append("mode %d" % c["mode"])
        out.append("stream %d" % c["stream"])
        out.append("cus %d" % c["cus"])
        out += ["env %s %s" % kv for kv in sorted(c["env"].items())]
        out.append("gen " + c["gen"])
        out.append("run")
    return "\n".join(out) + "\n"


def parse(line):
    """a line of the program, NAME key=value ... -> (NAME, {key: value})"""
    name, *fields = line.split()
    return name, dict(f.split("=", 1) for f in fields)


def lname(layout):
    return "unset" if layout is None else layout


def table_cases():
    """every ABFT_HIP_LAYOUT x format x mode, where the size gates decline (SMALL) and where they pass (WIDE)"""
    out = []
    for fmt in ("csr", "coo"):
        for mode in (NONE, CONSTRAINTS):
            for layout in LAYOUTS:
                out.append(case("table.small.%s.%d.%s" % (fmt, mode, lname(layout)), SMALL, fmt, mode, W16, layout))
                out.append(case("table.wide.%s.%d.%s" % (fmt, mode, lname(layout)), WIDE[fmt], fmt, mode, None, layout))
    for mode in (NONE, CONSTRAINTS):
        for layout in LAYOUTS:
            out.append(case("table.force_stream.csr.%d.%s" % (mode, lname(layout)), WIDE["csr"], "csr", mode, None, layout, stream=True))
    return out


def table_expectation(name):
    """the layout a table case ends in, by the table of layout_plan.h (small: the size gates decline; wide: they pass)"""
    _, size, fmt, mode, layout = name.split(".")
    mode = int(mode)
    if size == "force_stream" or layout == "stream":
        return STREAM
    if fmt == "coo":
        forced = layout in ("panels", "sweep")
        return PANELS if forced or size == "wide" else STREAM
    if mode == CONSTRAINTS:
        tried = layout in ("unset", "auto", "sweep")
        return SWEEP if tried and (layout == "sweep" or size == "wide") else STREAM
    if layout == "slice":
        return SLICE
    if layout == "sweep":
        return SWEEP
    if layout == "panels":
        return PANELS
    if size == "small":
        return STREAM
    return SWEEP if layout in ("unset", "auto") else PANELS  # (any other string: panels on auto)


def golden_cases():
    out = table_cases()
    add = lambda *a, **k: out.append(case(*a, **k))  # noqa: E731
    for mode in (NONE, SECDED):
        add("force_stream.small.%d" % mode, SMALL, "csr", mode, W16, "sweep", stream=True)
    # geometry knobs
    for layout in ("panels", "sweep", "slice"):
        for w in ("0", "1", "100", "599", "600", "100000"):
            add("width.%s.%s" % (layout, w), SMALL, "csr", NONE, {"ABFT_HIP_PANEL_WIDTH": w}, layout)
    add("width.coo.100", SMALL, "coo", NONE, {"ABFT_HIP_PANEL_WIDTH": "100"}, "panels")
    for rpt in ("2", "4", "8", "16", "3"):
        for mode in (NONE, CONSTRAINTS):
            add("rpt.%s.%d" % (rpt, mode), GROUPS3, "csr", mode, dict(W16, ABFT_HIP_SWEEP_RPT=rpt, ABFT_HIP_PANEL_WIDTH="700"), "sweep")
    for cus in (1, 2, 256):  # (which rows-per-thread the occupancy picks, and grids of several rounds)
        add("sweep.cus%d" % cus, GROUPS3, "csr", NONE, {"ABFT_HIP_PANEL_WIDTH": "700"}, "sweep", cus=cus)
        add("slice.cus%d" % cus, GROUPS3, "csr", NONE, {"ABFT_HIP_PANEL_WIDTH": "700"}, "slice", cus=cus)
    for rows in ("16", "64", "256", "2048", "100", "4096"):
        add("slice_rows.%s" % rows, GROUPS3, "csr", NONE, {"ABFT_HIP_PANEL_WIDTH": "700", "ABFT_HIP_SLICE_ROWS": rows}, "slice")
    for lag in ("0", "5", "-3"):
        add("sweep_lag.%s" % lag, SMALL, "csr", NONE, dict(W16, ABFT_HIP_SWEEP_LAG=lag), "sweep")
        add("slice_lag.%s" % lag, SMALL, "csr", NONE, dict(W16, ABFT_HIP_SLICE_LAG=lag), "slice")
    for fmt in ("csr", "coo"):
        for mode in (NONE, CONSTRAINTS) if fmt == "coo" else (NONE,):
            for cus in (1, 256):
                base = {"ABFT_HIP_PANEL_WIDTH": "700"}
                tag = "%s.%d.cus%d" % (fmt, mode, cus)
                add("panels.%s" % tag, GROUPS3, fmt, mode, base, "panels", cus=cus)
                for v in ("0", "1", "3"):
                    add("chunk.%s.%s" % (v, tag), GROUPS3, fmt, mode, dict(base, ABFT_HIP_PANEL_CHUNK=v), "panels", cus=cus)
                    add("lag.%s.%s" % (v, tag), GROUPS3, fmt, mode, dict(base, ABFT_HIP_PANEL_LAG=v), "panels", cus=cus)
                for v in ("1", "2", "5", "0"):
                    add("grid.%s.%s" % (v, tag), GROUPS3, fmt, mode, dict(base, ABFT_HIP_PANEL_GRID=v), "panels", cus=cus)
                add("grid_chunk.%s" % tag, GROUPS3, fmt, mode, dict(base, ABFT_HIP_PANEL_GRID="2", ABFT_HIP_PANEL_CHUNK="0"), "panels", cus=cus)
                add("lag_chunk.%s" % tag, GROUPS3, fmt, mode, dict(base, ABFT_HIP_PANEL_LAG="1", ABFT_HIP_PANEL_CHUNK="2"), "panels", cus=cus)
                add("xpf.%s" % tag, GROUPS3, fmt, mode, dict(base, ABFT_HIP_PANEL_XPF="3"), "panels", cus=cus)
    for mode in (NONE, CONSTRAINTS):
        for pc, lean in (("1", None), (None, "1"), ("1", "1"), ("0", "1"), ("0", "0")):
            env = {"ABFT_HIP_PANEL_WIDTH": "700"}
            if pc is not None:
                env["ABFT_HIP_COO_PC"] = pc
            if lean is not None:
                env["ABFT_HIP_COO_LEAN"] = lean
            for cus in (1, 256):
                add("coo_kernel.pc%s.lean%s.%d.cus%d" % (pc, lean, mode, cus), GROUPS3, "coo", mode, env, "panels", cus=cus)
    for co, pk in (("0", None), (None, "0"), ("0", "0"), ("1", "1")):
        env = {}
        if co is not None:
            env["ABFT_HIP_COMPACT_COLS"] = co
        if pk is not None:
            env["ABFT_HIP_PACKED"] = pk
        add("stream.compact%s.packed%s" % (co, pk), SMALL, "csr", NONE, env)
    add("stream.secded", SMALL, "csr", SECDED)
    # edges
    for fmt in ("csr", "coo"):
        for mode in (NONE, CONSTRAINTS):
            for layout in (None, "sweep", "slice"):
                add("empty50.%s.%d.%s" % (fmt, mode, lname(layout)), "empty 50", fmt, mode, W16, layout)
            add("empty0.%s.%d" % (fmt, mode), "empty 0", fmt, mode, W16, "sweep")
            add("trailing.%s.%d" % (fmt, mode), "trailing 600 7 50 3", fmt, mode)
            for layout in ("panels", "sweep", "slice"):
                add("trailing.%s.%d.%s" % (fmt, mode, layout), "trailing 600 7 50 3", fmt, mode, W16, layout)
    for layout in (None, "panels", "sweep", "slice"):
        add("one_row.%s" % lname(layout), "rand 1 600 7 1 3", "csr", NONE, W16, layout)
        add("one_row.coo.%s" % lname(layout), "rand 1 600 7 1 3", "coo", NONE, W16, layout)
        for n in (1024, 1025, 1026, 2049):  # a row at, one past and two past a CSR tile; more than two tiles
            add("long_row.%d.%s" % (n, lname(layout)), "longrow 40 40 3 %d" % n, "csr", NONE, {"ABFT_HIP_PANEL_WIDTH": "8"}, layout)
    add("long_row.1025.secded", "longrow 40 40 3 1025", "csr", SECDED)
    add("long_row.1025.coo", "longrow 40 40 3 1025", "coo", NONE)
    add("uniform", "uniform 600 5 7", "csr", NONE)
    add("uniform.broken", "uniform 600 5 7 300 3", "csr", NONE)
    add("uniform.one_long", "uniform 600 5 7 300 9", "csr", NONE)
    add("uniform.257_rows", "uniform 771 1 0", "csr", NONE)
    add("band", "band 600 3 2", "csr", NONE)
    add("band.coo", "band 600 3 2", "coo", CONSTRAINTS)
    for layout in ("panels", "sweep", "slice"):  # a row whose columns descend: every panel-type planner declines
        add("descending.%s" % layout, SMALL + " 17", "csr", NONE, W16, layout)
    add("descending.coo", "revrand 600 600 7 1 3", "coo", NONE, W16, "panels")
    add("descending.coo.constraints", "revrand 600 600 7 1 3", "coo", CONSTRAINTS, W16, "sweep")
    # the field limits: 255 elements of a row in one panel (sweep, else the forced panels), 65535 in a segment
    for n in (255, 256):
        add("count.%d" % n, "longrow 40 40 3 %d" % n, "csr", NONE, {"ABFT_HIP_PANEL_WIDTH": "64"}, "sweep")
    for k in (655, 656):
        add("segment.%d" % (k * 100), "rand 100 100 %d 1 3" % k, "csr", NONE, None, "panels")
    # compact columns: a block spanning 65535 and 65536 columns; packed codes: 16 and 17 values, spans at each shift
    for hi in (65535, 65536):
        add("span.%d" % hi, "span %d" % hi, "csr", NONE)
    for nv, shift in ((1, 16), (2, 15), (3, 14), (4, 14), (5, 13), (8, 13), (9, 12), (16, 12)):
        for hi in ((1 << shift) - 1, 1 << shift):
            add("vals.%d.%d" % (nv, hi), "vals %d %d" % (nv, hi), "csr", NONE)
    add("vals.17.100", "vals 17 100", "csr", NONE)
    # the `auto` size gates: a gathered vector of 8 MiB exactly stays streaming; too few elements per row for the tables
    add("gate.8MiB.csr", "rand 4096 1048576 40 5 3", "csr", NONE)
    add("gate.8MiB.coo", "rand 1048576 4096 1 5 3 -1 8", "coo", NONE)
    add("gate.square.3", "rand 1048577 1048577 3 7 3", "csr", NONE)
    add("gate.square.1", "rand 1048577 1048577 1 7 3", "csr", NONE)
    add("gate.tables.coo", "rand 1048577 4096 1 5 3 -1 128", "coo", NONE)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def random_cases(geo, count, tag):
    """seeded small matrices over every layout, format and mode (golden-free: the invariants alone)"""
    out = []
    for seed in range(count):
        layout = LAYOUTS[seed % len(LAYOUTS)]
        fmt = "coo" if seed % 3 == 2 else "csr"
        mode = (NONE, NONE, CONSTRAINTS, SECDED)[(seed // 3) % 4]
        n_out = 1 + seed % 37
        n_in = n_out if fmt == "coo" else 1 + (seed * 7) % 41
        env = {"ABFT_HIP_PANEL_WIDTH": str(1 + seed % 9)}
        if seed % 5 == 0:
            env["ABFT_HIP_SWEEP_RPT"] = ("2", "4", "8", "16")[(seed // 5) % 4]
        if seed % 11 == 0:
            env["ABFT_HIP_SLICE_ROWS"] = "16"
        out.append(case("random.%s.%d" % (tag, seed), "tiny %d %d %d %d %d" % (n_out, n_in, 1 + seed % 13, seed, seed % 4), fmt, mode, env,
                        layout, cus=1 + seed % 3, geo=geo))
    return out
