"""The packed family of tools/fuzz_parity.py (tools/fuzz_gen.py), checked on the CPU: 300 seeds
classified with the generator's own model -- every class the campaign's summary counts must be
reached by at least one eligible case in ten, so that a 20-second run on the GPU cannot miss one --
its "every block packs" / "no block packs" marks against a plain evaluation of the two one-sided
rules, and the oracle on every mode-none case (no case of that mode is left out of the comparison).
The library is not imported.

The CG-loop family (fuzz_gen.loop_case, played by tools/fuzz_loop.py): same seed same case, well-formed scripts, and --
over exactly the seeds tests/test_gpu_fuzz.py plays -- the coverage conditions on its structural tags, and its injects
against the oracle alone."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_gen  # noqa: E402
from _oracle import COO, CSR, OracleMatrix  # noqa: E402

SEEDS = range(1, 301)


@pytest.fixture(scope="module")
def cases():
    return [fuzz_gen.packed_case(s) for s in SEEDS]


def test_generator_does_not_need_the_library():
    with open(fuzz_gen.__file__) as f:
        assert "abft_sparse_cg_amd" not in f.read()


def test_palette_pool_size_is_the_sources():
    """tests/test_gpu_packed_replan.py fills the pool: its capacity is ABFT_PAL_SPARE of abft_hip.hip"""
    import re

    import test_gpu_packed_replan
    with open(os.path.join(ROOT, "abft_sparse_cg_amd", "csrc", "abft_hip.hip")) as f:
        m = re.search(r"#define\s+ABFT_PAL_SPARE\s+(\d+)u?", f.read())
    assert m and int(m.group(1)) == test_gpu_packed_replan.PAL_SPARE


def test_same_seed_same_case():
    a, b = fuzz_gen.packed_case(17), fuzz_gen.packed_case(17)
    assert np.array_equal(a.cols, b.cols) and np.array_equal(a.vals.view(np.uint64), b.vals.view(np.uint64))
    assert a.flips == b.flips and a.checks == b.checks and a.classes == b.classes


def test_every_class_in_one_eligible_case_in_ten(cases):
    for cls in fuzz_gen.CLASSES:
        eligible = [c for c in cases if cls in c.eligible]
        have = [c for c in eligible if cls in c.classes]
        assert len(eligible) >= 60, (cls, len(eligible))
        assert len(have) >= 0.1 * len(eligible), (cls, len(have), len(eligible))
    # mode none on CSR carries most cases; the other modes and COO a minority that is there
    main = [c for c in cases if (c.fmt, c.mode) == (CSR, "none")]
    assert 0.6 * len(cases) <= len(main) <= 0.9 * len(cases)
    assert any(c.fmt == COO for c in cases)
    assert {c.layout for c in main} == {"stream", "auto"}
    assert max(len(c.flips) for c in main) >= 30


def test_cases_are_well_formed(cases):
    for c in cases:
        nnz = len(c.vals)
        assert len(c.cols) == len(c.rows) == nnz
        key = c.rows.astype(np.int64) * c.n_in + c.cols
        assert np.all(np.diff(key) > 0), c.seed  # sorted by (row, column), no duplicates
        if nnz:
            assert c.rows.max() < c.n and c.cols.max() < c.n_in
        assert len(c.x) == c.n_in
        assert c.checks == sorted(set(c.checks)) and (not c.flips or c.checks[-1] == len(c.flips))
        width = 96 if c.fmt == CSR else 128
        for i, bits, _ in c.flips:
            assert 0 <= i < nnz and 1 <= len(bits) <= 32 and all(0 <= b < width for b in bits), (c.seed, i, bits)
        if c.interior:
            assert 0 <= c.interior[0] <= c.interior[1] <= c.n
        if c.spmm_k:
            assert c.fmt == CSR and c.n == c.n_in and c.index_base == 0 and c.layout == "stream"


def _rule_all(c, window):
    """no row longer than a tile, and every stretch of `window` elements starting at a multiple of the
    tile holds at most 16 patterns over fewer than 2^12 columns (every window of a tile lies in one)"""
    tile = fuzz_gen.TILE
    if len(c.vals) and np.diff(c.rowptr).max() > tile:
        return False
    vb = c.vals.view(np.uint64).tolist()
    cols = c.cols.tolist()
    for j in range(0, len(vb), tile):
        if len(set(vb[j:j + window])) > 16 or max(cols[j:j + window]) - min(cols[j:j + window]) >= 4096:
            return False
    return True


def _rule_none(c):
    """every single row holds more than 16 patterns or spans 65536 columns or more"""
    vb = c.vals.view(np.uint64).tolist()
    cols = c.cols.tolist()
    if not len(vb):
        return False
    for r in range(c.n):
        a, b = int(c.rowptr[r]), int(c.rowptr[r + 1])
        if a == b or not (len(set(vb[a:b])) > 16 or max(cols[a:b]) - min(cols[a:b]) >= 65536):
            return False
    return True


def test_marks_agree_with_the_rules(cases):
    seen = {"all": 0, "none": 0, None: 0}
    for c in cases:
        if (c.fmt, c.mode) != (CSR, "none"):
            assert c.mark is None
            continue
        want = "all" if _rule_all(c, fuzz_gen.WINDOW) else "none" if _rule_none(c) else None
        assert c.mark == want, (c.seed, c.kind, c.mark, want)
        seen[c.mark] += 1
        if c.mark == "all" and 0 < len(c.vals) <= 30000:  # the rule as the issue states it: EVERY window of a tile
            w = fuzz_gen.TILE
            v = np.lib.stride_tricks.sliding_window_view(c.vals.view(np.uint64), min(w, len(c.vals)))
            k = np.lib.stride_tricks.sliding_window_view(c.cols.astype(np.int64), min(w, len(c.vals)))
            assert int((k.max(axis=1) - k.min(axis=1)).max()) < 4096
            assert int((np.diff(np.sort(v, axis=1), axis=1) != 0).sum(axis=1).max()) + 1 <= 16
    assert seen["all"] >= 30 and seen["none"] >= 15 and seen[None] >= 30, seen


def test_values_hold_special_patterns_and_every_cardinality(cases):
    pats = set()
    counts = set()
    for c in cases:
        if (c.fmt, c.mode) == (CSR, "none"):
            pats |= set(np.unique(c.vals.view(np.uint64)).tolist()) & set(fuzz_gen.SPECIALS.tolist())
            counts |= {s[2] for s in c.segs}
    assert pats == set(fuzz_gen.SPECIALS.tolist())  # +-0.0, +-inf, subnormals, NaNs of several payloads and signs
    assert counts >= set(fuzz_gen.M_CHOICES)


def test_oracle_takes_every_mode_none_case_without_events(cases):
    """mode none detects nothing: whatever the flips, the oracle reports no event, so the campaign may
    skip no case of that mode"""
    for c in cases:
        if (c.fmt, c.mode) != (CSR, "none"):
            continue
        o = OracleMatrix(CSR, "none", c.cols, c.rows, c.vals, c.n, n_in=c.n_in, index_base=c.index_base)
        for stage in range(2):
            y = o.spmv(c.x)
            assert y.shape == (c.n,)
            assert o.events() == ([], False), (c.seed, stage)
            # a row of finite values times finite x entries inside n_in gives a finite or overflowed sum, never NaN
            if stage == 0 and len(c.vals):
                bad_el = ~np.isfinite(c.vals) | ~np.isfinite(c.x[c.cols])
                bad_row = np.zeros(c.n, bool)
                bad_row[c.rows[bad_el]] = True
                assert not np.isnan(y[~bad_row]).any(), c.seed
            for i, bits, _ in c.flips:
                o.inject(i, bits)
        o.close()


def test_other_modes_are_not_mostly_skipped(cases):
    """The campaign stops comparing a case once the oracle reports a fatal event, and its short run
    fails if that happens to more than half of the packed family's cases outside CSR mode none.
    Measured here from the oracle alone: the share of such cases, which must stay below that cap with
    room to spare.  (The first family, by the same measurement over seeds 100000..100299: 67 of 300
    cases end at a fatal event, 22 %.)"""
    other = [c for c in cases if (c.fmt, c.mode) != (CSR, "none")]
    assert len(other) >= 30
    fatal = 0
    for c in other:
        o = OracleMatrix(c.fmt, c.mode, c.cols, c.rows, c.vals, c.n, n_in=c.n_in, index_base=c.index_base)
        for i, bits, _ in c.flips:
            o.inject(i, bits)
        for _ in range(2):
            o.spmv(c.x)
            if o.events()[1]:
                fatal += 1
                break
        o.close()
    assert fatal <= 0.35 * len(other), (fatal, len(other))


# ---------------------------------------------------------------- the CG-loop family --

@pytest.fixture(scope="module")
def loops():
    return [fuzz_gen.loop_case(s) for s in fuzz_gen.LOOP_SEEDS]


def test_loop_blocks_cover_the_seed_range():
    assert len(fuzz_gen.LOOP_SEEDS) % fuzz_gen.LOOP_BLOCK == 0


def test_loop_same_seed_same_case():
    a, b = fuzz_gen.loop_case(23), fuzz_gen.loop_case(23)
    assert (a.mode, a.solves, a.script, a.iterations, a.tags) == (b.mode, b.solves, b.script, b.iterations, b.tags)
    assert fuzz_gen.loop_case(24).script != a.script


def test_loop_cases_are_well_formed(loops):
    for c in loops:
        assert c.mode in fuzz_gen.MODES and 1 <= len(c.solves) <= 3
        lengths = [v["n"] for v in c.solves]
        assert len(set(lengths)) == len(lengths) or (len(lengths) == 2 and lengths[0] == lengths[1]), c.seed
        for v in c.solves:
            cols, rows, vals, n = fuzz_gen.loop_matrix(v["spec"])
            assert (n, len(vals)) == (v["n"], v["nnz"]) and 1 <= n <= 3001
            assert v["scale"] in [0] + fuzz_gen.LOOP_SCALES
        # every solve's calls come in the loop's order, whatever lies between them
        at = {s: 0 for s in range(len(c.solves))}
        done = 0
        for item in c.script:
            s = item[1]
            assert 0 <= s < len(c.solves)
            if item[0] == "extra":
                assert item[2] in fuzz_gen.LOOP_EXTRAS and item[4] == at[s], (c.seed, item)
                if item[2] == "inject":
                    assert c.mode in fuzz_gen.INJECT_MODES
                    i, bits = item[3]
                    assert 0 <= i < c.solves[s]["nnz"] and bits and all(0 <= b < 96 for b in bits)
                    assert c.mode == "none" or len(bits) == 1
                continue
            name = "dot" if item[0] == "dot_copies" else item[0]
            assert fuzz_gen.LOOP_MAIN[at[s]] == name, (c.seed, item)
            if name in ("calc_xr", "calc_p"):
                assert (item[2] == "q" and item[3] in (-1, 0, 1)) or (item[2] == "c" and np.isfinite(item[3]))
            at[s] = (at[s] + 1) % 4
            done += name == "calc_p"
        assert all(v == 0 for v in at.values()), c.seed  # no iteration left open
        assert done == c.iterations and 10 <= c.iterations <= 40, (c.seed, c.iterations)


def test_loop_coverage_over_the_seeds_the_gpu_test_plays(loops):
    n = len(loops)
    assert 3 * sum(c.tags["must_commit"] for c in loops) >= n
    for kind in fuzz_gen.LOOP_EXTRAS:
        for gap in range(4):
            have = sum((kind, gap) in c.tags["in_flight"] for c in loops)
            assert have >= 3, (kind, gap, have)
    for tag in ("three_lengths", "same_length_pair", "switch_inside", "event_every_spmv", "plain_loop"):
        assert sum(bool(c.tags[tag]) for c in loops) >= 3, tag
    for e in fuzz_gen.LOOP_SCALES:
        assert sum(e in c.tags["scaled"] for c in loops) >= 3, e
    assert {c.mode for c in loops} == set(fuzz_gen.MODES)
    # stretches of three and more undisturbed iterations are common, and so are disturbed ones
    assert sum(len(c.tags["in_flight"]) for c in loops) >= 2 * n


def test_loop_injects_against_the_oracle(loops):
    """the oracle alone: a single-bit flip in an ECC mode is corrected (one event, not fatal, gone at the next SpMV),
    a flip in mode none is silent, and the order violation of a constraints case is reported at every SpMV"""
    seen = {m: 0 for m in fuzz_gen.INJECT_MODES}
    for c in loops:
        flips = [(i[1], i[3]) for i in c.script if i[0] == "extra" and i[2] == "inject"]
        assert bool(c.tags["event_every_spmv"]) == (c.mode == "constraints" and bool(flips))
        for s, v in enumerate(c.solves):
            mine = [f for t, f in flips if t == s]
            if not mine:
                continue
            cols, rows, vals, n = fuzz_gen.loop_matrix(v["spec"])
            o = OracleMatrix(CSR, c.mode, cols, rows, vals, n)
            x = np.ones(n)
            for i, bits in mine:
                o.inject(i, list(bits))
                seen[c.mode] += 1
            for stage in range(2):
                o.spmv(x)
                ev, fatal = o.events()
                if c.mode == "none":
                    assert (ev, fatal) == ([], False)
                elif c.mode == "constraints":
                    assert len(mine) == 1 and fatal and [e[:2] for e in ev] == [(8, mine[0][0])], (c.seed, ev)
                else:
                    assert not fatal and len(ev) == (len(mine) if stage == 0 else 0), (c.seed, c.mode, stage, ev)
            o.close()
    assert all(v >= 3 for v in seen.values()), seen
