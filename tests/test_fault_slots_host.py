"""The inputs of the matrix-fault sweeps (tests/_fault_slots.py), on the oracle alone: a flip in every element of a
chunk is reported once, repaired, and leaves the clean y and the clean words behind; the plan walks every bit
position but sec7's blind one; a chunk never holds more events than the oracle wrapper reads; and an oracle whose
sed flip was undone is a fresh one again -- so the GPU file (test_gpu_matrix_fault_slots.py) can hold one oracle per
(matrix, format, mode) and compare every pass with it."""
import numpy as np
import pytest

from _fault_slots import (CORRECTING, FNAME, NBITS, ORACLE_EVENTS, SEC7_BLIND, SEEDS, TwinOracle, chunks, fatal_sites,
                          flip_plan, second_bit, sweep_matrix)
from _oracle import COO, CSR, EV_BIT, EV_DOUBLE, EV_PARITY, EV_SED, OracleMatrix, event_lines, rhs

MATS = ["arrow1300", "holes", "rand", "diag23", "lap37x41"]
FMTS = [CSR, COO]


def bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def test_matrices_are_what_the_sweeps_count_on():
    cols, rows, vals, n = sweep_matrix("arrow1300")
    assert len(vals) == 3898 and int((rows == 0).sum()) == 1300 > 1024
    assert set(np.bincount(rows)[1:]) == {2}
    cols, rows, vals, n = sweep_matrix("holes")
    per_row = np.bincount(rows, minlength=n)
    assert n > 1024 and int((per_row == 0).sum()) == n // 3
    assert len(sweep_matrix("rand")[2]) == 26977
    cols, rows, vals, n = sweep_matrix("diag23")  # one element per row: a row block is full at 1024 rows, not elements
    assert n == len(vals) > 2 * 1024 and np.array_equal(rows, np.arange(n))


@pytest.mark.parametrize("fmt", FMTS, ids=FNAME.get)
@pytest.mark.parametrize("mode", CORRECTING)
def test_flip_plan_hits_every_bit_but_the_blind_one(fmt, mode):
    nb = NBITS[fmt]
    for mat in MATS:
        nnz = len(sweep_matrix(mat)[2])
        for seed in SEEDS:
            plan = flip_plan(fmt, mode, nnz, seed)
            assert len(plan) == nnz and plan.min() >= 0 and plan.max() < nb
            want = set(range(nb)) - ({SEC7_BLIND[fmt]} if mode == "sec7" else set())
            assert set(plan.tolist()) == want, (mat, seed)
            raw = (37 * np.arange(nnz) + 11 * seed + 5) % nb
            moved = plan != raw
            assert np.array_equal(moved, (raw == SEC7_BLIND[fmt]) & (mode == "sec7"))
            assert np.all(plan[moved] == SEC7_BLIND[fmt] + 1)
    # the three seeds give an element three different bits
    a, b, c = (flip_plan(fmt, "secded", 500, s) for s in SEEDS)
    assert not np.any(a == b) and not np.any(b == c) and not np.any(a == c)


def test_chunks_and_sites():
    for nnz in (0, 1, 5, ORACLE_EVENTS - 1, ORACLE_EVENTS, ORACLE_EVENTS + 1, 3898, 26977):
        cs = chunks(nnz)
        assert all(0 < len(c) <= ORACLE_EVENTS for c in cs)
        assert [i for c in cs for i in c] == list(range(nnz))
    assert len(chunks(26977)) == 7 and len(chunks(3898)) == 1
    assert fatal_sites(11, 5) == [0, 1, 5, 9, 10]
    assert fatal_sites(3898, 5)[:3] == [0, 1, 5] and fatal_sites(3898, 5)[-3:] == [3895, 3896, 3897]
    assert fatal_sites(2, 5) == [0, 1] and fatal_sites(1, 5) == [0]
    assert fatal_sites(40, 1) == list(range(40))


@pytest.mark.parametrize("fmt", FMTS, ids=FNAME.get)
@pytest.mark.parametrize("mode", CORRECTING)
@pytest.mark.parametrize("mat", MATS)
def test_a_flip_in_every_element_is_repaired(mat, mode, fmt):
    m = sweep_matrix(mat)
    co = TwinOracle(fmt, mode, m)
    x = rhs(co.n, 7) - 0.5
    clean_y, ev, fatal = co.run(x)
    assert ev == [] and not fatal
    for seed in SEEDS:
        plan = flip_plan(fmt, mode, co.nnz, seed)
        for ch in chunks(co.nnz):
            assert len(ch) <= ORACLE_EVENTS
            co.plant(ch, plan)
            damaged = co.o.stored_words()
            assert int(np.any(damaged != co.words, axis=1).sum()) == len(ch)
            y, ev, fatal = co.run(x)
            assert len(ev) == len(ch) and not fatal, (seed, ch)
            assert [e[1] for e in ev] == list(ch)
            for (kind, i, bit) in ev:  # the planted bit itself, or the parity bit by its own event
                if kind == EV_BIT:
                    assert bit == plan[i], (i, bit)
                else:
                    assert kind == EV_PARITY and mode != "sec7" and plan[i] == SEC7_BLIND[fmt], (kind, i)
            assert bits_equal(y, clean_y), (seed, ch)
            assert np.array_equal(co.o.stored_words(), co.words), (seed, ch)
            y2, ev2, fatal2 = co.run(x)
            assert ev2 == [] and not fatal2 and bits_equal(y2, clean_y)


@pytest.mark.parametrize("fmt", FMTS, ids=FNAME.get)
@pytest.mark.parametrize("mode,kind", [("sed", EV_SED), ("secded", EV_DOUBLE)])
@pytest.mark.parametrize("mat", ["arrow1300", "holes"])
def test_an_oracle_whose_flip_was_undone_is_a_fresh_one(mat, mode, kind, fmt):
    """sed: one flip; secded: two flips in one element.  One fatal event naming the element (sed) or nothing
    (secded's line carries no index); after a second inject of the same bits the oracle has the fresh one's
    words and its next pass is silent and gives the clean y -- at every site the GPU sweeps visit."""
    cols, rows, vals, n = m = sweep_matrix(mat)
    co = TwinOracle(fmt, mode, m)
    x = rhs(n, 7) - 0.5
    clean_y = OracleMatrix(fmt, mode, cols, rows, vals, n).spmv(x)
    plan = flip_plan(fmt, mode, co.nnz, 1)
    for i in fatal_sites(co.nnz, 1):
        bits = [int(plan[i])] + ([second_bit(fmt, int(plan[i]))] if mode == "secded" else [])
        co.o.inject(i, bits)
        _, ev, fatal = co.run(x)
        assert fatal and ev == [(kind, i, 0)], (i, ev)
        co.o.inject(i, bits)
        assert np.array_equal(co.o.stored_words(), co.words), i
        y, ev, fatal = co.run(x)
        assert ev == [] and not fatal and bits_equal(y, clean_y), i
    line = event_lines([(kind, 7, 0)], fmt)[0]
    assert line == ("[ECC] error detected at index 7\n" if mode == "sed" else "[ECC] double-bit error detected\n")
