"""The small matrices of the cross-call tests (tests/_x_in_spmv.py, tests/_ahead.py) and of the CG-loop family of
tools/fuzz_gen.py: (cols, rows, vals, n), sorted by (row, col).  numpy and the oracle's builders only."""
import numpy as np

from _oracle import laplace5, random_spd


def one_by_one():
    return np.array([0], np.uint32), np.array([0], np.uint32), np.array([3.5]), 1


def diagonal(n, distinct):
    i = np.arange(n)
    vals = 1.0 + (i % 23) * 0.37 if distinct else np.full(n, 2.5)
    return i.astype(np.uint32), i.astype(np.uint32), vals, n


def arrow(n):
    """row 0 full (n elements: longer than an LDS tile), every other row {column 0, diagonal}"""
    i = np.arange(1, n)
    rows = np.concatenate([np.zeros(n, np.int64), np.repeat(i, 2)])
    cols = np.concatenate([np.arange(n), np.stack([np.zeros(n - 1, np.int64), i], 1).reshape(-1)])
    vals = np.concatenate([np.full(n, -1.0 / n), np.stack([np.full(n - 1, -1.0 / n), 2.0 + 0.001 * i], 1).reshape(-1)])
    vals[0] = 3.0
    return cols.astype(np.uint32), rows.astype(np.uint32), vals, n


def every_third_row_empty(n):
    """rows with i % 3 == 2 hold nothing; the others their diagonal and, where it exists, column i + 1"""
    i = np.arange(n)
    keep = i[i % 3 != 2]
    rows, cols, vals = [], [], []
    for k in keep:
        rows.append(k); cols.append(k); vals.append(2.0 + (k % 7) * 0.125)
        if k + 1 < n:
            rows.append(k); cols.append(k + 1); vals.append(-0.5 - (k % 5) * 0.0625)
    return np.array(cols, np.uint32), np.array(rows, np.uint32), np.array(vals), n


MATRICES = {
    "lap40": lambda: laplace5(40, 40),        # N = 1600: 8 row blocks, packed, uniform and edge blocks
    "lap37x41": lambda: laplace5(37, 41),     # N = 1517, odd: calc_p's pair walk has a tail
    "lap3": lambda: laplace5(3, 3),
    "one": one_by_one,
    "rand": lambda: random_spd(3001, 8, seed=5),  # row pointers read; compact or wide blocks, not packed
    "diag23": lambda: diagonal(3000, True),   # blocks of 1024 rows, > 16 values: the row loop runs 4 times
    "diag1": lambda: diagonal(3000, False),   # the same, packed
    "arrow": lambda: arrow(1500),             # the long-row branch
    "holes": lambda: every_third_row_empty(2000),
}
_made = {}


def matrix(name):
    if name not in _made:
        _made[name] = MATRICES[name]()
    return _made[name]
