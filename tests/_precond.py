"""Shared by test_precond_host.py and test_gpu_precond.py: the badly scaled systems of the Jacobi tests and a
numpy model of the two loops (plain CG and Jacobi-preconditioned CG as context.cg_solve runs them), which
sets the iteration counts the GPU solves are held against.  No GPU, no package import."""
import numpy as np


def scaling(n):
    """s_i = 2^((7919 i mod 13) - 6): powers of two, so S A S is exact in fp64"""
    i = np.arange(n, dtype=np.int64)
    return np.ldexp(1.0, ((7919 * i) % 13 - 6).astype(np.int32))


def scaled(cols, rows, vals, n):
    """the triplets of S A S"""
    s = scaling(n)
    return cols, rows, vals * s[rows.astype(np.int64)] * s[cols.astype(np.int64)], n


def matvec(cols, rows, vals, n, x):
    return np.bincount(rows.astype(np.int64), weights=vals * x[cols.astype(np.int64)], minlength=n)


def diagonal(cols, rows, vals, n):
    """d[i] = sum of the elements with row == col == i, in element order (np.add.at is serial)"""
    d = np.zeros(n)
    m = rows == cols
    np.add.at(d, rows[m].astype(np.int64), vals[m])
    return d


def model_cg(cols, rows, vals, n, b, conv, max_itrs, dinv=None):
    """-> (iterations, rr, x): context.cg_solve's loop in numpy (dinv=None: plain CG)"""
    x = np.zeros(n)
    r = b.copy()
    z = r if dinv is None else dinv * r
    p = z.copy()
    rz, rr = float(np.sum(r * z)), float(np.sum(r * r))
    itr = 0
    while itr < max_itrs and rr > conv:
        w = matvec(cols, rows, vals, n, p)
        alpha = rz / float(np.sum(p * w))
        x = x + alpha * p
        r = r - alpha * w
        z = r if dinv is None else dinv * r
        rz_new, rr = float(np.sum(r * z)), float(np.sum(r * r))
        p = z + (rz_new / rz) * p
        rz = rz_new
        itr += 1
    return itr, rr, x
