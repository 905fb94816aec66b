"""What the structure-protection tests share (test_struct_ecc_host.py, test_gpu_structure_ecc.py): the matrices, and
host models of the two stored words -- a row extent word under the model of tests/_vecc.py, a row-block descriptor
under the oracle's COO secded element.  numpy and the oracle only."""
import numpy as np

import _vecc as V
from _matrices import matrix as _matrix
from _oracle import COO, Oracle, laplace5

U = np.uint64
M28 = (1 << 28) - 1
ROW, BLOCK = 0, 1  # the kind of a structure word / event

# `wide5`: a 300 x 5 grid.  lap40's rows change length every 40 rows, so none of its blocks of ~200 rows is uniform
# (test_struct_ecc_host.py proves both); here runs of 298 rows of 5 elements hold whole blocks, and the blocks across
# the grid's edges are not uniform.
NAMES = ["one", "lap3", "lap40", "wide5", "rand", "diag23", "arrow", "holes"]
_made = {}


def matrix(name):
    if name == "wide5":
        if name not in _made:
            _made[name] = laplace5(300, 5)
        return _made[name]
    return _matrix(name)


def rowptr_of(rows, n):
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, np.asarray(rows, np.int64) + 1, 1)
    return np.cumsum(ptr)


def pack(rs, re_):
    return (np.asarray(rs, dtype=U) << U(7)) | (np.asarray(re_, dtype=U) << U(35))


def row_words(ptr):
    """rowptr -> the stored row extent words"""
    ptr = np.asarray(ptr, dtype=U)
    return V.encode(pack(ptr[:-1], ptr[1:]).view(np.float64))


def strip_rows(words):
    """stored row words -> rowptr, code bits dropped, no check"""
    w = np.asarray(words, dtype=U)
    if not len(w):
        return np.zeros(1, np.int64)
    return np.concatenate([(w >> U(7)) & U(M28), [(w[-1] >> U(35)) & U(M28)]]).astype(np.int64)


def blk_words(desc):
    """(nblk, 4) plain descriptors -> the stored words"""
    return np.array([Oracle.encode(COO, "secded", [int(d[0]) & 0x00FFFFFF, int(d[1]), int(d[2]), int(d[3])]) for d in desc],
                    dtype=np.uint32).reshape(-1, 4)
