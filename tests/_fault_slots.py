"""What the matrix-fault sweeps are made of (test_fault_slots_host.py, test_gpu_matrix_fault_slots.py): one bit flip
per stored element, so that every slot of every tile of every SpMV / SpMM path has to repair one.  numpy and the
oracle only; nothing here loads libabft_hip.so."""
import numpy as np

from _matrices import arrow, matrix
from _oracle import COO, CSR, OracleMatrix

NBITS = {CSR: 96, COO: 128}
FNAME = {CSR: "csr", COO: "coo"}
# the position sec7 cannot see (bit 24 of the ECC word: sec8's overall parity bit, in none of the seven masks):
# documented and pinned against the oracle by test_gpu_parity.py::test_every_single_bit_flip -- the one thing the
# sweeps leave out
SEC7_BLIND = {CSR: 88, COO: 24}
CORRECTING = ["sec7", "sec8", "secded"]
SEEDS = [0, 1, 2]
# the oracle wrapper reads at most this many events per call (OracleMatrix.events)
ORACLE_EVENTS = 4096

_made = {}


def sweep_matrix(name):
    """arrow1300: 3898 elements, row 0 holds 1300 (longer than a 1024-element tile), the other rows two;
    holes: empty rows, 4 elements to 3 rows, row blocks cut by the 1024-element tile at 768 rows; rand: 26977 elements,
    27 tiles with ragged, odd block starts; diag23: one element per row, the one whose row blocks are cut by the
    1024-row cap; lap37x41: the regular one"""
    if name == "arrow1300":
        if name not in _made:
            _made[name] = arrow(1300)
        return _made[name]
    return matrix(name)


def flip_plan(fmt, mode, nnz, seed):
    """-> int array, the bit to flip in element i: (37 i + 11 seed + 5) % NBITS (37 is odd, so NBITS consecutive
    elements walk every position); in sec7 the blind position gives way to the next one"""
    nb = NBITS[fmt]
    bits = (37 * np.arange(nnz, dtype=np.int64) + 11 * seed + 5) % nb
    if mode == "sec7":
        bits[bits == SEC7_BLIND[fmt]] = (SEC7_BLIND[fmt] + 1) % nb
    return bits


def chunks(nnz):
    """consecutive index ranges of at most ORACLE_EVENTS elements: one pass is made per chunk"""
    return [range(lo, min(lo + ORACLE_EVENTS, nnz)) for lo in range(0, nnz, ORACLE_EVENTS)]


def fatal_sites(nnz, stride):
    """the first two and the last two elements, and every stride-th"""
    return sorted(set(i for i in (0, 1, nnz - 2, nnz - 1) if 0 <= i < nnz) | set(range(0, nnz, stride)))


def second_bit(fmt, bit):
    """the partner of `bit` in a double flip (secded: detected, not repaired)"""
    return (bit + 41) % NBITS[fmt]


class TwinOracle:
    """the oracle that takes the same flips as the matrix under test, one per (matrix, format, mode), reused across
    chunks and seeds: the flips of a chunk are repaired by the pass that reports them (test_fault_slots_host.py holds
    that against the clean words, `words`, after every pass)"""

    def __init__(self, fmt, mode, mat):
        cols, rows, vals, n = mat
        self.fmt, self.mode, self.n, self.nnz = fmt, mode, n, len(vals)
        self.o = OracleMatrix(fmt, mode, cols, rows, vals, n)
        self.words = self.o.stored_words()

    def plant(self, sites, bits):
        for i in sites:
            self.o.inject(int(i), [int(bits[i])])

    def run(self, x):
        """-> (y, events, fatal)"""
        y = self.o.spmv(x)
        ev, fatal = self.o.events()
        return y, ev, fatal
