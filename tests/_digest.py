"""The numpy model of the matrix digest (abft_sparse_cg_amd/csrc/matrix_digest.h), shared by test_matrix_digest_host.py
and test_gpu_matrix_digest.py: a segment's bytes as little-endian 32-bit words w[0..n), the last one zero-extended,
D = sum w[i] (2 i + 1) mod 2^64.  numpy only."""
import numpy as np

MAX_WORDS = 1 << 31
MASK = (1 << 64) - 1


def words(data):
    """bytes / uint8 array -> uint32[n], n = ceil(len / 4), zero-extended"""
    b = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    pad = (-len(b)) % 4
    if pad:
        b = np.concatenate([b, np.zeros(pad, np.uint8)])
    return b.view("<u4")


def digest(data):
    w = words(data)
    if len(w) > MAX_WORDS:
        raise OverflowError("more than 2^31 words")
    if not len(w):
        return 0
    # uint64 arithmetic wraps mod 2^64, which is the definition
    weight = np.arange(len(w), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    with np.errstate(over="ignore"):
        return int(np.sum(w.astype(np.uint64) * weight, dtype=np.uint64))


def digest_exact(data):
    """the same with Python integers: the model of the model"""
    return sum(int(v) * (2 * i + 1) for i, v in enumerate(words(data))) & MASK
