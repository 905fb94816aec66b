"""numpy model of the protected block operations (abft_hip_spmm_dot_vecc, abft_hip_dot_block_vecc,
abft_hip_calc_r_block_vecc, abft_hip_calc_px_block_vecc), built on the model of the single
protected calls (tests/_vecc.py) column by column.  A block is an (N, K) array of stored words, row-major as on the
device: entry (i, j) at i * K + j.  An active column is computed with _vecc's functions; an inactive column of a
written block comes back as its words REPAIRED (a clean word keeps every bit, a single flip is undone, two flips stay).
Every sum is serial, in row order, with separate multiply and add."""
import numpy as np

import _vecc

U = np.uint64


def block(words, k):
    """flat stored words (device order) -> (N, K)"""
    w = np.asarray(words, dtype=U)
    assert w.size % k == 0
    return w.reshape(-1, k).copy()


def flat(b):
    return np.ascontiguousarray(b, dtype=U).reshape(-1)


def on(active, j):
    return bool((int(active) >> j) & 1)


def repaired(w):
    return _vecc.decode(w)[0]


def spmm_dot(csr, P):
    """-> (W words (N, K), the K fused products val(P[:, j]) . strip(W[:, j]))"""
    k = P.shape[1]
    W = np.empty_like(P)
    out = np.zeros(k)
    for j in range(k):
        W[:, j], out[j] = _vecc.spmv(*csr, P[:, j])
    return W, out


def dot_block(A, B):
    return np.array([_vecc.dot(A[:, j], B[:, j]) for j in range(A.shape[1])])


def calc_r_block(R, W, alpha, active):
    """-> (R words, the K sums over the stored R of EVERY column)"""
    k = R.shape[1]
    out = np.empty_like(R)
    for j in range(k):
        if on(active, j):
            with np.errstate(all="ignore"):
                out[:, j] = _vecc.encode(_vecc.value(R[:, j]) - alpha[j] * _vecc.value(W[:, j]))
        else:
            out[:, j] = repaired(R[:, j])
    with np.errstate(all="ignore"):
        sums = np.array([_vecc.serial_sum(_vecc.strip(out[:, j]) * _vecc.strip(out[:, j])) for j in range(k)])
    return out, sums


def calc_px_block(X, P, R, alpha, beta, active):
    """-> (X words, P words), both from the old P"""
    k = X.shape[1]
    xo, po = np.empty_like(X), np.empty_like(P)
    for j in range(k):
        if on(active, j):
            with np.errstate(all="ignore"):
                xo[:, j] = _vecc.encode(_vecc.value(X[:, j]) + alpha[j] * _vecc.value(P[:, j]))
            po[:, j] = _vecc.calc_p(P[:, j], R[:, j], beta[j])
        else:
            xo[:, j], po[:, j] = repaired(X[:, j]), repaired(P[:, j])
    return xo, po


def flipped(b, i, j, bits):
    out = np.array(b, dtype=U, copy=True)
    for bit in bits:
        out[i, j] ^= U(1 << bit)
    return out


def fdiv(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def cg_block_loop(csr, B, max_itrs, threshold, total=None, hook=None):
    """cg_solve_block(vector_ecc=True) on the model: B (N, K) plain doubles, x0 = 0 -> (itrs[K], history (a list
    of rr[K] per iteration), X words).  total: the summation every reduction uses (default: serial).  hook(itr, state):
    called after iteration itr with the dict of blocks, which it may damage in place."""
    total = total or _vecc.serial_sum
    n, k = B.shape
    Bw = np.stack([_vecc.encode(B[:, j]) for j in range(k)], axis=1)
    X = np.stack([_vecc.encode(np.zeros(n)) for j in range(k)], axis=1)
    R = repaired(Bw)
    P = R.copy()

    def sums(a, b):
        with np.errstate(all="ignore"):
            return np.array([total(_vecc.value(a[:, j]) * _vecc.value(b[:, j])) for j in range(k)])

    rr = sums(R, R)
    itrs, hist, itr = [0] * k, [], 0
    while True:
        active = sum(1 << j for j in range(k) if itrs[j] < max_itrs and rr[j] > threshold)
        if not active:
            break
        W = spmm_dot(csr, P)[0]
        with np.errstate(all="ignore"):
            pw = np.array([total(_vecc.value(P[:, j]) * _vecc.strip(W[:, j])) for j in range(k)])
        alpha = [fdiv(rr[j], pw[j]) if on(active, j) else 0.0 for j in range(k)]
        R = calc_r_block(R, W, alpha, active)[0]
        rr_new = sums(R, R)
        beta = [fdiv(rr_new[j], rr[j]) if on(active, j) else 0.0 for j in range(k)]
        X, P = calc_px_block(X, P, R, alpha, beta, active)
        for j in range(k):
            if on(active, j):
                rr[j] = rr_new[j]
                itrs[j] += 1
        hist.append(rr.copy())
        if hook is not None:
            state = dict(X=X, R=R, P=P)
            hook(itr, state)
            X, R, P = state["X"], state["R"], state["P"]
        itr += 1
    return itrs, hist, repaired(X)
