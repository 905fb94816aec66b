"""numpy model of the guarded block iteration on protected vectors (abft_hip_cg_block_vecc_iteration_until_dev;
DESIGN.md section 5n), on top of the model of the protected block calls (tests/_vecc_block.py): one iteration is
spmm_dot + calc_r_block + calc_px_block with the mask of the columns whose record word is above the threshold, the
2K quotients IEEE divisions; the records are plain doubles, moved as integers where a column is frozen.
Written from the text of the section, not from the device code.  Every sum is serial, as in _vecc."""
import numpy as np

import _vecc
import _vecc_block as B

U = np.uint64
# the ordinals of the entry's vector events: the single guarded entries' numbering (0: the P the SpMM gathers)
OPERAND = {"gather": 0, "X": 1, "R": 2, "P": 3, "W": 4}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(U)


def live_mask(rr, threshold):
    """bit j: rr[j] > threshold (false for NaN)"""
    with np.errstate(all="ignore"):
        return sum(1 << j for j in range(len(rr)) if rr[j] > threshold)


def iteration(csr, X, R, P, rec, threshold, p_dot_w=None, sums=None):
    """One guarded iteration.  X, R, P: (N, K) stored words; rec: the 2K record words {r.r[K], r.z[K]} as float64.
    -> dict(active, X, R, P, W, pw, rec): rec the 2K words of the record it leaves, as uint64.  No column live: X, R, P
    are the arrays passed in, W and pw None (unspecified), the record's words handed on.  p_dot_w, sums: the device's
    tree sums, where the caller wants the words those give and not the words the model's serial sums give."""
    k = X.shape[1]
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    assert rec.size == 2 * k
    words = rec.view(U).copy()
    active = live_mask(rec[:k], threshold)
    if not active:
        return dict(active=0, X=X, R=R, P=P, W=None, pw=None, rec=words)
    W, fused = B.spmm_dot(csr, P)
    pw = fused if p_dot_w is None else np.asarray(p_dot_w, dtype=np.float64)
    alpha = [B.fdiv(rec[k + j], pw[j]) if B.on(active, j) else 0.0 for j in range(k)]
    R1, model_sums = B.calc_r_block(R, W, alpha, active)
    s = model_sums if sums is None else np.asarray(sums, dtype=np.float64)
    beta = [B.fdiv(s[j], rec[k + j]) if B.on(active, j) else 0.0 for j in range(k)]
    X1, P1 = B.calc_px_block(X, P, R1, alpha, beta, active)
    for j in range(k):
        if B.on(active, j):  # a live column: its new sum in both words; a frozen one: its old words
            words[j] = words[k + j] = bits(s[j:j + 1])[0]
    return dict(active=active, X=X1, R=R1, P=P1, W=W, pw=pw, rec=words)


def cg_block_loop(csr, Bm, max_itrs, threshold, stride=16):
    """cg_solve_block_device(vector_ecc=True) on the model, driven record by record over a trail of stride + 1
    records: Bm (N, K) plain doubles, x0 = 0 -> (itrs[K], history (a list of rr[K] per live iteration), X words)"""
    n, k = Bm.shape
    X = np.stack([_vecc.encode(np.zeros(n)) for _ in range(k)], axis=1)
    R = B.repaired(np.stack([_vecc.encode(Bm[:, j]) for j in range(k)], axis=1))
    P = R.copy()
    rr = B.dot_block(R, R)
    itrs, hist = [0] * k, []
    if max_itrs == 0 or not live_mask(rr, threshold):
        return itrs, hist, B.repaired(X)
    trail = np.zeros((stride + 1, 2 * k), dtype=U)
    trail[stride] = bits(np.concatenate([rr, rr]))
    done = 0
    while True:
        m = min(stride, max_itrs - done)
        trail[0] = trail[stride]
        for i in range(m):  # the batch: enqueued blind, frozen iterations included
            out = iteration(csr, X, R, P, trail[i].view(np.float64), threshold)
            X, R, P, trail[i + 1] = out["X"], out["R"], out["P"], out["rec"]
        stopped = False
        for i in range(m):  # the host's look at the downloaded trail
            active = live_mask(trail[i, :k].view(np.float64), threshold)
            if not active:
                stopped = True
                break
            for j in range(k):
                itrs[j] += (active >> j) & 1
            hist.append(trail[i + 1, :k].view(np.float64).copy())
            done += 1
        if stopped or done >= max_itrs:
            break
    return itrs, hist, B.repaired(X)
