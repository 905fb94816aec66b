"""A plain numpy model of one iteration of the device-scalar CG loop (abft_hip_cg_iteration_dev, or
abft_hip_spmv_dot_dev + abft_hip_calc_xr_ratio_dev + abft_hip_calc_p_ratio_dev; reference loop cg.cpp:97-112), for
the GPU tests to compare against (test infrastructure only, not a conftest).

The model shares nothing with the kernels: the SpMV is the oracle's, the vector updates are numpy's element-wise
multiply and add -- two roundings each, as in the library, which is built with -ffp-contract=off -- and the two
reductions are not formed at all: the model hands back their TERMS, so that a caller can hold the device's scalars
against _ieee.exact_sum(terms) within _ieee.sum_bound(terms, depth of the kernel's summation tree).  alpha and beta
are the IEEE quotients of the scalars the device left behind (the method of tools/fuzz_sequence.py's devstep): given
those two numbers every vector is determined bit for bit."""
from collections import namedtuple

import numpy as np

Iteration = namedtuple("Iteration", "x r p w alpha beta pw_terms rr_terms")


def model_iteration(o, x, r, p_full, off, w_prev, rr, pw, rr_new):
    """o: the OracleMatrix (n_out rows, n_in = len(p_full) columns); x, r: the shard's n_out entries; p_full: the
    vector the SpMV reads, p being its window [off, off + n_out); w_prev: what w held before the call -- the SpMV
    rewrites every entry, so nothing of it may show in any result (only its length is used); rr: the scalar the
    iteration started from; pw, rr_new: what the device left in the two pairs.
    -> Iteration(x, r, p [the window's new values], w, alpha, beta, pw_terms, rr_terms); the inputs stay unchanged."""
    x = np.asarray(x, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    p_full = np.asarray(p_full, dtype=np.float64)
    n = len(x)
    assert len(r) == n and len(w_prev) == n and 0 <= off and off + n <= len(p_full)
    p = p_full[off:off + n]
    with np.errstate(all="ignore"):
        w = o.spmv(p_full)
        pw_terms = p * w
        alpha = np.float64(rr) / np.float64(pw)        # cg.cpp:102
        r_new = r - alpha * w                          # the product rounded, then the difference
        rr_terms = r_new * r_new
        beta = np.float64(rr_new) / np.float64(rr)     # cg.cpp:109
        x_new = x + alpha * p
        p_new = r_new + beta * p
    return Iteration(x_new, r_new, p_new, w, float(alpha), float(beta), pw_terms, rr_terms)
