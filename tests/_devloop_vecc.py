"""numpy model of the two-kernel tail on protected vectors and of the guarded iteration built on it (DESIGN.md
section 5k), on top of the model of tests/_vecc.py: calc_r and calc_px are calc_xr and calc_p cut where the plain
loop cuts them -- the r half alone, the x half inside the pass over p -- and the guarded iteration is
spmv + p.w + calc_r + calc_px behind the stop test `rr > threshold`, the two quotients IEEE divisions.
Written from the text of the section, not from the device code.  Every sum is serial, as in _vecc."""
import numpy as np

import _vecc

U = np.uint64
# the ordinals of the guarded entry's vector events: its vector arguments vec, x, r, p, w in order
OPERAND = {"vec": 0, "x": 1, "r": 2, "p": 3, "w": 4}


def fdiv(a, b):
    """the IEEE quotient (x / 0 and 0 / 0 included) -- what the device forms"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def calc_r(rw, ww, alpha):
    """r <- enc(dec(r) - alpha dec(w)) -> (r words, r.r over the stored r)"""
    with np.errstate(all="ignore"):
        rs = _vecc.encode(_vecc.value(rw) - alpha * _vecc.value(ww))
        return rs, _vecc.serial_sum(_vecc.strip(rs) * _vecc.strip(rs))


def calc_px(xw, pw, rw, alpha, beta):
    """x <- enc(dec(x) + alpha dec(p)), p <- enc(dec(r) + beta dec(p)), both from the old p -> (x words, p words)"""
    with np.errstate(all="ignore"):
        p = _vecc.value(pw)
        return _vecc.encode(_vecc.value(xw) + alpha * p), _vecc.encode(_vecc.value(rw) + beta * p)


def iteration(csr, xw, rw, pw, rr, threshold, p_dot_w=None, rr_new=None):
    """One guarded iteration with vec = p.  -> dict(live, x, r, p, w, pw, rr_new): live False is the frozen
    iteration -- x, r, p the arrays passed in, w and pw None (unspecified), rr_new the BITS of rr handed on.
    p_dot_w, rr_new: the device's tree sums, where the caller wants the words those give and not the words the
    model's serial sums give (the two differ in the last bits and everything behind them follows)."""
    if not (rr > threshold):  # false for NaN
        return dict(live=False, x=xw, r=rw, p=pw, w=None, pw=None, rr_new=rr)
    rowptr, cols, vals = csr
    ww, fused = _vecc.spmv(rowptr, cols, vals, pw)
    p_dot_w = fused if p_dot_w is None else p_dot_w
    alpha = fdiv(rr, p_dot_w)
    rs, rr_model = calc_r(rw, ww, alpha)
    rr_new = rr_model if rr_new is None else rr_new
    xs, ps = calc_px(xw, pw, rs, alpha, fdiv(rr_new, rr))
    return dict(live=True, x=xs, r=rs, p=ps, w=ww, pw=p_dot_w, rr_new=rr_new)


def flipped(words, index, bits):
    out = np.asarray(words, dtype=U).copy()
    for b in bits:
        out[index] ^= U(1 << b)
    return out
