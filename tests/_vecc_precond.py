"""numpy model of Jacobi-preconditioned CG on protected vectors, on top of the model of the
protected element in tests/_vecc.py.  Written from the rules of the section, not from the device code:

  val(w)  the repaired word without its 7 code bits        (_vecc.value)
  enc(v)  v truncated toward zero plus the code bits       (_vecc.encode)
  strip   clears the code bits                             (_vecc.strip)

z = val(dinv[i]) * (value of r[i]) is one rounded fp64 product, never stored and never truncated; every multiply and
add is separate; sums are taken over the values as stored (r after enc, z as formed from that r).  Sums are serial, in
element order, unless a caller passes another `total`."""
import numpy as np

import _vecc
from _oracle import laplace5

U = np.uint64
# the ordinals of the guarded entry's vector events: its vector arguments in order
OPERAND = {"vec": 0, "x": 1, "r": 2, "p": 3, "w": 4, "dinv": 5}


def fdiv(a, b):
    """the IEEE quotient (x / 0 and 0 / 0 included)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def pairwise_sum(terms):
    """the same terms added as a balanced binary tree: another order of the same adds"""
    t = np.asarray(terms, dtype=np.float64)
    if len(t) == 0:
        return 0.0
    while len(t) > 1:
        if len(t) % 2:
            t = np.concatenate([t, [0.0]])
        with np.errstate(all="ignore"):
            t = t[0::2] + t[1::2]
    return float(t[0])


def precond_start(rw, dw, total=_vecc.serial_sum):
    """p <- enc(z), z from val(r) -> (p words, sum val(r) z, sum val(r) val(r))"""
    with np.errstate(all="ignore"):
        r = _vecc.value(rw)
        z = _vecc.value(dw) * r
        return _vecc.encode(z), total(r * z), total(r * r)


def calc_r_precond(rw, ww, dw, alpha, total=_vecc.serial_sum):
    """r <- enc(val(r) - alpha val(w)) -> (r words, sum r' z', sum r' r'), r' = strip(stored r), z' = val(dinv) r'"""
    with np.errstate(all="ignore"):
        rs = _vecc.encode(_vecc.value(rw) - alpha * _vecc.value(ww))
        r = _vecc.strip(rs)
        z = _vecc.value(dw) * r
        return rs, total(r * z), total(r * r)


def calc_px_precond(xw, pw, rw, dw, alpha, beta):
    """x <- enc(val(x) + alpha val(p)), p <- enc(val(dinv) val(r) + beta val(p)), both from the old p -> (x, p) words"""
    with np.errstate(all="ignore"):
        p = _vecc.value(pw)
        z = _vecc.value(dw) * _vecc.value(rw)
        return _vecc.encode(_vecc.value(xw) + alpha * p), _vecc.encode(z + beta * p)


def spmv_dot(csr, pw, total=_vecc.serial_sum):
    """-> (w words, p.w over the stored w)"""
    ww, fused = _vecc.spmv(*csr, pw)
    if total is _vecc.serial_sum:
        return ww, fused
    with np.errstate(all="ignore"):
        return ww, total(_vecc.value(pw) * _vecc.strip(ww))


def pcg_loop(csr, b, dinv, max_itrs, conv_threshold, total=_vecc.serial_sum):
    """cg_solve(vector_ecc=True, precond=dinv) from x = 0: b and dinv plain doubles, encoded here.  dinv None: the
    unpreconditioned protected loop (calc_xr + calc_p of _vecc).  -> (iterations, history of r.r, x words)"""
    n = len(b)
    bw, xw = _vecc.encode(b), _vecc.encode(np.zeros(n))
    rw = bw.copy()
    if dinv is None:
        pw, rr = rw.copy(), total(_vecc.value(rw) * _vecc.value(rw))
        rz = rr
    else:
        dw = _vecc.encode(dinv)
        pw, rz, rr = precond_start(rw, dw, total)
    hist, itr = [], 0
    while itr < max_itrs and rr > conv_threshold:
        ww, p_dot_w = spmv_dot(csr, pw, total)
        alpha = fdiv(rz, p_dot_w)
        if dinv is None:
            with np.errstate(all="ignore"):
                xw = _vecc.encode(_vecc.value(xw) + alpha * _vecc.value(pw))
                rw = _vecc.encode(_vecc.value(rw) - alpha * _vecc.value(ww))
                rr_new = total(_vecc.strip(rw) * _vecc.strip(rw))
                pw = _vecc.encode(_vecc.value(rw) + fdiv(rr_new, rr) * _vecc.value(pw))
            rz = rr_new
        else:
            rw, rz_new, rr_new = calc_r_precond(rw, ww, dw, alpha, total)
            xw, pw = calc_px_precond(xw, pw, rw, dw, alpha, fdiv(rz_new, rz))
            rz = rz_new
        rr = rr_new
        hist.append(rr)
        itr += 1
    return itr, hist, xw


def iteration(csr, xw, rw, pw, dw, rec, threshold, p_dot_w=None, sums=None):
    """One guarded iteration with vec = p; rec = (r.r, r.z) of the record it reads.  -> dict(live, x, r, p, w, pw, out):
    live False is the frozen iteration -- x, r, p the arrays passed in, w and pw None (unspecified), out the record's
    two values handed on.  p_dot_w, sums = (r.z', r.r'): the device's tree sums, where the caller wants the words
    those give and not the words the model's serial sums give."""
    rr, rz = rec
    if not (rr > threshold):  # false for NaN
        return dict(live=False, x=xw, r=rw, p=pw, w=None, pw=None, out=(rr, rz))
    ww, fused = _vecc.spmv(*csr, pw)
    p_dot_w = fused if p_dot_w is None else p_dot_w
    alpha = fdiv(rz, p_dot_w)
    rs, rz_m, rr_m = calc_r_precond(rw, ww, dw, alpha)
    rz_new, rr_new = (rz_m, rr_m) if sums is None else sums
    xs, ps = calc_px_precond(xw, pw, rs, dw, alpha, fdiv(rz_new, rz))
    return dict(live=True, x=xs, r=rs, p=ps, w=ww, pw=p_dot_w, out=(rr_new, rz_new))


def flipped(words, index, bits):
    out = np.asarray(words, dtype=U).copy()
    for b in bits:
        out[index] ^= U(1 << b)
    return out


def scaled_laplace(nx, ny, span):
    """D^(1/2) L D^(1/2) of laplace5(nx, ny), D = diag(d) with d log-spaced over `span` decades (10^(-span/2) ..
    10^(span/2) in row order): symmetric positive definite, badly scaled -- its diagonal 4 d spans `span` decades --,
    and Jacobi undoes exactly that scaling.  -> (cols, rows, vals, n), sorted as laplace5 sorts"""
    cols, rows, vals, n = laplace5(nx, ny)
    s = np.sqrt(np.logspace(-span / 2.0, span / 2.0, n))
    return cols, rows, s[rows] * vals * s[cols], n


def jacobi(mat):
    """1 / diagonal, as ctx.jacobi forms it for a matrix with one positive diagonal element per row"""
    cols, rows, vals, n = mat
    d = np.zeros(n)
    on = cols == rows
    d[rows[on]] = vals[on]
    return 1.0 / d
