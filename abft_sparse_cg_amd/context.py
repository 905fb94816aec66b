"""HIPContext -- the Python mirror of the reference's CGContext plugin interface
(reference CGContext.h:13-36) for the `hip` target: same thirteen operations,
same argument meaning, same error behaviour (ECC / constraint events are
printed with the reference's text; fatal ones end the run with status 1).

Every method is a thin call into libabft_hip.so through the C ABI of
include/abft_hip.h; the C++ HIPContext under host/ binds the same ABI for the
cg-csr / cg-coo executables.
"""
import ctypes as C
import functools
import inspect
import math
import sys

import numpy as np

from . import capi
from .capi import FMT_COO, FMT_CSR, MODE_ID, check


class FatalEvent(SystemExit):
    """A fatal ABFT event: the reference prints the line and calls exit(1)
    (e.g. CSR/CPUContext.cpp:233-234).  Subclasses SystemExit(1) so an
    unhandled one ends the process exactly like that."""

    def __init__(self, events):
        super().__init__(1)
        self.events = events


class ResidualCheckFailed(RuntimeError):
    """A residual check failed more than max_rollbacks times, or failed at max_itrs: the
    solve cannot vouch for x (which holds the last checkpoint that passed).  `checks` is the
    record of every check of the solve: (itr, gap, ok, rolled_back_to[, rhs]) as on_check saw it."""

    def __init__(self, message, checks):
        super().__init__(message)
        self.checks = checks


class Matrix:
    def __init__(self, ctx, handle, fmt, mode, n_out, n_in, nnz):
        self.ctx, self.h, self.fmt, self.mode = ctx, handle, fmt, mode
        self.n_out, self.n_in, self.nnz = n_out, n_in, nnz
        self.structure_ecc = False  # create_matrix(structure_ecc=True): the row structure is stored as codewords
        self.digest_armed = False  # arm_matrix has taken its reference digests


class Vector:
    def __init__(self, ctx, handle, n, k=None):
        self.ctx, self.h, self.N = ctx, handle, n
        self.K = k  # block vectors (create_block): N*K entries, (i, j) at i*K + j
        self._dptr = None

    @property
    def device_ptr(self):
        # asked once: the address never changes, and every call of the C function
        # first applies a deferred update (include/abft_hip.h)
        if self._dptr is None:
            self._dptr = capi.load().abft_hip_vector_device_ptr(self.h)
        return self._dptr


class HIPContext:
    """One (format, mode) backend instance on one GPU -- what
    CGContext::create("hip", mode) returns in cg-csr (fmt='csr') or cg-coo
    (fmt='coo')."""

    BITFLIP = {"ANY": capi.FLIP_ANY, "VALUE": capi.FLIP_VALUE, "INDEX": capi.FLIP_INDEX}

    def __init__(self, mode="none", fmt="csr", device=0, on_event=None, rng=None):
        if mode not in MODE_ID:
            # reference CGContext.cpp:20-23
            sys.stderr.write("\nNo implementation found for hip-%s\n\n" % mode)
            raise SystemExit(1)
        self.L = capi.load()
        self.mode, self.mode_id = mode, MODE_ID[mode]
        self.fmt = FMT_CSR if fmt in ("csr", FMT_CSR) else FMT_COO
        self.on_event = on_event
        self.rng = rng  # callable () -> int, stands in for libc rand(); default: libc
        h = C.c_void_p()
        check(self.L.abft_hip_init(device, C.byref(h)))
        self.h = h
        self.event_log = []
        self._evbuf, self._evcap = None, 0
        self.prof_mask = 0
        self.matrix_verifications = 0  # verify_matrix / verify_matrix_dev calls made so far
        self._live = []  # matrices and vectors not yet destroyed, in creation order

    def close(self):
        """destroy what the caller left behind (views before their parents: reverse creation
        order), then the context"""
        if self.h:
            for obj in reversed(self._live):
                if obj.h:
                    if isinstance(obj, Matrix):
                        self.L.abft_hip_matrix_destroy(obj.h)
                    else:
                        self.L.abft_hip_vector_destroy(obj.h)
                    obj.h = None
            self._live = []
            self.L.abft_hip_shutdown(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- matrix -----------------------------------------------------------
    def create_matrix(self, columns, rows, values, N, nnz, n_in=None, index_base=0, layout=None, structure_ecc=False):
        """reference CGContext.h:15-18.  n_in/index_base make a row-block shard.
        layout="stream": CSR, whole matrix, always in the streaming row-block layout -- the
        one spmm runs on (abft_hip_matrix_create_csr_stream); None: the library's choice.
        structure_ecc=True (with layout="stream" only): the row structure is stored as SECDED codewords
        (abft_hip_matrix_create_csr_protected) -- the single-vector SpMV and everything
        built on it run on such a matrix, the block entries refuse it."""
        columns = np.ascontiguousarray(columns, dtype=np.uint32)
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert len(columns) >= nnz and len(rows) >= nnz and len(values) >= nnz
        if layout not in (None, "stream"):
            raise ValueError("layout must be None or 'stream', not %r" % (layout,))
        if structure_ecc and (layout != "stream" or self.fmt != FMT_CSR or (n_in is not None and n_in != N) or index_base):
            raise ValueError("structure_ecc=True takes a whole CSR matrix with layout='stream'")
        h = C.c_void_p()
        if layout == "stream":
            if self.fmt != FMT_CSR or (n_in is not None and n_in != N) or index_base:
                raise ValueError("layout='stream' takes a whole CSR matrix")
            create = self.L.abft_hip_matrix_create_csr_protected if structure_ecc else self.L.abft_hip_matrix_create_csr_stream
            check(create(self.h, self.mode_id, columns.ctypes.data_as(capi.u32p), rows.ctypes.data_as(capi.u32p),
                         values.ctypes.data_as(capi.f64p), N, nnz, C.byref(h)))
            m = Matrix(self, h, self.fmt, self.mode, N, N, nnz)
            m.structure_ecc = bool(structure_ecc)
            self._live.append(m)
            return m
        n_in = N if n_in is None else n_in
        check(self.L.abft_hip_matrix_create_shard(
            self.h, self.fmt, self.mode_id, columns.ctypes.data_as(capi.u32p), rows.ctypes.data_as(capi.u32p),
            values.ctypes.data_as(capi.f64p), N, n_in, nnz, index_base, C.byref(h)))
        m = Matrix(self, h, self.fmt, self.mode, N, n_in, nnz)
        self._live.append(m)
        return m

    def destroy_matrix(self, mat):
        self._drain()
        check(self.L.abft_hip_matrix_destroy(mat.h))
        mat.h = None
        self._live = [o for o in self._live if o is not mat]

    def stored_words(self, mat):
        """(nnz, 3|4) uint32 image of the stored elements in the caller's order."""
        if mat.fmt == FMT_CSR:
            c = np.empty(mat.nnz, dtype=np.uint32)
            v = np.empty(mat.nnz, dtype=np.float64)
            check(self.L.abft_hip_matrix_read_csr(mat.h, c.ctypes.data, None, v.ctypes.data))
            w = np.empty((mat.nnz, 3), dtype=np.uint32)
            w[:, :2] = v.view(np.uint32).reshape(-1, 2)
            w[:, 2] = c
            return w
        w = np.empty((mat.nnz, 4), dtype=np.uint32)
        check(self.L.abft_hip_matrix_read_coo(mat.h, w.ctypes.data))
        return w

    def rowptr(self, mat):
        rp = np.empty(mat.n_out + 1, dtype=np.uint32)
        check(self.L.abft_hip_matrix_read_csr(mat.h, None, rp.ctypes.data, None))
        return rp

    # ---- the protected row structure (include/abft_hip.h) ----
    def structure_protected(self, mat):
        """was the matrix created with structure_ecc=True?"""
        return self._structure_info(mat)[0]

    def _structure_info(self, mat):
        on, rows, blocks = C.c_int(0), C.c_uint32(0), C.c_uint32(0)
        check(self.L.abft_hip_matrix_structure_info(mat.h, C.byref(on), C.byref(rows), C.byref(blocks)))
        return bool(on.value), rows.value, blocks.value

    def read_structure(self, mat):
        """-> (row extent words: uint64[N], row-block descriptors: uint32[nblk, 4]), the stored codewords as they are"""
        _, rows, blocks = self._structure_info(mat)
        ext = np.zeros(rows, dtype=np.uint64)
        blk = np.zeros((blocks, 4), dtype=np.uint32)
        check(self.L.abft_hip_matrix_read_structure(mat.h, ext.ctypes.data, blk.ctypes.data))
        return ext, blk

    def write_structure(self, mat, rowext=None, blk=None):
        """store the given words as they are (the shapes read_structure returns): a fault injector for whole sweeps"""
        _, rows, blocks = self._structure_info(mat)
        ext = None if rowext is None else np.ascontiguousarray(rowext, dtype=np.uint64)
        b4 = None if blk is None else np.ascontiguousarray(blk, dtype=np.uint32)
        if (ext is not None and ext.shape != (rows,)) or (b4 is not None and b4.shape != (blocks, 4)):
            raise ValueError("write_structure wants %d row words and (%d, 4) descriptor words" % (rows, blocks))
        check(self.L.abft_hip_matrix_write_structure(mat.h, None if ext is None else ext.ctypes.data,
                                                     None if b4 is None else b4.ctypes.data))

    def flip_structure(self, mat, kind, index, bits):
        """XOR `bits` into one stored word: kind capi.STRUCT_ROW / "row" (bits 0..63 of row `index`'s word) or
        capi.STRUCT_BLOCK / "block" (bits 0..127 of descriptor `index`)"""
        kind = {"row": capi.STRUCT_ROW, "block": capi.STRUCT_BLOCK}.get(kind, kind)
        b = np.ascontiguousarray(bits, dtype=np.int32)
        check(self.L.abft_hip_inject_structure(mat.h, int(kind), int(index), b.ctypes.data_as(capi.i32p), len(b)))

    def scrub_structure(self, mat):
        """check every row word and every descriptor and write repaired ones back; -> (corrected, uncorrectable).
        Events as after any call that reads a result (FatalEvent on an uncorrectable word)."""
        c, u = C.c_uint32(0), C.c_uint32(0)
        check(self.L.abft_hip_matrix_scrub_structure(self.h, mat.h, C.byref(c), C.byref(u)))
        self._drain()
        return c.value, u.value

    # ---- matrix digests (include/abft_hip.h) ----
    def matrix_segments(self, mat):
        """-> [(name, bytes)]: the stored arrays of the matrix that kernels only read or only repair, in the order
        matrix_digest reports them"""
        n = C.c_int(0)
        check(self.L.abft_hip_matrix_segments(mat.h, None, None, 0, C.byref(n)))
        kinds, nbytes = (C.c_uint32 * max(n.value, 1))(), (C.c_uint64 * max(n.value, 1))()
        check(self.L.abft_hip_matrix_segments(mat.h, kinds, nbytes, n.value, C.byref(n)))
        return [(capi.segment_name(kinds[k]), int(nbytes[k])) for k in range(n.value)]

    def matrix_digest(self, mat):
        """-> {name: digest}, the current D = sum w[i] (2 i + 1) mod 2^64 of every segment (synchronous)"""
        names = [s for s, _ in self.matrix_segments(mat)]
        out = (C.c_uint64 * max(len(names), 1))()
        check(self.L.abft_hip_matrix_digest(self.h, mat.h, out, len(names)))
        return {s: int(out[k]) for k, s in enumerate(names)}

    def arm_matrix(self, mat):
        """take the current digests as the reference verify_matrix / verify_matrix_dev compare with; arming again
        takes a new reference"""
        check(self.L.abft_hip_matrix_digest_arm(self.h, mat.h))
        mat.digest_armed = True

    def verify_matrix(self, mat):
        """recompute the digests and compare (synchronous) -> the names of the segments that differ, [] when clean;
        AbftError on a matrix that is not armed"""
        n = C.c_int(0)
        bad = (C.c_uint32 * capi.SEG_COUNT)()
        check(self.L.abft_hip_matrix_verify(self.h, mat.h, C.byref(n), bad, capi.SEG_COUNT))
        self.matrix_verifications += 1
        return [capi.segment_name(bad[k]) for k in range(min(n.value, capi.SEG_COUNT))]

    def verify_matrix_dev(self, mat):
        """the same as two launches on the stream, nothing else (capturable): one (EV_MATRIX_DIGEST, segment kind, 0)
        event per differing segment arrives with the next drain, fatal"""
        self._enqueue_verify(mat)
        self.matrix_verifications += 1

    def _enqueue_verify(self, mat):
        # not counted: the device loops count per batch (a captured call runs once per replay, not once per call)
        check(self.L.abft_hip_matrix_verify_dev(self.h, mat.h))

    def read_segment(self, mat, name):
        """-> the segment's bytes as stored (uint8[bytes], padding included)"""
        size = dict(self.matrix_segments(mat)).get(name)
        if size is None:
            raise ValueError("the matrix has no segment %r" % (name,))
        buf = np.zeros(size, dtype=np.uint8)
        check(self.L.abft_hip_matrix_read_segment(self.h, mat.h, capi.segment_kind(name), buf.ctypes.data, size))
        return buf

    def flip_segment(self, mat, name, word, bits):
        """XOR `bits` (0..31) into stored 32-bit word `word` of the segment: the injector for arrays no other
        injector reaches.  A raw write: nothing else follows it, the armed digests least of all"""
        b = np.ascontiguousarray(bits, dtype=np.int32)
        check(self.L.abft_hip_matrix_flip_segment(self.h, mat.h, capi.segment_kind(name), int(word),
                                                  b.ctypes.data_as(capi.i32p), len(b)))

    # ---- vectors ----------------------------------------------------------
    def create_vector(self, N):
        h = C.c_void_p()
        check(self.L.abft_hip_vector_create(self.h, N, C.byref(h)))
        v = Vector(self, h, N)
        self._live.append(v)
        return v

    def create_block(self, N, K):
        """a block vector of N rows and K columns (1 <= K <= 8): one vector of N*K entries, row-major"""
        if not 1 <= K <= capi.MAX_RHS:
            raise ValueError("K = %d outside [1, %d]" % (K, capi.MAX_RHS))
        v = self.create_vector(N * K)
        v.K = K
        return v

    def view_vector(self, parent, offset, N):
        h = C.c_void_p()
        check(self.L.abft_hip_vector_view(parent.h, offset, N, C.byref(h)))
        v = Vector(self, h, N)
        self._live.append(v)
        return v

    def destroy_vector(self, vec):
        check(self.L.abft_hip_vector_destroy(vec.h))
        vec.h = None
        self._live = [o for o in self._live if o is not vec]

    def map_vector(self, v):
        """-> numpy view of the pinned staging buffer (valid until unmap)."""
        p = capi.f64p()
        check(self.L.abft_hip_vector_map(v.h, C.byref(p)))
        self._drain()
        if v.N == 0:
            return np.empty(0)
        return np.ctypeslib.as_array(p, shape=(v.N,))

    def unmap_vector(self, v, h):
        if v.N:
            check(self.L.abft_hip_vector_unmap(v.h, h.ctypes.data_as(capi.f64p)))

    def copy_vector(self, dst, src):
        check(self.L.abft_hip_vector_copy(dst.h, src.h))

    def upload(self, v, array):
        """array: (N,), or (N, K) for a block vector (stored row-major)"""
        h = self.map_vector(v)
        h[:] = np.ascontiguousarray(array, dtype=np.float64).reshape(-1)
        self.unmap_vector(v, h)

    def download(self, v):
        """-> (N,), or (N, K) for a block vector made by create_block"""
        h = self.map_vector(v)
        out = h.copy()
        return out.reshape(-1, v.K) if v.K else out

    # ---- kernels ----------------------------------------------------------
    def dot(self, a, b):
        r = C.c_double()
        check(self.L.abft_hip_dot(self.h, a.h, b.h, C.byref(r)))
        self._drain_if_pending()
        return r.value

    def calc_xr(self, x, r, p, w, alpha):
        out = C.c_double()
        check(self.L.abft_hip_calc_xr(self.h, x.h, r.h, p.h, w.h, alpha, C.byref(out)))
        self._drain_if_pending()
        return out.value

    def calc_p(self, p, r, beta):
        check(self.L.abft_hip_calc_p(self.h, p.h, r.h, beta))

    def spmv(self, mat, vec, result, part=capi.PART_ALL):
        if part == capi.PART_ALL:
            check(self.L.abft_hip_spmv(self.h, mat.h, vec.h, result.h))
        else:
            check(self.L.abft_hip_spmv_part(self.h, mat.h, vec.h, result.h, part))

    # ---- block right-hand sides (K columns per call; include/abft_hip.h) ----
    def spmm(self, mat, X, Y, k, drain=True):
        """Y = A X for k columns, one pass over the matrix.  Events as after spmv: drained and
        printed (FatalEvent on a fatal one) -- at once, or with drain=False by the next call
        that reads a result (the CG loop's dot_block), as the spmv of cg_solve is."""
        check(self.L.abft_hip_spmm(self.h, mat.h, X.h, Y.h, k))
        if drain:
            self._drain()

    def dot_block(self, a, b, k):
        """-> np.ndarray of k dots a[:, j] . b[:, j]"""
        out = np.zeros(k)
        check(self.L.abft_hip_dot_block(self.h, a.h, b.h, k, out.ctypes.data_as(capi.f64p)))
        self._drain_if_pending()
        return out

    def calc_xr_block(self, x, r, p, w, k, alpha, active):
        """x[:, j] += alpha[j] p[:, j]; r[:, j] -= alpha[j] w[:, j] for the columns j set in `active`
        (bit mask); -> np.ndarray of k values r[:, j] . r[:, j]"""
        a = np.zeros(capi.MAX_RHS)
        a[:k] = alpha
        out = np.zeros(k)
        check(self.L.abft_hip_calc_xr_block(self.h, x.h, r.h, p.h, w.h, k, a.ctypes.data_as(capi.f64p), int(active),
                                            out.ctypes.data_as(capi.f64p)))
        self._drain_if_pending()
        return out

    def calc_p_block(self, p, r, k, beta, active):
        """p[:, j] = r[:, j] + beta[j] p[:, j] for the columns j set in `active`"""
        b = np.zeros(capi.MAX_RHS)
        b[:k] = beta
        check(self.L.abft_hip_calc_p_block(self.h, p.h, r.h, k, b.ctypes.data_as(capi.f64p), int(active)))

    # ---- the fused block iteration (include/abft_hip.h): cg_solve_block(..., fused=True) ----
    def spmm_dot(self, mat, P, W, k, drain=True):
        """W = A P as spmm, and -> np.ndarray of the k products P[:, j] . W[:, j], formed inside the
        SpMM from W's rows (no separate dot pass).  The sums are read here, so events pending after
        the call are drained as after dot_block; drain=True drains in any case, as spmm does."""
        out = np.zeros(k)
        check(self.L.abft_hip_spmm_dot(self.h, mat.h, P.h, W.h, k, out.ctypes.data_as(capi.f64p)))
        if drain:
            self._drain()
        else:
            self._drain_if_pending()
        return out

    def calc_r_block(self, R, W, k, alpha, active, dinv=None):
        """R[:, j] -= alpha[j] W[:, j] for the columns set in `active`; -> rr[k], or with dinv
        (rz[k], rr[k]), of every column: the bits calc_xr_block / calc_xr_precond_block give"""
        a = np.zeros(capi.MAX_RHS)
        a[:k] = alpha
        if dinv is None:
            out = np.zeros(k)
            check(self.L.abft_hip_calc_r_block(self.h, R.h, W.h, k, a.ctypes.data_as(capi.f64p), int(active),
                                               out.ctypes.data_as(capi.f64p)))
            self._drain_if_pending()
            return out
        out = np.zeros(2 * k)
        check(self.L.abft_hip_calc_r_precond_block(self.h, R.h, W.h, dinv.h, k, a.ctypes.data_as(capi.f64p),
                                                   int(active), out.ctypes.data_as(capi.f64p)))
        self._drain_if_pending()
        return out[0::2].copy(), out[1::2].copy()

    def calc_px_block(self, X, P, R, k, alpha, beta, active, dinv=None):
        """for the columns set in `active`: X[:, j] += alpha[j] P[:, j], then P[:, j] = R[:, j] + beta[j] P[:, j]
        (with dinv: dinv * R[:, j] in R[:, j]'s place), P read once"""
        a = np.zeros(capi.MAX_RHS)
        a[:k] = alpha
        b = np.zeros(capi.MAX_RHS)
        b[:k] = beta
        if dinv is None:
            check(self.L.abft_hip_calc_px_block(self.h, X.h, P.h, R.h, k, a.ctypes.data_as(capi.f64p),
                                                b.ctypes.data_as(capi.f64p), int(active)))
        else:
            check(self.L.abft_hip_calc_px_precond_block(self.h, X.h, P.h, R.h, dinv.h, k, a.ctypes.data_as(capi.f64p),
                                                        b.ctypes.data_as(capi.f64p), int(active)))

    # ---- residual checks (include/abft_hip.h) ----
    def flip_vector(self, v, index, bits):
        """XOR the given bits (0-63) into the double v[index] (for a block vector: row * K + column)"""
        b = np.ascontiguousarray(bits, dtype=np.int32)
        check(self.L.abft_hip_vector_flip(v.h, int(index), b.ctypes.data_as(capi.i32p), len(b)))

    def residual_gap(self, mat, b, x, r, scratch):
        """scratch = A x; -> (sum ((b - Ax) - r)^2, sum (b - Ax)^2).  Events as after spmv + dot."""
        out = np.zeros(2)
        check(self.L.abft_hip_residual_gap(self.h, mat.h, b.h, x.h, r.h, scratch.h, out.ctypes.data_as(capi.f64p)))
        self._drain_if_pending()
        return float(out[0]), float(out[1])

    def residual_restart(self, mat, b, x, r, p, scratch):
        """r = b - A x, p = r; -> r . r (the bits dot(r, r) gives)"""
        out = C.c_double()
        check(self.L.abft_hip_residual_restart(self.h, mat.h, b.h, x.h, r.h, p.h, scratch.h, C.byref(out)))
        self._drain_if_pending()
        return out.value

    def residual_gap_block(self, mat, B, X, R, scratch, k, active):
        """-> (gap2[k], tt2[k]) for the columns set in `active` (0.0 elsewhere)"""
        out = np.zeros(2 * k)
        check(self.L.abft_hip_residual_gap_block(self.h, mat.h, B.h, X.h, R.h, scratch.h, k, int(active),
                                                 out.ctypes.data_as(capi.f64p)))
        self._drain_if_pending()
        return out[0::2].copy(), out[1::2].copy()

    def residual_restart_block(self, mat, B, X, R, P, scratch, k, mask):
        """R[:, j] = B[:, j] - (A X)[:, j], P[:, j] = R[:, j] for the columns set in `mask`;
        -> np.ndarray of k values R[:, j] . R[:, j] (every column)"""
        out = np.zeros(k)
        check(self.L.abft_hip_residual_restart_block(self.h, mat.h, B.h, X.h, R.h, P.h, scratch.h, k, int(mask),
                                                     out.ctypes.data_as(capi.f64p)))
        self._drain_if_pending()
        return out

    def copy_block(self, dst, src, k, mask):
        """dst[:, j] = src[:, j] for the columns set in `mask`"""
        check(self.L.abft_hip_copy_block(self.h, dst.h, src.h, k, int(mask)))

    # ---- protected vectors (include/abft_hip.h) ----
    def encode_vector(self, v):
        """v[i] <- the (64, 57) codeword of v[i], in place (the double loses its low 7 mantissa bits)"""
        check(self.L.abft_hip_vector_encode(self.h, v.h))

    def scrub_vector(self, v):
        """check every word of v and write repaired ones back; -> (corrected, uncorrectable).  Events as
        after any call that reads a result (FatalEvent on an uncorrectable word)."""
        c, u = C.c_int(0), C.c_int(0)
        check(self.L.abft_hip_vector_scrub(self.h, v.h, C.byref(c), C.byref(u)))
        self._drain()
        return c.value, u.value

    def spmv_vecc(self, mat, vec, result):
        check(self.L.abft_hip_spmv_vecc(self.h, mat.h, vec.h, result.h))

    def dot_vecc(self, a, b):
        r = C.c_double()
        check(self.L.abft_hip_dot_vecc(self.h, a.h, b.h, C.byref(r)))
        self._drain_if_pending()
        return r.value

    def calc_xr_vecc(self, x, r, p, w, alpha):
        out = C.c_double()
        check(self.L.abft_hip_calc_xr_vecc(self.h, x.h, r.h, p.h, w.h, alpha, C.byref(out)))
        self._drain_if_pending()
        return out.value

    def calc_p_vecc(self, p, r, beta):
        check(self.L.abft_hip_calc_p_vecc(self.h, p.h, r.h, beta))

    def calc_r_vecc(self, r, w, alpha):
        """calc_xr_vecc's r half on its own: r -= alpha w on codewords -> r.r over the stored r (abft_hip_calc_r_vecc;
        operands 0: r, 1: w).  With calc_px_vecc behind it: what calc_xr_vecc + calc_p_vecc leave, p read once"""
        out = C.c_double()
        check(self.L.abft_hip_calc_r_vecc(self.h, r.h, w.h, alpha, C.byref(out)))
        self._drain_if_pending()
        return out.value

    def calc_px_vecc(self, x, p, r, alpha, beta):
        """x += alpha p and p = r + beta p on codewords, in one pass over the old p (abft_hip_calc_px_vecc; operands
        0: x, 1: p, 2: r)"""
        check(self.L.abft_hip_calc_px_vecc(self.h, x.h, p.h, r.h, alpha, beta))

    def precond_start_vecc(self, r, dinv, p):
        """p = enc(z), z = val(dinv) * val(r), on codewords -- dinv's too: ctx.jacobi(A, protected=True) --
        -> (r . z, r . r), the second the bits dot_vecc(r, r) gives (abft_hip_precond_start_vecc; operands 0: r,
        1: dinv, 2: p).  A repaired dinv word is stored back: dinv outlives the iteration"""
        out = np.zeros(2)
        check(self.L.abft_hip_precond_start_vecc(self.h, r.h, dinv.h, p.h, out.ctypes.data_as(capi.f64p)))
        self._drain_if_pending()
        return float(out[0]), float(out[1])

    def calc_r_precond_vecc(self, r, w, dinv, alpha):
        """r -= alpha w on codewords -> (r . z, r . r) over the stored r, z = val(dinv) * r
        (abft_hip_calc_r_precond_vecc; operands 0: r, 1: w, 2: dinv)"""
        out = np.zeros(2)
        check(self.L.abft_hip_calc_r_precond_vecc(self.h, r.h, w.h, dinv.h, alpha, out.ctypes.data_as(capi.f64p)))
        self._drain_if_pending()
        return float(out[0]), float(out[1])

    def calc_px_precond_vecc(self, x, p, r, dinv, alpha, beta):
        """x += alpha p and p = dinv r + beta p on codewords, in one pass over the old p
        (abft_hip_calc_px_precond_vecc; operands 0: x, 1: p, 2: r, 3: dinv)"""
        check(self.L.abft_hip_calc_px_precond_vecc(self.h, x.h, p.h, r.h, dinv.h, alpha, beta))

    # ---- protected block vectors (include/abft_hip.h): cg_solve_block(..., vector_ecc=True) ----
    def spmm_dot_vecc(self, mat, P, W, k, drain=True):
        """spmm_dot on codewords: W = enc(A val(P)) -> np.ndarray of the k products val(P[:, j]) . strip(W[:, j])
        (abft_hip_spmm_dot_vecc; operand 0: P, not written back).  Events as after spmm_dot."""
        out = np.zeros(k)
        check(self.L.abft_hip_spmm_dot_vecc(self.h, mat.h, P.h, W.h, k, out.ctypes.data_as(capi.f64p)))
        if drain:
            self._drain()
        else:
            self._drain_if_pending()
        return out

    def dot_block_vecc(self, a, b, k):
        """-> np.ndarray of k dots val(a[:, j]) . val(b[:, j]) (abft_hip_dot_block_vecc; operands 0: a, 1: b)"""
        out = np.zeros(k)
        check(self.L.abft_hip_dot_block_vecc(self.h, a.h, b.h, k, out.ctypes.data_as(capi.f64p)))
        self._drain_if_pending()
        return out

    def calc_r_block_vecc(self, R, W, k, alpha, active):
        """calc_r_block on codewords: R[:, j] = enc(val(R) - alpha[j] val(W)) in the columns set in `active`
        -> rr[k] over the stored R of every column (abft_hip_calc_r_block_vecc; operands 0: R, 1: W)"""
        a = np.zeros(capi.MAX_RHS)
        a[:k] = alpha
        out = np.zeros(k)
        check(self.L.abft_hip_calc_r_block_vecc(self.h, R.h, W.h, k, a.ctypes.data_as(capi.f64p), int(active),
                                                out.ctypes.data_as(capi.f64p)))
        self._drain_if_pending()
        return out

    def calc_px_block_vecc(self, X, P, R, k, alpha, beta, active):
        """calc_px_block on codewords, in the columns set in `active`: X = enc(val(X) + alpha[j] val(P)) and
        P = enc(val(R) + beta[j] val(P)), both from the old P (abft_hip_calc_px_block_vecc; operands 0: X, 1: P, 2: R)"""
        a = np.zeros(capi.MAX_RHS)
        a[:k] = alpha
        b = np.zeros(capi.MAX_RHS)
        b[:k] = beta
        check(self.L.abft_hip_calc_px_block_vecc(self.h, X.h, P.h, R.h, k, a.ctypes.data_as(capi.f64p),
                                                 b.ctypes.data_as(capi.f64p), int(active)))

    def vecc_supported(self, mat):
        """spmv_vecc runs on CSR matrices in the streaming layout only"""
        return mat.fmt == FMT_CSR and self.matrix_info(mat)[0] == "stream"

    # ---- Jacobi preconditioning (include/abft_hip.h) ----
    def jacobi(self, mat, strict=True, protected=False):
        """-> a new Vector dinv, dinv[i] = 1 / (sum of the diagonal elements of row i), the Jacobi
        preconditioner of cg_solve(..., precond=dinv).  Rows without a positive finite diagonal get 1.0;
        their number is dinv.bad, and with strict they raise ValueError (Jacobi wants a positive diagonal).
        protected=True encodes dinv in place (encode_vector) and sets dinv.protected = True: the preconditioner
        of cg_solve / cg_solve_device(..., vector_ecc=True, precond=dinv), and of those only."""
        dinv = self.create_vector(mat.n_out)
        bad = C.c_uint32(0)
        try:
            check(self.L.abft_hip_matrix_diag_inverse(self.h, mat.h, dinv.h, C.byref(bad)))
        except capi.AbftError:
            self.destroy_vector(dinv)
            raise
        dinv.bad = bad.value
        if strict and bad.value:
            self.destroy_vector(dinv)
            raise ValueError("jacobi: %d of %d rows have no positive finite diagonal (strict=False sets their "
                             "entries to 1.0)" % (bad.value, mat.n_out))
        if protected:
            self.encode_vector(dinv)
            dinv.protected = True
        return dinv

    def precond_start(self, r, dinv, p):
        """p = z = dinv * r; -> (r . z, r . r), the second the bits dot(r, r) gives"""
        out = np.zeros(2)
        check(self.L.abft_hip_precond_start(self.h, r.h, dinv.h, p.h, out.ctypes.data_as(capi.f64p)))
        self._drain_if_pending()
        return float(out[0]), float(out[1])

    def calc_xr_precond(self, x, r, p, w, dinv, alpha):
        """x += alpha p; r -= alpha w; -> (r . z, r . r) of the new r, z = dinv * r"""
        out = np.zeros(2)
        check(self.L.abft_hip_calc_xr_precond(self.h, x.h, r.h, p.h, w.h, dinv.h, alpha,
                                              out.ctypes.data_as(capi.f64p)))
        self._drain_if_pending()
        return float(out[0]), float(out[1])

    def calc_p_precond(self, p, r, dinv, beta):
        """p = dinv * r + beta p"""
        check(self.L.abft_hip_calc_p_precond(self.h, p.h, r.h, dinv.h, beta))

    def precond_start_block(self, R, dinv, P, k, mask):
        """P[:, j] = dinv * R[:, j] for the columns set in `mask`; -> (rz[k], rr[k]) of every column"""
        out = np.zeros(2 * k)
        check(self.L.abft_hip_precond_start_block(self.h, R.h, dinv.h, P.h, k, int(mask),
                                                  out.ctypes.data_as(capi.f64p)))
        self._drain_if_pending()
        return out[0::2].copy(), out[1::2].copy()

    def calc_xr_precond_block(self, x, r, p, w, dinv, k, alpha, active):
        """calc_xr_block with one dinv for all columns; -> (rz[k], rr[k]) of every column"""
        a = np.zeros(capi.MAX_RHS)
        a[:k] = alpha
        out = np.zeros(2 * k)
        check(self.L.abft_hip_calc_xr_precond_block(self.h, x.h, r.h, p.h, w.h, dinv.h, k, a.ctypes.data_as(capi.f64p),
                                                    int(active), out.ctypes.data_as(capi.f64p)))
        self._drain_if_pending()
        return out[0::2].copy(), out[1::2].copy()

    def calc_p_precond_block(self, p, r, dinv, k, beta, active):
        """p[:, j] = dinv * r[:, j] + beta[j] p[:, j] for the columns j set in `active`"""
        b = np.zeros(capi.MAX_RHS)
        b[:k] = beta
        check(self.L.abft_hip_calc_p_precond_block(self.h, p.h, r.h, dinv.h, k, b.ctypes.data_as(capi.f64p),
                                                   int(active)))

    def matrix_info(self, mat):
        """-> (layout: 'stream' | 'panels' | 'sweep' | 'slice', kernel launches per spmv) -- measurement only"""
        lay, n = C.c_int(0), C.c_int(0)
        check(self.L.abft_hip_matrix_info(mat.h, C.byref(lay), C.byref(n)))
        return ("stream", "panels", "sweep", "slice")[lay.value], n.value

    def packed_stats(self, mat):
        """-> (packed row blocks, those staged without per-element bound tests, those of them whose equal-length rows
        are also summed without clamps) -- measurement and tests only (include/abft_hip.h, abft_hip_packed_stats)"""
        p, s, r = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(self.L.abft_hip_packed_stats(mat.h, C.byref(p), C.byref(s), C.byref(r)))
        return p.value, s.value, r.value

    def set_interior(self, mat, row_lo, row_hi):
        """rows [row_lo, row_hi) read nothing a peer still has to send (include/abft_hip.h)"""
        check(self.L.abft_hip_matrix_set_interior(mat.h, row_lo, row_hi))

    def inject_bitflip(self, mat, kind, num_flips):
        """reference CSR/CPUContext.cpp:135-159 / COO/CPUContext.cpp:123-140: the
        1 + num_flips rand() draws happen here on the host, in that order."""
        kind = self.BITFLIP.get(kind, kind)
        rand = self.rng or _libc_rand
        index = rand() % mat.nnz
        if mat.fmt == FMT_CSR:
            start, end = (0, 64) if kind == capi.FLIP_VALUE else (64, 96) if kind == capi.FLIP_INDEX else (0, 96)
        else:
            start, end = (64, 128) if kind == capi.FLIP_VALUE else (0, 64) if kind == capi.FLIP_INDEX else (0, 128)
        bits = []
        for _ in range(num_flips):
            bit = rand() % (end - start) + start
            sys.stdout.write("*** flipping bit %d at index %d ***\n" % (bit, index))
            bits.append(bit)
        self.inject_at(mat, index, bits)
        return index, bits

    def inject_at(self, mat, index, bits):
        b = np.ascontiguousarray(bits, dtype=np.int32)
        check(self.L.abft_hip_inject(mat.h, index, b.ctypes.data_as(capi.i32p), len(b)))

    # ---- events -----------------------------------------------------------
    def synchronize(self):
        check(self.L.abft_hip_synchronize(self.h))

    def drain_events(self):
        """-> ([(kind, index, bit)], fatal) -- raw, nothing printed."""
        if self._evbuf is None:  # sized to the device queue: drain never truncates
            self._evcap = self.L.abft_hip_event_capacity()
            self._evbuf = (capi.Event * self._evcap)()
        n, fatal = C.c_int(0), C.c_int(0)
        check(self.L.abft_hip_drain_events(self.h, self._evbuf, self._evcap, C.byref(n), C.byref(fatal)))
        return [self._evbuf[i].tup() for i in range(n.value)], bool(fatal.value)

    def _drain_if_pending(self):
        if self.L.abft_hip_pending_events(self.h):
            self._drain()

    def _drain(self):
        events, fatal = self.drain_events()
        self._report(events, fatal)

    def _report(self, events, fatal):
        """events [(kind, index, bit)] as a drain hands them over: logged, then on_event's, or printed (FatalEvent on
        a fatal one)"""
        if not events:
            return
        self.event_log.extend(events)
        if self.on_event is not None:
            self.on_event(events, fatal)
            return
        for k, i, b in events:
            sys.stdout.write(capi.format_event(k, i, b, self.fmt))
        if fatal:
            sys.stdout.flush()
            raise FatalEvent(events)

    # ---- measurement ------------------------------------------------------
    def profile(self, mask=0xF, stride=1):
        """bit k of mask brackets kernel k (capi.K_*) with HIP events, every
        `stride`-th launch of it; 0 = off"""
        self.prof_mask = 0xF if mask is True else int(mask)
        check(self.L.abft_hip_profile_stride(self.h, stride))
        check(self.L.abft_hip_profile_enable(self.h, self.prof_mask))
        check(self.L.abft_hip_profile_reset(self.h))

    def profile_read(self, kernel):
        ms, n = C.c_double(), C.c_long()
        check(self.L.abft_hip_profile_read(self.h, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def stream_probe(self, nbytes=1 << 30, reps=10):
        c, r = C.c_double(), C.c_double()
        check(self.L.abft_hip_stream_probe(self.h, nbytes, reps, C.byref(c), C.byref(r)))
        return c.value, r.value

    def tail_stats(self):
        """what the last abft_hip_cg_iteration_dev ran behind its SpMV -> (path, grid, want, counts[4]): path 0 the three
        kernels, 1 / 2 / 3 the one launch as cg_tail_kernel<1, false> / <2, false> / <2, true> (include/abft_hip.h)"""
        path, grid, want = C.c_int(0), C.c_int(0), C.c_int(0)
        counts = (C.c_long * 4)()
        check(self.L.abft_hip_tail_stats(self.h, C.byref(path), C.byref(grid), C.byref(want), counts))
        return path.value, grid.value, want.value, list(counts)

    def x_in_spmv_stats(self):
        """x updates left pending on the old p by calc_p -> (absorbed, flushed): applied by the SpMV that followed, or
        on their own because something else came first (abft_hip_x_in_spmv_stats, include/abft_hip.h)"""
        absorbed, flushed = C.c_long(0), C.c_long(0)
        check(self.L.abft_hip_x_in_spmv_stats(self.h, C.byref(absorbed), C.byref(flushed)))
        return absorbed.value, flushed.value

    def lazy_x_stats(self):
        """the queue of x updates (ABFT_HIP_LAZY_X) -> (bursts, applied_in_bursts, applied_by_flush): SpMV launches that
        applied a full queue, the updates they applied, and queued updates applied on their own because something other
        than the loop's next call came first (abft_hip_lazy_x_stats, include/abft_hip.h)"""
        b, a, f = C.c_long(0), C.c_long(0), C.c_long(0)
        check(self.L.abft_hip_lazy_x_stats(self.h, C.byref(b), C.byref(a), C.byref(f)))
        return b.value, a.value, f.value

    def ahead_stats(self):
        """kernels of the host-scalar loop run ahead of the scalars -> (committed_p, committed_r, dropped): calc_p / calc_xr
        calls that took one over, and run-aheads thrown away (abft_hip_ahead_stats, include/abft_hip.h)"""
        cp, cr, d = C.c_long(0), C.c_long(0), C.c_long(0)
        check(self.L.abft_hip_ahead_stats(self.h, C.byref(cp), C.byref(cr), C.byref(d)))
        return cp.value, cr.value, d.value

    # ---- the device-scalar loop (include/abft_hip.h): cg_solve_device ----
    def cg_iteration_until_dev(self, mat, vec, x, r, p, w, scalars, rr_at, pw_at, rr_new_at, threshold, vec_offset=0,
                               part=capi.PART_ALL):
        """one guarded CG iteration, enqueue-only (abft_hip_cg_iteration_until_dev): live when scalars[rr_at] >
        threshold on the device, else frozen.  scalars: a vector of device doubles; rr_at, pw_at, rr_new_at: where the
        pairs {r.r, events} read, {p.w, events} and {r.r, events} written start in it"""
        base = scalars.device_ptr
        check(self.L.abft_hip_cg_iteration_until_dev(self.h, mat.h, vec.h, vec_offset, part, x.h, r.h, p.h, w.h,
                                                     base + 8 * rr_at, base + 8 * pw_at, base + 8 * rr_new_at,
                                                     threshold))

    def cg_vecc_iteration_until_dev(self, mat, vec, x, r, p, w, scalars, rr_at, pw_at, rr_new_at, threshold,
                                    vec_offset=0, part=capi.PART_ALL):
        """one guarded CG iteration on protected vectors, enqueue-only (abft_hip_cg_vecc_iteration_until_dev; DESIGN.md
        section 5k): cg_iteration_until_dev's arguments and pairs, the vectors codewords.  Vector events name their
        operand among vec, x, r, p, w = 0 .. 4.  CSR matrices in the streaming layout only"""
        base = scalars.device_ptr
        check(self.L.abft_hip_cg_vecc_iteration_until_dev(self.h, mat.h, vec.h, vec_offset, part, x.h, r.h, p.h, w.h,
                                                          base + 8 * rr_at, base + 8 * pw_at, base + 8 * rr_new_at,
                                                          threshold))

    def pcg_vecc_iteration_until_dev(self, mat, vec, x, r, p, w, dinv, scalars, in_at, pw_at, out_at, threshold,
                                     vec_offset=0, part=capi.PART_ALL):
        """one guarded Jacobi-preconditioned CG iteration on protected vectors, enqueue-only
        (abft_hip_pcg_vecc_iteration_until_dev): pcg_iteration_until_dev's arguments and records,
        the vectors -- dinv too -- codewords.  Vector events name their operand among vec, x, r, p, w, dinv = 0 .. 5.
        Under graph capture it needs one eager precond_start_vecc on the context first"""
        base = scalars.device_ptr
        check(self.L.abft_hip_pcg_vecc_iteration_until_dev(self.h, mat.h, vec.h, vec_offset, part, x.h, r.h, p.h, w.h,
                                                           dinv.h, base + 8 * in_at, base + 8 * pw_at,
                                                           base + 8 * out_at, threshold))

    def pcg_iteration_until_dev(self, mat, vec, x, r, p, w, dinv, scalars, in_at, pw_at, out_at, threshold,
                                vec_offset=0, part=capi.PART_ALL):
        """one guarded Jacobi-preconditioned CG iteration, enqueue-only (abft_hip_pcg_iteration_until_dev; DESIGN.md
        section 5g): live when scalars[in_at] > threshold on the device, else frozen.  scalars: a vector of device
        doubles; in_at, out_at: where the records {r.r, events, r.z, 0.0} read and written start in it, pw_at: where
        the pair {p.w, events} goes.  Under graph capture the context must have made a preconditioned call before
        (precond_start): see the header"""
        base = scalars.device_ptr
        check(self.L.abft_hip_pcg_iteration_until_dev(self.h, mat.h, vec.h, vec_offset, part, x.h, r.h, p.h, w.h,
                                                      dinv.h, base + 8 * in_at, base + 8 * pw_at, base + 8 * out_at,
                                                      threshold))

    # ---- the device-scalar loop on a protected trail (include/abft_hip.h) ----
    # The four guarded iterations with their scalars as SECDED slots of two doubles: records of 4 doubles (8 with
    # dinv), the pair 4; rr_at / in_at, pw_at, rr_new_at / out_at count doubles and must be even.
    def cg_trail_iteration_until_dev(self, mat, vec, x, r, p, w, scalars, rr_at, pw_at, rr_new_at, threshold,
                                     vec_offset=0, part=capi.PART_ALL):
        """cg_iteration_until_dev on a protected trail (abft_hip_cg_trail_iteration_until_dev)"""
        base = scalars.device_ptr
        check(self.L.abft_hip_cg_trail_iteration_until_dev(self.h, mat.h, vec.h, vec_offset, part, x.h, r.h, p.h, w.h,
                                                           base + 8 * rr_at, base + 8 * pw_at, base + 8 * rr_new_at,
                                                           threshold))

    def pcg_trail_iteration_until_dev(self, mat, vec, x, r, p, w, dinv, scalars, in_at, pw_at, out_at, threshold,
                                      vec_offset=0, part=capi.PART_ALL):
        """pcg_iteration_until_dev on a protected trail (abft_hip_pcg_trail_iteration_until_dev)"""
        base = scalars.device_ptr
        check(self.L.abft_hip_pcg_trail_iteration_until_dev(self.h, mat.h, vec.h, vec_offset, part, x.h, r.h, p.h, w.h,
                                                            dinv.h, base + 8 * in_at, base + 8 * pw_at,
                                                            base + 8 * out_at, threshold))

    def cg_vecc_trail_iteration_until_dev(self, mat, vec, x, r, p, w, scalars, rr_at, pw_at, rr_new_at, threshold,
                                          vec_offset=0, part=capi.PART_ALL):
        """cg_vecc_iteration_until_dev on a protected trail (abft_hip_cg_vecc_trail_iteration_until_dev)"""
        base = scalars.device_ptr
        check(self.L.abft_hip_cg_vecc_trail_iteration_until_dev(self.h, mat.h, vec.h, vec_offset, part, x.h, r.h, p.h,
                                                                w.h, base + 8 * rr_at, base + 8 * pw_at,
                                                                base + 8 * rr_new_at, threshold))

    def pcg_vecc_trail_iteration_until_dev(self, mat, vec, x, r, p, w, dinv, scalars, in_at, pw_at, out_at, threshold,
                                           vec_offset=0, part=capi.PART_ALL):
        """pcg_vecc_iteration_until_dev on a protected trail (abft_hip_pcg_vecc_trail_iteration_until_dev)"""
        base = scalars.device_ptr
        check(self.L.abft_hip_pcg_vecc_trail_iteration_until_dev(self.h, mat.h, vec.h, vec_offset, part, x.h, r.h, p.h,
                                                                 w.h, dinv.h, base + 8 * in_at, base + 8 * pw_at,
                                                                 base + 8 * out_at, threshold))

    def encode_trail(self, values, first_ordinal=0):
        """n values -> their n slots as 2 n doubles, value i under ordinal first_ordinal + i (abft_hip_trail_encode)"""
        v = np.ascontiguousarray(values, dtype=np.float64)
        out = np.zeros(2 * len(v))
        check(self.L.abft_hip_trail_encode(v.ctypes.data_as(capi.f64p), len(v), int(first_ordinal),
                                           out.ctypes.data_as(capi.f64p)))
        return out

    def decode_trail(self, slots):
        """2 n doubles -> (values[n], status[n], bits[n]): status 0 clean, 1 one flipped bit repaired (bits: which),
        -1 two flips, the value as stored (abft_hip_trail_decode)"""
        s = np.ascontiguousarray(slots, dtype=np.float64)
        n = len(s) // 2
        values, status, bits = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
        check(self.L.abft_hip_trail_decode(s.ctypes.data_as(capi.f64p), n, values.ctypes.data_as(capi.f64p),
                                           status.ctypes.data_as(capi.i32p), bits.ctypes.data_as(capi.i32p)))
        return values, status, bits

    def flip_trail(self, trail, slot, bits):
        """XOR the given bits (0-127, numbered as the COO element's) into slot `slot` of the trail vector"""
        b = np.ascontiguousarray(bits, dtype=np.int32)
        check(self.L.abft_hip_trail_flip(self.h, trail.device_ptr, int(slot), b.ctypes.data_as(capi.i32p), len(b)))

    def trail_inject_at(self, stage, record, ordinal, bits):
        """arm one flip of a slot that lives inside an iteration: the next eager protected guarded call XORs `bits`
        into slot `ordinal` of `record` (capi.TRAIL_START / TRAIL_PW / TRAIL_NEXT) behind its fold (stage 1) or its r
        half (stage 2)"""
        b = np.ascontiguousarray(bits, dtype=np.int32)
        check(self.L.abft_hip_trail_inject_at(self.h, int(stage), int(record), int(ordinal),
                                              b.ctypes.data_as(capi.i32p), len(b)))

    def report_trail(self, slots, rec, stride):
        """the host's view of a downloaded trail of stride + 1 records of `rec` slots and the pair: -> the values, in
        the unprotected trail's layout.  A slot with one flipped bit is reported once, with the device's line (record:
        the pair, else the start record); two flips raise FatalEvent"""
        values, status, bits = self.decode_trail(slots)
        # a codeword in the wrong place -- the ordinal under the code is not the slot's, or word 1 is set --: as two flips
        words = np.ascontiguousarray(slots, dtype=np.float64).view(np.uint32).reshape(-1, 4)
        j = np.arange(len(values))
        ordinals = np.where(j >= rec * (stride + 1), j - rec * (stride + 1), j % rec)
        status = np.where((status == 0) & (((words[:, 0] & 0xFFFFFF) != ordinals) | (words[:, 1] != 0)), -1, status)
        bad = np.flatnonzero(status)
        if len(bad):
            events = []
            for j in bad.tolist():
                pair = j >= rec * (stride + 1)
                ordinal = j - rec * (stride + 1) if pair else j % rec
                where = (capi.TRAIL_PW if pair else capi.TRAIL_START) << 8
                if status[j] > 0:
                    events.append((capi.EV_TRAIL_CORRECTED, ordinal, int(bits[j]) | where))
                else:
                    events.append((capi.EV_TRAIL_DOUBLE, ordinal, where))
                    break
            fatal = events[-1][0] == capi.EV_TRAIL_DOUBLE
            self._report(events, fatal)
            if fatal:
                raise FatalEvent(events)
        return values

    def cg_block_iteration_until_dev(self, mat, X, R, P, W, k, scalars, in_at, pw_at, out_at, threshold, dinv=None):
        """one guarded iteration of the fused block loop, enqueue-only (abft_hip_cg_block_iteration_until_dev; DESIGN.md
        section 5h): column j is live when scalars[in_at + j] > threshold on the device, else frozen.  scalars: a vector
        of device doubles; in_at, out_at: where the records of 2k + 2 doubles {r.r[k], r.z[k], events, 0.0} read and
        written start in it, pw_at: where the k + 1 doubles {P.W[k], events} go.  dinv: the Jacobi vector, or None for
        the plain form.  Under graph capture the context must hold the loop's buffers: block_loop_reserve"""
        base = scalars.device_ptr
        check(self.L.abft_hip_cg_block_iteration_until_dev(self.h, mat.h, X.h, R.h, P.h, W.h,
                                                           None if dinv is None else dinv.h, k, base + 8 * in_at,
                                                           base + 8 * pw_at, base + 8 * out_at, threshold))

    def cg_block_vecc_iteration_until_dev(self, mat, X, R, P, W, k, scalars, in_at, pw_at, out_at, threshold):
        """one guarded iteration of the fused block loop on protected block vectors, enqueue-only
        (abft_hip_cg_block_vecc_iteration_until_dev): cg_block_iteration_until_dev's arguments
        and records without a dinv, the vectors codewords, the records plain doubles.  Vector events name their
        operand as the single guarded entries do -- the gathered P, X, R, P, W = 0 .. 4 -- with index row * k + column.
        CSR matrices in the streaming layout only.  Under graph capture: block_loop_reserve first"""
        base = scalars.device_ptr
        check(self.L.abft_hip_cg_block_vecc_iteration_until_dev(self.h, mat.h, X.h, R.h, P.h, W.h, k, base + 8 * in_at,
                                                                base + 8 * pw_at, base + 8 * out_at, threshold))

    def block_loop_reserve(self, mat, k):
        """allocate what cg_block_iteration_until_dev needs for this matrix, so that it can be captured on a context
        that has not run it yet (abft_hip_block_loop_reserve); not under capture"""
        check(self.L.abft_hip_block_loop_reserve(self.h, mat.h, k))

    # ---- the block loop on a protected trail (include/abft_hip.h) ----
    # Records of 2 (2k + 2) doubles, the tail 2 (k + 1): every word a SECDED slot of two doubles under its ordinal in
    # the record; in_at, pw_at, out_at count doubles and must be even.
    def cg_block_trail_iteration_until_dev(self, mat, X, R, P, W, k, scalars, in_at, pw_at, out_at, threshold,
                                           dinv=None):
        """cg_block_iteration_until_dev on a protected trail (abft_hip_cg_block_trail_iteration_until_dev)"""
        base = scalars.device_ptr
        check(self.L.abft_hip_cg_block_trail_iteration_until_dev(self.h, mat.h, X.h, R.h, P.h, W.h,
                                                                 None if dinv is None else dinv.h, k,
                                                                 base + 8 * in_at, base + 8 * pw_at,
                                                                 base + 8 * out_at, threshold))

    def cg_block_vecc_trail_iteration_until_dev(self, mat, X, R, P, W, k, scalars, in_at, pw_at, out_at, threshold):
        """cg_block_vecc_iteration_until_dev on a protected trail
        (abft_hip_cg_block_vecc_trail_iteration_until_dev)"""
        base = scalars.device_ptr
        check(self.L.abft_hip_cg_block_vecc_trail_iteration_until_dev(self.h, mat.h, X.h, R.h, P.h, W.h, k,
                                                                      base + 8 * in_at, base + 8 * pw_at,
                                                                      base + 8 * out_at, threshold))

    def block_trail_inject_at(self, stage, record, ordinal, bits):
        """trail_inject_at for the two block trail calls, armed apart from it: the next eager one XORs `bits` into
        slot `ordinal` (r.r[j]: j, r.z[j]: k + j, events: 2k; in the tail P.W[j]: j, events: k) of `record` behind
        its fold (stage 1) or its r half (stage 2)"""
        b = np.ascontiguousarray(bits, dtype=np.int32)
        check(self.L.abft_hip_block_trail_inject_at(self.h, int(stage), int(record), int(ordinal),
                                                    b.ctypes.data_as(capi.i32p), len(b)))

    def residual_check_dev(self, mat, b, x, r, scratch, x_ckpt, trail, chk_at, limit):
        """a whole residual check, enqueue-only, its verdict formed and acted on on the device
        (abft_hip_residual_check_dev): scratch = A x, then trail[chk_at .. chk_at + 3] =
        {sum ((b - Ax) - r)^2, sum (b - Ax)^2, verdict, queued events} -- the sums residual_gap returns, verdict 1.0
        when the first is <= limit and both are finite, else 2.0 --, then x_ckpt <- x when it passed, x <- x_ckpt
        when not.  trail: a vector of device doubles.  Under graph capture: residual_check_reserve first"""
        check(self.L.abft_hip_residual_check_dev(self.h, mat.h, b.h, x.h, r.h, scratch.h, x_ckpt.h,
                                                 trail.device_ptr + 8 * chk_at, limit))

    def residual_check_reserve(self):
        """allocate what residual_check_dev needs, so that it can be captured on a context that has made no
        K-wide reduction yet (abft_hip_residual_check_reserve); not under capture"""
        check(self.L.abft_hip_residual_check_reserve(self.h))

    def graph_begin(self):
        """start capturing the asynchronous calls on the context's stream (include/abft_hip.h, graph replay)"""
        check(self.L.abft_hip_graph_begin(self.h))

    def graph_end(self):
        """-> the captured graph (graph_launch, graph_destroy)"""
        g = C.c_void_p()
        check(self.L.abft_hip_graph_end(self.h, C.byref(g)))
        return g

    def graph_launch(self, graph):
        check(self.L.abft_hip_graph_launch(graph))

    def graph_destroy(self, graph):
        check(self.L.abft_hip_graph_destroy(graph))

    @property
    def stream(self):
        return self.L.abft_hip_get_stream(self.h)


_libc = None


def _libc_rand():
    global _libc
    if _libc is None:
        _libc = C.CDLL(None)
    return _libc.rand()


def vecc_strip(array):
    """a downloaded protected vector -> its values: bits 0..6 (the code bits) of every word cleared"""
    words = np.ascontiguousarray(array, dtype=np.float64).view(np.uint64) & np.uint64(0xFFFFFFFFFFFFFF80)
    return words.view(np.float64)


def fdiv(a, b):
    """a / b as the reference's C++ computes it (cg.cpp:102, 109): IEEE-754, so a zero
    denominator gives inf / nan instead of Python's ZeroDivisionError"""
    if b == 0.0:
        a = float(a)
        return float("nan") if a == 0.0 or a != a else float("inf") if (a > 0) == (str(float(b))[0] != "-") else float("-inf")
    return a / b


def threshold_ambiguous(rr, conv_threshold):
    """True when rr lies within rounding of the stop test's threshold (reference cg.cpp:94): the two
    reductions are tree sums, ~1e-13 relative from the reference's serial sums, so only then can the
    iteration count differ from the reference's by one ("iteration-count parity")."""
    return conv_threshold > 0.0 and abs(rr - conv_threshold) <= 1e-12 * abs(rr)


def note_threshold(rr, conv_threshold, state):
    """one stderr line per run when the stop test is ambiguous (stdout stays the reference's)"""
    import sys
    if not state.get("noted") and threshold_ambiguous(rr, conv_threshold):
        state["noted"] = True
        sys.stderr.write("note: threshold-ambiguous run: rr = %s is within 1e-12 (relative) of the convergence "
                         "threshold %.17g; the reference's serially summed rr may fall on the other side and run "
                         "one iteration more or fewer\n" % (float(rr).hex(), conv_threshold))


def _check_passes(gap2, tt2, bb, check_tol):
    """the pass rule: gap2 <= check_tol^2 ||b||^2 with both sums finite (NaN fails the comparison)"""
    return (gap2 <= check_tol * check_tol * bb) and math.isfinite(gap2) and math.isfinite(tt2)


def _ckpt_name(itr):
    return "the start" if itr < 0 else "iteration %d" % itr


def _check_protected_precond(precond, vector_ecc):
    """-> whether precond is a protected dinv (ctx.jacobi(A, protected=True)).  dinv's words must be what the loop's
    kernels read them as: codewords with vector_ecc, plain doubles without -- anything else is refused here"""
    protected = precond is not None and bool(getattr(precond, "protected", False))
    if vector_ecc and precond is not None and not protected:
        raise ValueError("vector_ecc with an unprotected precond: the protected kernels would misread its plain "
                         "doubles as codewords; make it with ctx.jacobi(A, protected=True)")
    if protected and not vector_ecc:
        raise ValueError("a protected precond (ctx.jacobi(A, protected=True)) without vector_ecc: the plain "
                         "preconditioned kernels would multiply with its code bits; pass vector_ecc=True, or make "
                         "the precond with ctx.jacobi(A)")
    return protected


def _refuse_structure_ecc(ctx, A, what):
    """the block solvers read plain row structure (the SpMM kernels): refused before anything runs, and without a call
    on the context (the matrix carries the mark create_matrix gave it; the library refuses such a matrix as well)"""
    if getattr(A, "structure_ecc", False):
        raise ValueError("%s: the matrix was created with structure_ecc=True; block right-hand sides run on "
                         "matrices with a plain row structure" % what)


def _check_args(check_every, check_tol, max_rollbacks):
    if check_every < 0 or int(check_every) != check_every:
        raise ValueError("check_every must be a whole number >= 0, not %r" % (check_every,))
    if not check_tol > 0 or not math.isfinite(check_tol):
        raise ValueError("check_tol must be a positive number, not %r" % (check_tol,))
    if max_rollbacks < 0:
        raise ValueError("max_rollbacks must be >= 0, not %r" % (max_rollbacks,))


class _NoWatch:
    """matrix_check_every=0: the solvers make exactly the calls they make without the keyword"""
    every = 0

    def ran(self, count):
        pass

    def before_check(self):
        pass

    def final(self):
        pass

    def due(self, done, m):
        return False

    def enqueued(self):
        pass

    def final_dev(self):
        pass


_NO_WATCH = _NoWatch()


class _MatrixWatch(_NoWatch):
    """matrix_check_every=M > 0 of the four solvers: the matrix is armed if it is not, and its
    digests are verified on the schedule below.  The hook never looks inside the iteration: it touches no vector and
    no scalar, and the library's digest entries leave the loop's state between calls alone, so a clean run makes the
    launches and computes the bits of the run without it.  `fresh`: a verification has seen the matrix since the last
    iteration ran.

    Host loops: ran(count) behind every iteration (count iterations run so far) verifies when count % M == 0;
    before_check() in front of every residual check, before the checkpoint copy; final() before the solver returns --
    the last two only on a state no verification has seen.  A mismatch is reported as the fatal events
    (EV_MATRIX_DIGEST, segment kind, 0), behind whatever else is queued: FatalEvent, nothing restored.
    Device loops (_device_batches): due(done, m) -- does the batch of m iterations that starts at count `done` reach
    or pass the next multiple of M? -- is known before the batch is enqueued; such a batch has verify_matrix_dev
    behind its last iteration (enqueued() notes it), and its verdict arrives with the batch's download."""

    def __init__(self, ctx, A, every):
        if int(every) != every or every < 0:
            raise ValueError("matrix_check_every must be a whole number >= 0, not %r" % (every,))
        self.ctx, self.A, self.every = ctx, A, int(every)
        self.fresh = False
        if not getattr(A, "digest_armed", False):
            ctx.arm_matrix(A)

    def verify(self):
        bad = self.ctx.verify_matrix(self.A)
        if bad:
            self.ctx._drain()  # what the kernels queued comes first
            self.ctx._report([(capi.EV_MATRIX_DIGEST, capi.segment_kind(s), 0) for s in bad], True)
        self.fresh = True

    def ran(self, count):
        self.fresh = False
        if count % self.every == 0:
            self.verify()

    def before_check(self):
        if not self.fresh:
            self.verify()

    def final(self):
        if not self.fresh:
            self.verify()

    def due(self, done, m):
        self.fresh = False  # a batch of iterations is about to run
        return done + m >= (done // self.every + 1) * self.every

    def enqueued(self):
        self.fresh = True  # (the download behind the batch raises FatalEvent on a mismatch)
        self.ctx.matrix_verifications += 1

    def final_dev(self):
        """a device loop's last batch had no verification: one is enqueued and waited for"""
        if not self.fresh:
            self.ctx.verify_matrix_dev(self.A)
            self.ctx._drain()
            self.fresh = True


def _watch(ctx, A, matrix_check_every):
    return _MatrixWatch(ctx, A, matrix_check_every) if matrix_check_every else _NO_WATCH


def _with_matrix_check(positional, impl):
    """the public form of a host-loop solver: `positional`'s parameters by position or by name, as they have always
    been, and behind them the KEYWORD-ONLY matrix_check_every=0.  inspect.signature follows the wrapper to
    `positional`'s list."""
    @functools.wraps(positional, assigned=("__module__", "__name__", "__qualname__", "__doc__"))
    def solver(*args, matrix_check_every=0, **kw):
        if not matrix_check_every:
            return positional(*args, **kw)
        bound = inspect.signature(positional).bind(*args, **kw)
        bound.apply_defaults()
        return impl(*bound.args, _watch(bound.arguments["ctx"], bound.arguments["A"], matrix_check_every))
    return solver


def cg_solve(ctx, A, b, x, r, p, w, max_itrs=1000, conv_threshold=1e-3, on_iteration=None, check_every=0,
             check_tol=1e-7, max_rollbacks=3, x_ckpt=None, on_check=None, precond=None, vector_ecc=False):
    """cg_solve(ctx, A, b, x, r, p, w, max_itrs=1000, conv_threshold=1e-3, on_iteration=None, check_every=0,
    check_tol=1e-7, max_rollbacks=3, x_ckpt=None, on_check=None, precond=None, vector_ecc=False, *, matrix_check_every=0)

    The reference driver's CG loop, call for call (cg.cpp:87-118).

    check_every > 0 adds residual checks: after iteration i when (i + 1) %
    check_every == 0, and whenever the loop is about to stop on a state no check has seen, the
    recurrence's r is compared with b - A x (ctx.residual_gap, w as the scratch vector).  A check passes
    when ||b - A x - r|| <= check_tol ||b||; then x is copied to the checkpoint x_ckpt (a vector of x's
    length, made here when None).  A failed check copies the checkpoint back into x and restarts the
    recurrence from it (r = b - A x, p = r: ctx.residual_restart).  More than max_rollbacks failures, or a
    failure at max_itrs, raise ResidualCheckFailed.  on_check(itr, gap, ok, rolled_back_to): itr the
    iteration the check follows (-1: the start), gap = ||b - A x - r||, rolled_back_to the iteration of
    the restored checkpoint (-1: the start) or None.  itr counts every iteration run, repeated ones
    included.  With check_every=0 the calls are exactly the loop's above.

    precond: a vector dinv (ctx.jacobi(A)) turns the loop into Jacobi-preconditioned CG (DESIGN.md section
    5d): z = dinv * r is formed inside precond_start / calc_xr_precond / calc_p_precond, which replace
    copy p <- r + dot, calc_xr and calc_p; alpha = r.z / p.w, beta = r.z_new / r.z.  The stop test, on_iteration
    and the residual checks stay on r.r and on r against b - A x (neither depends on M); a restart is followed
    by precond_start on the restarted r.  With precond=None the calls are exactly those without it.

    vector_ecc=True runs the loop on protected vectors: b and x are encoded in place,
    once; r <- b is a copy of codewords that is scrubbed at once (b is read there and nowhere else: a flip
    in it is repaired in r, reported, and left in b); the loop makes the same calls in their protected
    forms (spmv_vecc, dot_vecc, calc_xr_vecc, calc_p_vecc), each of which repairs a flipped bit of any
    operand in registers; x and b are scrubbed before returning, so what the caller downloads is repaired
    (vecc_strip gives the values).  Stop test, on_iteration and the return value are as without it; a word
    with two flipped bits raises FatalEvent.  Refused (ValueError, before anything runs) with check_every > 0
    and for a matrix spmv_vecc does not run on: those kernels write unencoded vectors.
    With vector_ecc=False the calls are exactly those made without the argument.

    vector_ecc=True with precond=ctx.jacobi(A, protected=True) is Jacobi-preconditioned CG on protected vectors
    (DESIGN.md section 5l), dinv under the code like the rest: the same start up to the scrub of r, then
    rz, rr = precond_start_vecc(r, dinv, p), and per iteration spmv_vecc, dot_vecc(p, w),
    rz_new, rr = calc_r_precond_vecc(r, w, dinv, rz / pw) and calc_px_precond_vecc(x, p, r, dinv, alpha, rz_new / rz);
    x, b and dinv are scrubbed before returning.  A precond that is not marked protected is refused with
    vector_ecc (its plain doubles would be misread as codewords), a protected one without it (ValueError, before
    anything runs).

    matrix_check_every=M > 0 (keyword-only) verifies the matrix's digests as the loop runs:
    the residual checks compare r with b - A x through the same A, so they cannot see a damaged A; this can.  The
    matrix is armed (ctx.arm_matrix) if it is not.  A verification (ctx.verify_matrix) follows every iteration i with
    (i + 1) % M == 0, behind on_iteration; with check_every > 0 one also runs in front of EVERY residual check, before
    the checkpoint copy; and one runs before the solver returns -- the last two on a state no verification has seen
    yet.  So no checkpoint is taken and no check trusted on a matrix that has not just been verified.  A mismatch is
    fatal like a double-bit error: the line "[ABFT] matrix digest mismatch in segment NAME" per segment and
    FatalEvent; nothing is restored, the caller re-creates the matrix.  Works with precond and vector_ecc, on every
    layout, format and mode.  ctx.matrix_verifications counts the verifications.  With matrix_check_every=0 the calls
    are exactly those made without the keyword."""
    return _cg_solve(ctx, A, b, x, r, p, w, max_itrs, conv_threshold, on_iteration, check_every, check_tol, max_rollbacks,
                     x_ckpt, on_check, precond, vector_ecc, _NO_WATCH)


def _cg_solve(ctx, A, b, x, r, p, w, max_itrs, conv_threshold, on_iteration, check_every, check_tol, max_rollbacks,
              x_ckpt, on_check, precond, vector_ecc, watch):
    """cg_solve's body; watch: _NO_WATCH, or the _MatrixWatch of matrix_check_every"""
    _check_args(check_every, check_tol, max_rollbacks)
    if vector_ecc and check_every:
        raise ValueError("vector_ecc with check_every > 0: the residual kernels write unencoded vectors")
    _check_protected_precond(precond, vector_ecc)
    if vector_ecc:
        if not ctx.vecc_supported(A):
            raise ValueError("vector_ecc needs a CSR matrix in the streaming layout (this one: %s)"
                             % ("COO" if A.fmt != FMT_CSR else ctx.matrix_info(A)[0]))
        return _cg_solve_vecc(ctx, A, b, x, r, p, w, max_itrs, conv_threshold, on_iteration, precond, watch)
    ctx.copy_vector(r, b)
    rz = None
    if precond is None:
        ctx.copy_vector(p, r)
        rr = ctx.dot(r, r)
    else:
        rz, rr = ctx.precond_start(r, precond, p)
    itr = 0
    noted = {}
    note_threshold(rr, conv_threshold, noted)
    if check_every:
        bb = rr  # r = b: ||b||^2
        own_ckpt = x_ckpt is None
        if own_ckpt:
            x_ckpt = ctx.create_vector(x.N)
        ctx.copy_vector(x_ckpt, x)
        st = dict(checked=False, ckpt=-1, fails=0, records=[])

        def check():
            nonlocal rr, rz
            watch.before_check()
            gap2, tt2 = ctx.residual_gap(A, b, x, r, w)
            ok = _check_passes(gap2, tt2, bb, check_tol)
            gap = math.sqrt(gap2) if gap2 >= 0 else gap2
            back = None
            if ok:
                ctx.copy_vector(x_ckpt, x)
                st["ckpt"] = itr - 1
            else:
                st["fails"] += 1
                back = st["ckpt"]
                ctx.copy_vector(x, x_ckpt)
                rr = ctx.residual_restart(A, b, x, r, p, w)
                if precond is not None:
                    rz, rr = ctx.precond_start(r, precond, p)  # p = z of the restarted r
                note_threshold(rr, conv_threshold, noted)
            st["checked"] = True
            st["records"].append((itr - 1, gap, ok, back))
            if on_check is not None:
                on_check(itr - 1, gap, ok, back)
            if not ok and (st["fails"] > max_rollbacks or itr >= max_itrs):
                raise ResidualCheckFailed(
                    "residual check failed at iteration %d (gap %.3e > %.3e) %s; x holds the checkpoint of %s"
                    % (itr - 1, gap, check_tol * math.sqrt(bb),
                       "after %d rollbacks" % (st["fails"] - 1) if itr < max_itrs else "at max_itrs",
                       _ckpt_name(back)), st["records"])
    try:
        while True:
            if not (itr < max_itrs and rr > conv_threshold):
                if not check_every or st["checked"]:
                    break
                check()  # the final state (a failure restarts the loop from the checkpoint)
                continue
            ctx.spmv(A, p, w)
            pw = ctx.dot(p, w)
            if precond is None:
                alpha = fdiv(rr, pw)
                rr_new = ctx.calc_xr(x, r, p, w, alpha)
                beta = fdiv(rr_new, rr)
                ctx.calc_p(p, r, beta)
            else:
                alpha = fdiv(rz, pw)
                rz_new, rr_new = ctx.calc_xr_precond(x, r, p, w, precond, alpha)
                ctx.calc_p_precond(p, r, precond, fdiv(rz_new, rz))
                rz = rz_new
            rr = rr_new
            note_threshold(rr, conv_threshold, noted)
            if on_iteration is not None:
                on_iteration(itr, rr)
            itr += 1
            watch.ran(itr)
            if check_every:
                st["checked"] = False
                if itr % check_every == 0:
                    check()
        watch.final()
    finally:
        if check_every and own_ckpt:
            ctx.destroy_vector(x_ckpt)
    return itr, rr


cg_solve = _with_matrix_check(cg_solve, _cg_solve)


# iterations per look at the scalars in cg_solve_device.  Not measured: the smallest stride within 2 % of the best
# time on the 1 M-row matrix is to replace it (tools/device_loop_bench.py).  The block form
# (cg_solve_block_device) has been swept over 4, 16 and 64: 16 is that stride on the 1 M-row matrix.
DEFAULT_STRIDE = 16


def _whole_stride(stride):
    if int(stride) != stride or stride < 1:
        raise ValueError("stride must be a whole number >= 1, not %r" % (stride,))
    return int(stride)


def _device_batches(ctx, max_itrs, stride, graph, rec, tail, seed, enqueue, record, before_capture=None,
                    slots=False, on_batch=None, watch=_NO_WATCH):
    """The batch loop of cg_solve_device and cg_solve_block_device: a trail of stride + 1 records of `rec` doubles
    with `tail` doubles behind them (at pw_at = rec * (stride + 1): the SpMV's product), record `stride` starting
    with `seed`.  A batch copies record `stride` to record 0 and calls enqueue(trail, i, pw_at) for its iterations
    i = 0 .. m - 1; a full batch is captured once (behind before_capture()) and replayed when `graph`, else, and a
    short last one, enqueued call by call.  Then the trail is downloaded -- the one synchronisation, which drains
    the events -- and record(t, i, done) is called for i in order: true when iteration `done` was live (its
    bookkeeping done), false at the first frozen one, which ends the loop.  -> the count of live iterations.
    slots: a protected trail -- every word a SECDED slot of two doubles, so all offsets double
    (pw_at included), the seed record is encoded, and what is downloaded is decoded on the host (ctx.report_trail)
    before record() sees it, in the unprotected layout.  on_batch(done, trail): called after a batch's callbacks with
    the trail vector, whose record `stride` starts the next batch.
    watch: the _MatrixWatch of matrix_check_every=M.  A batch whose end count reaches or passes
    the next multiple of M -- known before it is enqueued, from `done` and m -- has ctx.verify_matrix_dev enqueued
    behind its last iteration; the two shapes of a full batch, with and without it, are captured once each.  The
    verdict arrives with the batch's download, which drains the events: FatalEvent there, before the batch's
    callbacks.  When the last batch had none, one verification is enqueued and waited for behind the loop.  A flip is
    therefore seen at most M + stride - 1 iterations after it happened."""
    # (the records' lengths and word indices, here and in the callers, are those csrc/guard_protocol.h defines)
    wide = 2 if slots else 1  # doubles per trail word
    pw_at = wide * rec * (stride + 1)
    trail = ctx.create_vector(pw_at + wide * tail)
    first, last = ctx.view_vector(trail, 0, wide * rec), ctx.view_vector(trail, wide * rec * stride, wide * rec)
    start = np.zeros(pw_at + wide * tail)
    if slots:  # every slot a codeword of its ordinal from the start: +0.0 everywhere, the seed in record `stride`
        whole = np.zeros(rec)
        start[:pw_at] = np.tile(ctx.encode_trail(whole, 0), stride + 1)
        start[pw_at:] = ctx.encode_trail(np.zeros(tail), 0)
        whole[:len(seed)] = seed
        start[wide * rec * stride:wide * rec * (stride + 1)] = ctx.encode_trail(whole, 0)
    else:
        start[rec * stride:rec * stride + len(seed)] = seed  # where the first batch's copy finds it
    ctx.upload(trail, start)

    def batch(m, verify):
        ctx.copy_vector(first, last)
        for i in range(m):
            enqueue(trail, i, pw_at)
        if verify:
            ctx._enqueue_verify(watch.A)  # counted by watch.enqueued(), per batch: captured or not

    done, graphs = 0, {}
    try:
        while True:
            m = min(stride, max_itrs - done)
            verify = watch.due(done, m)
            if graph and m == stride:
                if verify not in graphs:
                    if before_capture is not None and not graphs:
                        before_capture()
                    ctx.graph_begin()
                    try:
                        batch(m, verify)
                    finally:
                        graphs[verify] = ctx.graph_end()
                ctx.graph_launch(graphs[verify])
            else:
                batch(m, verify)
            if verify:
                watch.enqueued()
            t = ctx.download(trail)  # synchronises, then drains the events
            if slots:
                t = ctx.report_trail(t, rec, stride)
            stopped = False
            for i in range(m):
                if not record(t, i, done):
                    stopped = True
                    break
                done += 1
            if on_batch is not None:
                on_batch(done, trail)
            if stopped or done >= max_itrs:
                break
        watch.final_dev()
    finally:
        for g in graphs.values():
            ctx.graph_destroy(g)
        for v in (first, last, trail):
            ctx.destroy_vector(v)
    return done


def _check_batch(done, max_itrs, stride, check_every):
    """The batch schedule of cg_solve_device(check_every > 0): -> (m, check), the length of the batch that starts
    at iteration count done < max_itrs and whether a residual check is enqueued behind its last iteration.  A batch
    never crosses a check position (the counts that are multiples of check_every), so the check follows exactly the
    iterations i with (i + 1) % check_every == 0.  From a multiple of check_every on -- the start, and the count
    after every periodic check, rollbacks included -- two shapes recur: (stride, False), and
    ((check_every - 1) % stride + 1, True)."""
    next_check = (done // check_every + 1) * check_every
    m = min(stride, max_itrs - done, next_check - done)
    return m, done + m == next_check


def _device_batches_checked(ctx, A, b, x, r, w, x_ckpt, max_itrs, stride, graph, rec, seed, enqueue, record, goes_on,
                            restart, check_every, check_tol, max_rollbacks, bb, on_check, on_batch=None):
    """_device_batches with residual checks.  The trail has four more doubles behind the p.w
    pair (at chk_at = pw_at + 2) for ctx.residual_check_dev.  A batch of m iterations uses records stride - m ..
    stride, so that record `stride` holds the latest scalars after every batch, whatever its length: it copies
    record `stride` to record stride - m, calls enqueue(trail, i, pw_at) for i = stride - m .. stride - 1 and, when
    _check_batch says so, enqueues the check behind them.  The two recurring shapes are captured once each (behind
    ctx.residual_check_reserve) and replayed when `graph`; every other batch is enqueued call by call.  The download
    of the trail stays the one synchronisation; record(t, i, done) as in _device_batches, then the check's slot.
    goes_on(): cg_solve's `rr > conv_threshold` on the last live r.r.  restart() -> the seed of a recurrence
    restarted from the restored x.  -> the count of live iterations."""
    pw_at = rec * (stride + 1)
    chk_at = pw_at + 2
    trail = ctx.create_vector(chk_at + 4)
    last, chk = ctx.view_vector(trail, rec * stride, rec), ctx.view_vector(trail, chk_at, 4)
    firsts, graphs = {}, {}
    start = np.zeros(chk_at + 4)
    start[rec * stride:rec * stride + len(seed)] = seed
    ctx.upload(trail, start)
    limit = check_tol * check_tol * bb  # as _check_passes forms it
    recurring = ((stride, False), ((check_every - 1) % stride + 1, True))
    st = dict(checked=False, ckpt=-1, fails=0, records=[])
    done = 0

    def batch(m, check):
        ctx.copy_vector(firsts[m], last)
        for i in range(stride - m, stride):
            enqueue(trail, i, pw_at)
        if check:
            ctx.residual_check_dev(A, b, x, r, w, x_ckpt, trail, chk_at, limit)

    def verdict(c):
        """the slot of a check that followed iteration done - 1: the device has copied x to the checkpoint (passed)
        or the checkpoint back into x (anything else)"""
        gap2, ok = float(c[0]), c[2] == 1.0
        gap = math.sqrt(gap2) if gap2 >= 0 else gap2
        back = None
        if ok:
            st["ckpt"] = done - 1
        else:
            st["fails"] += 1
            back = st["ckpt"]
            again = np.zeros(rec)
            new = restart()
            again[:len(new)] = new
            ctx.upload(last, again)
        st["checked"] = True
        st["records"].append((done - 1, gap, ok, back))
        if on_check is not None:
            on_check(done - 1, gap, ok, back)
        if not ok and (st["fails"] > max_rollbacks or done >= max_itrs):
            raise ResidualCheckFailed(
                "residual check failed at iteration %d (gap %.3e > %.3e) %s; x holds the checkpoint of %s"
                % (done - 1, gap, check_tol * math.sqrt(bb),
                   "after %d rollbacks" % (st["fails"] - 1) if done < max_itrs else "at max_itrs",
                   _ckpt_name(back)), st["records"])

    try:
        while True:
            if not (done < max_itrs and goes_on()):
                if st["checked"]:
                    break
                # the final state, which no check has seen: the one extra synchronisation of a solve
                ctx.residual_check_dev(A, b, x, r, w, x_ckpt, trail, chk_at, limit)
                verdict(ctx.download(chk))
                continue
            m, check = _check_batch(done, max_itrs, stride, check_every)
            if m not in firsts:
                firsts[m] = ctx.view_vector(trail, rec * (stride - m), rec)
            if graph and (m, check) in recurring:
                if (m, check) not in graphs:
                    ctx.residual_check_reserve()
                    ctx.graph_begin()
                    try:
                        batch(m, check)
                    finally:
                        graphs[(m, check)] = ctx.graph_end()
                ctx.graph_launch(graphs[(m, check)])
            else:
                batch(m, check)
            t = ctx.download(trail)  # synchronises, then drains the events
            for i in range(stride - m, stride):
                if not record(t, i, done):
                    break  # frozen: a check behind this batch has seen the final state
                done += 1
                st["checked"] = False
            if check:
                verdict(t[chk_at:chk_at + 4])
            if on_batch is not None:  # behind the batch's callbacks, on_check included
                on_batch(done, trail)
    finally:
        for g in graphs.values():
            ctx.graph_destroy(g)
        for v in list(firsts.values()) + [last, chk, trail]:
            ctx.destroy_vector(v)
    return done


def cg_solve_device(ctx, A, b, x, r, p, w, max_itrs=1000, conv_threshold=1e-3, on_iteration=None,
                    stride=DEFAULT_STRIDE, graph=True, precond=None, vector_ecc=False, check_every=0,
                    check_tol=1e-7, max_rollbacks=3, x_ckpt=None, on_check=None):
    """The parameters cg_solve_device takes by position or by name, in the order they have always had (the residual
    checks' five stay the last of them: tests/test_device_loop_check_host.py pins that).  The public cg_solve_device
    below wraps this function and adds two KEYWORD-ONLY arguments behind them, trail_ecc=False and on_batch=None;
    inspect.signature follows the wrapper to this list, so look there for those two."""
    return _cg_solve_device(ctx, A, b, x, r, p, w, max_itrs, conv_threshold, on_iteration, stride, graph, precond,
                            vector_ecc, check_every, check_tol, max_rollbacks, x_ckpt, on_check, False, None, 0)


_cg_solve_device_positional = cg_solve_device


@functools.wraps(_cg_solve_device_positional, assigned=("__module__", "__name__", "__qualname__"))
def cg_solve_device(*args, trail_ecc=False, on_batch=None, **kw):
    # (matrix_check_every=0, keyword-only like the two above, is taken out of **kw: the wrapper's own keyword defaults
    # stay the pair tests/test_trail_ecc_host.py pins)
    matrix_check_every = kw.pop("matrix_check_every", 0)
    if not trail_ecc and on_batch is None and not matrix_check_every:
        return _cg_solve_device_positional(*args, **kw)
    bound = inspect.signature(_cg_solve_device_positional).bind(*args, **kw)
    bound.apply_defaults()
    return _cg_solve_device(*bound.args, trail_ecc, on_batch, matrix_check_every)


def _cg_solve_device(ctx, A, b, x, r, p, w, max_itrs, conv_threshold, on_iteration, stride, graph, precond, vector_ecc,
                     check_every, check_tol, max_rollbacks, x_ckpt, on_check, trail_ecc, on_batch, matrix_check_every):
    """cg_solve_device(ctx, A, b, x, r, p, w, max_itrs=1000, conv_threshold=1e-3, on_iteration=None,
    stride=DEFAULT_STRIDE, graph=True, precond=None, vector_ecc=False, check_every=0, check_tol=1e-7, max_rollbacks=3,
    x_ckpt=None, on_check=None, *, trail_ecc=False, on_batch=None, matrix_check_every=0)

    cg_solve's loop (cg.cpp:87-118) with alpha, beta and the stop test on the device:
    the host looks at the scalars once per batch of `stride` iterations instead of twice per iteration.

    copy r <- b, copy p <- r and rr0 = dot(r, r) as cg_solve; with max_itrs == 0 or not rr0 > conv_threshold
    that is all: (0, rr0).  Otherwise batches of m = min(stride, max_itrs - done) guarded iterations
    (ctx.cg_iteration_until_dev) over a trail of stride + 1 pairs {r.r, events}: iteration k of a batch reads
    pair k and writes pair k + 1, and is frozen -- x, r, p untouched, the pair handed on -- once its pair is not
    above conv_threshold.  Every batch starts by copying pair `stride` to pair 0.  A full batch is one graph,
    captured once and replayed (graph=True); a short last batch, and everything with graph=False, is enqueued
    call by call.  After a batch the trail is downloaded -- the one synchronisation --, events are drained
    (FatalEvent is raised there, before any callback of the batch), and the pairs are read in order: iteration
    `done` was live with result pair k + 1 while pair k is above the threshold.

    on_iteration(itr, rr) is called for every live iteration in order, but AFTER its batch: the vectors it sees
    are the batch's end state, not that iteration's.  -> (itr, rr) as cg_solve: the count of live iterations and
    the last live r.r (a frozen tail costs at most stride - 1 SpMVs per solve, plus one batch when the loop
    stops on a batch's last iteration before max_itrs).

    precond: a vector dinv (ctx.jacobi(A)) makes it cg_solve(precond=dinv)'s loop: r <- b and
    rz, rr0 = precond_start(r, dinv, p) as there, then batches of ctx.pcg_iteration_until_dev over a trail of
    stride + 1 records of four doubles {r.r, events, r.z, 0.0} -- record k at 4 k, the pair p.w behind them at
    4 (stride + 1), record `stride` seeded with {rr0, 0, rz, 0}.  Batches, the graph, the download, events, callbacks
    and the return value are as above; the stop test stays on r.r.  With precond=None the calls and the trail are
    exactly those made without the argument.

    vector_ecc=True makes it cg_solve(vector_ecc=True)'s loop on protected vectors: the start
    is that loop's -- b and x encoded in place, r <- b scrubbed at once, p <- r, rr0 = dot_vecc(r, r) --, then batches
    of ctx.cg_vecc_iteration_until_dev over the same trail of pairs as the plain loop, and x and b are scrubbed before
    returning (x and b hold codewords then: vecc_strip what is downloaded).  The pairs are plain doubles in device
    memory, outside any code.  Refused (ValueError, before anything runs) for a matrix ctx.vecc_supported refuses.
    With vector_ecc=False the calls are exactly those made without the argument.

    vector_ecc=True with precond=ctx.jacobi(A, protected=True) makes it cg_solve's loop of the same arguments
    (DESIGN.md section 5l): that start -- rz, rr0 = precond_start_vecc(r, dinv, p) behind the scrub of r --, then
    batches of ctx.pcg_vecc_iteration_until_dev over the preconditioned trail of four-double records, and x, b and
    dinv are scrubbed before returning.  A precond not marked protected is refused with vector_ecc, a protected one
    without it (ValueError, before anything runs).

    check_every > 0 adds cg_solve's residual checks with rollback (check_tol, max_rollbacks,
    x_ckpt, on_check and ResidualCheckFailed as there), the download after a batch still the only synchronisation.
    No batch crosses a check position (_check_batch): a batch that ends on one has ctx.residual_check_dev enqueued
    behind its last iteration -- w the scratch vector --, which forms the verdict on the device with the host's pass
    rule (limit = check_tol^2 * rr0) and acts on it there: x_ckpt <- x when the check passed, x <- x_ckpt when not.
    The trail has four more doubles behind the p.w pair for {gap^2, tt^2, verdict, events}; a batch of m iterations
    uses records stride - m .. stride.  With graph=True the two recurring batches -- `stride` iterations, and
    (check_every - 1) % stride + 1 iterations plus the check -- are captured once each; anything else is enqueued call
    by call.  After the download on_iteration runs for the live iterations, then on_check(itr, gap, ok,
    rolled_back_to) when the batch carried a check; a check behind a batch in which the loop froze has seen the final
    state.  After a failed check the host restarts the recurrence (ctx.residual_restart, with precond
    ctx.precond_start), reseeds record `stride` and goes on, the iteration count running on as in cg_solve.  When the
    loop is about to stop on a state no check has seen, one check is enqueued on its own and its slot downloaded: the
    one extra synchronisation of a solve.  precond (a plain dinv) is supported; vector_ecc=True with check_every > 0
    is refused as in cg_solve.  With check_every=0 the calls are exactly those made without the arguments.

    trail_ecc=True (keyword-only, as on_batch is) keeps the scalar trail under a SECDED code:
    every word of every record and
    of the p.w pair is a slot of two doubles, the seed is encoded (ctx.encode_trail), the batches are made of
    ctx.cg_trail_iteration_until_dev / pcg_trail_ / cg_vecc_trail_ / pcg_vecc_trail_ -- the same loops, the same bits
    --, and after every download the trail is decoded on the host (ctx.report_trail): a slot found with one flipped bit
    there is reported once, with the device's line, two flips raise FatalEvent.  On the device one flipped bit in a
    slot a launch reads is repaired, stored back and reported; two flips in a slot a decision depends on are fatal,
    and x, r and p keep every bit from that iteration on (FatalEvent at that batch's download, before its callbacks).
    Works with precond, vector_ecc, a structure-protected matrix, graph on or off, every stride.  Refused (ValueError,
    before anything runs) with check_every > 0: the check's four words are not under the code.
    on_batch(done, trail) runs after a batch's callbacks with the trail vector; its record `stride` starts the next
    batch (with trail_ecc: ctx.flip_trail(trail, slot, bits) flips a bit of it); with check_every > 0 it runs behind
    on_check as well, and the latest record is still record `stride`.  With trail_ecc=False and
    on_batch=None the calls are exactly those made without the arguments.

    matrix_check_every=M > 0 (keyword-only) verifies the matrix's digests as the loop runs (what
    it is for: cg_solve).  The matrix is armed if it is not.  A batch whose end count reaches or passes the next
    multiple of M has ctx.verify_matrix_dev enqueued behind its last iteration; with graph=True the two shapes of a
    full batch, with and without the verification, are captured once each.  The verdict arrives with the batch's
    download: a mismatch raises FatalEvent there, before the batch's callbacks, with the line "[ABFT] matrix digest
    mismatch in segment NAME"; nothing is restored.  One final verification is enqueued and waited for when the last
    batch had none.  A flip is seen at most M + stride - 1 iterations after it happened.  Works with precond,
    vector_ecc, trail_ecc and structure_ecc matrices.  Refused (ValueError, before anything runs) with
    check_every > 0.  With matrix_check_every=0 the calls are exactly those made without the keyword."""
    stride = _whole_stride(stride)
    _check_args(check_every, check_tol, max_rollbacks)
    if matrix_check_every and check_every:
        raise ValueError("cg_solve_device with check_every > 0 and matrix_check_every > 0: the device loop does not "
                         "verify the matrix in front of its residual checks yet; use cg_solve, or one of the two")
    if int(matrix_check_every) != matrix_check_every or matrix_check_every < 0:
        raise ValueError("matrix_check_every must be a whole number >= 0, not %r" % (matrix_check_every,))
    if trail_ecc and check_every:
        raise ValueError("trail_ecc with check_every > 0: the residual check's four words are not under the code")
    if vector_ecc and check_every:
        raise ValueError("vector_ecc with check_every > 0: the residual kernels write unencoded vectors")
    protected = _check_protected_precond(precond, vector_ecc)
    if vector_ecc:
        if not ctx.vecc_supported(A):
            raise ValueError("vector_ecc needs a CSR matrix in the streaming layout (this one: %s)"
                             % ("COO" if A.fmt != FMT_CSR else ctx.matrix_info(A)[0]))
        ctx.encode_vector(b)
        ctx.encode_vector(x)
    ctx.copy_vector(r, b)
    if vector_ecc:
        ctx.scrub_vector(r)  # the one read of b: repaired in r, b itself stays as it is until the end
        if protected:
            rz, rr = ctx.precond_start_vecc(r, precond, p)
            rec, seed = 4, [rr, 0.0, rz]
        else:
            ctx.copy_vector(p, r)
            rr = ctx.dot_vecc(r, r)
            rec, seed = 2, [rr]
    elif precond is None:
        ctx.copy_vector(p, r)
        rr = ctx.dot(r, r)
        rec, seed = 2, [rr]  # doubles per record of the trail: the pair {r.r, events}
    else:
        rz, rr = ctx.precond_start(r, precond, p)
        rec, seed = 4, [rr, 0.0, rz]  # {r.r, events, r.z, 0.0}
    noted = {}
    note_threshold(rr, conv_threshold, noted)
    done, last_rr = 0, [rr]
    watch = _watch(ctx, A, matrix_check_every)

    def enqueue(trail, k, pw_at):
        if trail_ecc:  # the same four loops on slots of two doubles
            if protected:
                ctx.pcg_vecc_trail_iteration_until_dev(A, p, x, r, p, w, precond, trail, 8 * k, pw_at, 8 * k + 8,
                                                       conv_threshold)
            elif vector_ecc:
                ctx.cg_vecc_trail_iteration_until_dev(A, p, x, r, p, w, trail, 4 * k, pw_at, 4 * k + 4, conv_threshold)
            elif precond is None:
                ctx.cg_trail_iteration_until_dev(A, p, x, r, p, w, trail, 4 * k, pw_at, 4 * k + 4, conv_threshold)
            else:
                ctx.pcg_trail_iteration_until_dev(A, p, x, r, p, w, precond, trail, 8 * k, pw_at, 8 * k + 8,
                                                  conv_threshold)
        elif protected:
            ctx.pcg_vecc_iteration_until_dev(A, p, x, r, p, w, precond, trail, 4 * k, pw_at, 4 * k + 4,
                                             conv_threshold)
        elif vector_ecc:
            ctx.cg_vecc_iteration_until_dev(A, p, x, r, p, w, trail, 2 * k, pw_at, 2 * k + 2, conv_threshold)
        elif precond is None:
            ctx.cg_iteration_until_dev(A, p, x, r, p, w, trail, 2 * k, pw_at, 2 * k + 2, conv_threshold)
        else:
            ctx.pcg_iteration_until_dev(A, p, x, r, p, w, precond, trail, 4 * k, pw_at, 4 * k + 4, conv_threshold)

    def record(t, k, done):
        if not (t[rec * k] > conv_threshold):
            return False
        last_rr[0] = float(t[rec * k + rec])
        note_threshold(last_rr[0], conv_threshold, noted)
        if on_iteration is not None:
            on_iteration(done, last_rr[0])
        return True

    if check_every:
        def restart():
            last_rr[0] = ctx.residual_restart(A, b, x, r, p, w)
            new = [last_rr[0]]
            if precond is not None:
                rz, last_rr[0] = ctx.precond_start(r, precond, p)  # p = z of the restarted r
                new = [last_rr[0], 0.0, rz]
            note_threshold(last_rr[0], conv_threshold, noted)
            return new

        own_ckpt = x_ckpt is None
        if own_ckpt:
            x_ckpt = ctx.create_vector(x.N)
        try:
            ctx.copy_vector(x_ckpt, x)
            done = _device_batches_checked(ctx, A, b, x, r, w, x_ckpt, max_itrs, stride, graph, rec, seed, enqueue,
                                           record, lambda: last_rr[0] > conv_threshold, restart, int(check_every),
                                           check_tol, max_rollbacks, rr, on_check,  # bb = rr: r = b, ||b||^2
                                           **({} if on_batch is None else {"on_batch": on_batch}))
        finally:
            if own_ckpt:
                ctx.destroy_vector(x_ckpt)
        return done, last_rr[0]
    if max_itrs != 0 and rr > conv_threshold:
        done = _device_batches(ctx, max_itrs, stride, graph, rec, 2, seed, enqueue, record, slots=bool(trail_ecc),
                               on_batch=on_batch, **({"watch": watch} if watch.every else {}))
    watch.final_dev()
    if vector_ecc:
        ctx.scrub_vector(x)
        ctx.scrub_vector(b)
        if protected:
            ctx.scrub_vector(precond)
    return done, last_rr[0]


cg_solve_device.__doc__ = _cg_solve_device.__doc__


def cg_solve_block_device(ctx, A, B, X, R, P, W, max_itrs=1000, conv_threshold=1e-3, on_iteration=None,
                          stride=DEFAULT_STRIDE, graph=True, precond=None, vector_ecc=False):
    """The parameters cg_solve_block_device takes by position or by name, in the order they have always had
    (tests/test_device_loop_block_vecc_host.py pins the last two).  The public cg_solve_block_device below wraps this
    function and adds two KEYWORD-ONLY arguments behind them, trail_ecc=False and on_batch=None, the way
    cg_solve_device does; inspect.signature follows the wrapper to this list."""
    return _cg_solve_block_device(ctx, A, B, X, R, P, W, max_itrs, conv_threshold, on_iteration, stride, graph, precond,
                                  vector_ecc, False, None, 0)


_cg_solve_block_device_positional = cg_solve_block_device


@functools.wraps(_cg_solve_block_device_positional, assigned=("__module__", "__name__", "__qualname__"))
def cg_solve_block_device(*args, trail_ecc=False, on_batch=None, **kw):
    matrix_check_every = kw.pop("matrix_check_every", 0)  # keyword-only, as in cg_solve_device
    if not trail_ecc and on_batch is None and not matrix_check_every:
        return _cg_solve_block_device_positional(*args, **kw)
    bound = inspect.signature(_cg_solve_block_device_positional).bind(*args, **kw)
    bound.apply_defaults()
    return _cg_solve_block_device(*bound.args, trail_ecc, on_batch, matrix_check_every)


def _cg_solve_block_device(ctx, A, B, X, R, P, W, max_itrs, conv_threshold, on_iteration, stride, graph, precond,
                           vector_ecc, trail_ecc, on_batch, matrix_check_every):
    """cg_solve_block_device(ctx, A, B, X, R, P, W, max_itrs=1000, conv_threshold=1e-3, on_iteration=None,
    stride=DEFAULT_STRIDE, graph=True, precond=None, vector_ecc=False, *, trail_ecc=False, on_batch=None,
    matrix_check_every=0)

    cg_solve_block(fused=True)'s loop with the K alphas, the K betas and the column mask on the device (DESIGN.md
    section 5h): the host looks at the scalars once per batch of `stride` iterations instead of twice per iteration.

    The start is cg_solve_block's: copy R <- B, then copy P <- R and dot_block, or with precond (ctx.jacobi(A))
    precond_start_block.  With max_itrs == 0 or no column above conv_threshold that is all.  Otherwise batches of
    m = min(stride, max_itrs - done) guarded iterations (ctx.cg_block_iteration_until_dev) over a trail of stride + 1
    records of 2K + 2 doubles {r.r[K], r.z[K] (plain: r.r again), events, 0.0} -- record i at (2K + 2) i, the K + 1
    doubles {P.W[K], events} behind them, record `stride` seeded with the start's sums.  Iteration i of a batch reads
    record i and writes record i + 1; column j is live in it while record i's r.r[j] is above conv_threshold, frozen
    -- its X, R, P untouched, its words handed on -- from then on.  Every batch starts by copying record `stride` to
    record 0.  A full batch is one graph, captured once (behind ctx.block_loop_reserve) and replayed (graph=True); a
    short last batch, and everything with graph=False, is enqueued call by call.  After a batch the trail is
    downloaded -- the one synchronisation --, events are drained (FatalEvent is raised there, before any callback of
    the batch), and the records are read in order: `active` of iteration i is the set of columns whose record-i r.r is
    above the threshold, and the loop stops at the first i without one.

    on_iteration(itr, rr, active) as cg_solve_block calls it -- rr of all K columns from record i + 1 -- but AFTER the
    batch: the vectors it sees are the batch's end state.  -> (itrs[K], rr[K]) as cg_solve_block.

    vector_ecc=True makes it cg_solve_block(vector_ecc=True)'s loop on protected block vectors:
    the start is that loop's -- B and X encoded in place, R <- B scrubbed at once, P <- R, rr = dot_block_vecc(R, R)
    --, then batches of ctx.cg_block_vecc_iteration_until_dev over the same trail of records, which are plain doubles
    in device memory, outside any code; X and B are scrubbed before returning, on the early return as well (X and B
    hold codewords then: vecc_strip what is downloaded).  Batches, the graph, the download, events, callbacks and the
    return value are as above.  Refused (ValueError, before anything runs) with any precond and for a matrix
    ctx.vecc_supported refuses.  With vector_ecc=False the calls are exactly those made without the argument.

    trail_ecc=True (keyword-only, as on_batch is) keeps the scalar trail under a SECDED code:
    every word of the records and of the {P.W[K], events} tail is a slot of two doubles under its ordinal in the
    record, the seed is encoded (ctx.encode_trail), the batches are made of ctx.cg_block_trail_iteration_until_dev /
    ctx.cg_block_vecc_trail_iteration_until_dev -- the same loops, the same bits --, and after every download the
    trail is decoded on the host (ctx.report_trail): a slot found with one flipped bit is reported once, two flips
    raise FatalEvent, and the records are then read in the plain layout.  The device repairs one flipped bit in a
    slot it reads and reports it (event 14); two flips stop the batch's remaining launches and raise FatalEvent at
    the download (event 15).  It works with precond, with vector_ecc, with the graph on or off, at every stride;
    the refusals are those above.
    on_batch(done, trail) runs after a batch's callbacks with the trail vector; its record `stride` starts the next
    batch (with trail_ecc: ctx.flip_trail(trail, slot, bits) flips a bit of it).  With trail_ecc=False and
    on_batch=None the calls are exactly those made without the two arguments.
    matrix_check_every=M > 0 (keyword-only): as in cg_solve_device -- ctx.verify_matrix_dev behind the last iteration of
    every batch that reaches or passes a multiple of M, FatalEvent at that batch's download on a mismatch, one final
    verification when the last batch had none.  With 0 the calls are exactly those made without the keyword.
    No check_every, one GPU."""
    _refuse_structure_ecc(ctx, A, "cg_solve_block_device")
    stride = _whole_stride(stride)
    if int(matrix_check_every) != matrix_check_every or matrix_check_every < 0:
        raise ValueError("matrix_check_every must be a whole number >= 0, not %r" % (matrix_check_every,))
    if vector_ecc:
        if precond is not None:
            raise ValueError("vector_ecc with a precond: the protected block loop has no Jacobi form")
        if not ctx.vecc_supported(A):
            raise ValueError("vector_ecc needs a CSR matrix in the streaming layout (this one: %s)"
                             % ("COO" if A.fmt != FMT_CSR else ctx.matrix_info(A)[0]))
    _check_protected_precond(precond, False)  # (a protected dinv has no block loop to go to)
    k = B.K
    if not k:
        raise ValueError("cg_solve_block_device wants block vectors (create_block)")
    if vector_ecc:
        ctx.encode_vector(B)
        ctx.encode_vector(X)
    ctx.copy_vector(R, B)
    if vector_ecc:
        ctx.scrub_vector(R)  # the one read of B: repaired in R, B itself stays as it is until the end
        ctx.copy_vector(P, R)
        rr = np.array(ctx.dot_block_vecc(R, R, k), dtype=np.float64)
        rz = rr
    elif precond is None:
        ctx.copy_vector(P, R)
        rr = np.array(ctx.dot_block(R, R, k), dtype=np.float64)
        rz = rr
    else:
        rz, rr = ctx.precond_start_block(R, precond, P, k, (1 << k) - 1)
        rz, rr = np.array(rz, dtype=np.float64), np.array(rr, dtype=np.float64)
    itrs = [0] * k
    noted = {}
    for j in range(k):
        note_threshold(rr[j], conv_threshold, noted)
    watch = _watch(ctx, A, matrix_check_every)
    if max_itrs == 0 or not any(rr[j] > conv_threshold for j in range(k)):
        watch.final_dev()
        if vector_ecc:
            ctx.scrub_vector(X)
            ctx.scrub_vector(B)
        return itrs, rr
    rec = 2 * k + 2  # doubles per record of the trail
    last_rr = [rr]

    def enqueue(trail, i, pw_at):
        if trail_ecc:  # the same two loops on slots of two doubles
            if vector_ecc:
                ctx.cg_block_vecc_trail_iteration_until_dev(A, X, R, P, W, k, trail, 2 * rec * i, pw_at,
                                                            2 * rec * (i + 1), conv_threshold)
            else:
                ctx.cg_block_trail_iteration_until_dev(A, X, R, P, W, k, trail, 2 * rec * i, pw_at, 2 * rec * (i + 1),
                                                       conv_threshold, dinv=precond)
            return
        if vector_ecc:
            ctx.cg_block_vecc_iteration_until_dev(A, X, R, P, W, k, trail, rec * i, pw_at, rec * (i + 1),
                                                  conv_threshold)
            return
        ctx.cg_block_iteration_until_dev(A, X, R, P, W, k, trail, rec * i, pw_at, rec * (i + 1), conv_threshold,
                                         dinv=precond)

    def record(t, i, done):
        active = sum(1 << j for j in range(k) if t[rec * i + j] > conv_threshold)
        if not active:
            return False
        rr = last_rr[0] = np.array(t[rec * (i + 1):rec * (i + 1) + k], dtype=np.float64)
        for j in range(k):
            if (active >> j) & 1:
                itrs[j] += 1
                note_threshold(rr[j], conv_threshold, noted)
        if on_iteration is not None:
            on_iteration(done, rr.copy(), active)
        return True

    _device_batches(ctx, max_itrs, stride, graph, rec, k + 1, np.concatenate([rr, rz]), enqueue, record,
                    before_capture=lambda: ctx.block_loop_reserve(A, k), slots=bool(trail_ecc), on_batch=on_batch,
                    **({"watch": watch} if watch.every else {}))
    if vector_ecc:
        ctx.scrub_vector(X)
        ctx.scrub_vector(B)
    return itrs, last_rr[0]


cg_solve_block_device.__doc__ = _cg_solve_block_device.__doc__


def _cg_solve_vecc(ctx, A, b, x, r, p, w, max_itrs, conv_threshold, on_iteration, precond=None, watch=_NO_WATCH):
    """cg_solve(vector_ecc=True): the loop of cg_solve on protected vectors; precond: a protected dinv"""
    ctx.encode_vector(b)
    ctx.encode_vector(x)
    ctx.copy_vector(r, b)
    ctx.scrub_vector(r)  # the one read of b: repaired in r, b itself stays as it is until the end
    if precond is None:
        ctx.copy_vector(p, r)
        rr = ctx.dot_vecc(r, r)
    else:
        rz, rr = ctx.precond_start_vecc(r, precond, p)
    itr = 0
    noted = {}
    note_threshold(rr, conv_threshold, noted)
    while itr < max_itrs and rr > conv_threshold:
        ctx.spmv_vecc(A, p, w)
        pw = ctx.dot_vecc(p, w)
        if precond is None:
            rr_new = ctx.calc_xr_vecc(x, r, p, w, fdiv(rr, pw))
            ctx.calc_p_vecc(p, r, fdiv(rr_new, rr))
        else:
            alpha = fdiv(rz, pw)
            rz_new, rr_new = ctx.calc_r_precond_vecc(r, w, precond, alpha)
            ctx.calc_px_precond_vecc(x, p, r, precond, alpha, fdiv(rz_new, rz))
            rz = rz_new
        rr = rr_new
        note_threshold(rr, conv_threshold, noted)
        if on_iteration is not None:
            on_iteration(itr, rr)
        itr += 1
        watch.ran(itr)
    watch.final()
    ctx.scrub_vector(x)
    ctx.scrub_vector(b)
    if precond is not None:
        ctx.scrub_vector(precond)
    return itr, rr


def _cg_solve_block_vecc(ctx, A, B, X, R, P, W, k, max_itrs, conv_threshold, on_iteration, watch=_NO_WATCH):
    """cg_solve_block(vector_ecc=True): the fused block loop on protected block vectors"""
    ctx.encode_vector(B)
    ctx.encode_vector(X)
    ctx.copy_vector(R, B)
    ctx.scrub_vector(R)  # the one read of B: repaired in R, B itself stays as it is until the end
    ctx.copy_vector(P, R)
    rr = np.array(ctx.dot_block_vecc(R, R, k), dtype=np.float64)
    itrs = [0] * k
    noted = {}
    for j in range(k):
        note_threshold(rr[j], conv_threshold, noted)
    itr = 0
    while True:
        active = sum(1 << j for j in range(k) if itrs[j] < max_itrs and rr[j] > conv_threshold)
        if not active:
            break
        on = [(active >> j) & 1 for j in range(k)]
        pw = ctx.spmm_dot_vecc(A, P, W, k, drain=False)
        alpha = [fdiv(rr[j], pw[j]) if on[j] else 0.0 for j in range(k)]
        rr_new = ctx.calc_r_block_vecc(R, W, k, alpha, active)
        beta = [fdiv(rr_new[j], rr[j]) if on[j] else 0.0 for j in range(k)]
        ctx.calc_px_block_vecc(X, P, R, k, alpha, beta, active)
        for j in range(k):
            if on[j]:
                rr[j] = rr_new[j]
                itrs[j] += 1
                note_threshold(rr[j], conv_threshold, noted)
        if on_iteration is not None:
            on_iteration(itr, rr.copy(), active)
        itr += 1
        watch.ran(itr)
    watch.final()
    ctx.scrub_vector(X)
    ctx.scrub_vector(B)
    return itrs, rr


def cg_solve_block(ctx, A, B, X, R, P, W, max_itrs=1000, conv_threshold=1e-3, on_iteration=None, check_every=0,
                   check_tol=1e-7, max_rollbacks=3, x_ckpt=None, on_check=None, precond=None, fused=False,
                   vector_ecc=False):
    """cg_solve_block(ctx, A, B, X, R, P, W, max_itrs=1000, conv_threshold=1e-3, on_iteration=None, check_every=0,
    check_tol=1e-7, max_rollbacks=3, x_ckpt=None, on_check=None, precond=None, fused=False, vector_ecc=False, *,
    matrix_check_every=0)

    cg_solve for the K columns of block vectors (ctx.create_block) at once: per column j exactly
    cg_solve's control flow -- column j iterates while itrs[j] < max_itrs and rr[j] > conv_threshold --
    on one spmm / dot_block / calc_xr_block / calc_p_block per iteration.  A column that has stopped
    is frozen through the active mask (its x, r, p are not touched again); the loop ends when no
    column is active.  on_iteration(itr, rr, active): after every iteration, rr of all K columns and
    the mask of the columns that iteration updated.  -> (itrs[K], rr[K])

    Residual checks (check_every > 0) as in cg_solve, per column: the columns due for a check share one
    residual_gap_block; a failed column alone is restored (copy_block from x_ckpt, a block vector made
    here when None) and restarted (residual_restart_block with its bit in the mask); the other columns'
    x, r, p keep their bits.  on_check(itr, gap, ok, rolled_back_to, rhs), itr counting column rhs's
    iterations.

    precond: as in cg_solve, one N-entry dinv for all K columns (one operator), through the *_precond_block
    calls; after a rollback precond_start_block rewrites P in the rolled-back columns only.

    fused: the iteration in three calls -- spmm_dot (P . W out of the SpMM), calc_r_block (r and its sums),
    calc_px_block (x and p in one pass over p) -- instead of spmm / dot_block / calc_xr_block / calc_p_block:
    64 N K bytes of vectors behind the SpMM instead of 88 N K.  Control flow, masks and checks are the same;
    x, r and p get the same operations, and only P . W is summed in another order.

    vector_ecc=True runs the loop on protected block vectors, as cg_solve(vector_ecc=True) does
    for one column: B and X are encoded in place, R <- B is a copy of codewords that is scrubbed at once, P <- R,
    rr = dot_block_vecc(R, R); per iteration spmm_dot_vecc, calc_r_block_vecc and calc_px_block_vecc -- always the
    three-call iteration: `fused` is ignored, there is no four-call protected form --; X and B are scrubbed before
    returning.  Every word of every column is checked by every call, stopped columns included, and a stopped
    column's words are stored back repaired.  Control flow, masks, on_iteration and the return value are as
    without it.  Refused (ValueError, before anything runs) with check_every > 0, with any precond, and for a matrix
    ctx.vecc_supported refuses.  With vector_ecc=False the calls are exactly those made without the argument.

    matrix_check_every=M > 0 (keyword-only): as in cg_solve, the loop's iterations counted whatever columns they
    update -- a verification of the matrix's digests behind every M-th iteration, in front of every residual check
    and before returning; a mismatch raises FatalEvent.  With 0 the calls are exactly those made without it."""
    return _cg_solve_block(ctx, A, B, X, R, P, W, max_itrs, conv_threshold, on_iteration, check_every, check_tol,
                           max_rollbacks, x_ckpt, on_check, precond, fused, vector_ecc, _NO_WATCH)


def _cg_solve_block(ctx, A, B, X, R, P, W, max_itrs, conv_threshold, on_iteration, check_every, check_tol, max_rollbacks,
                    x_ckpt, on_check, precond, fused, vector_ecc, watch):
    """cg_solve_block's body; watch: _NO_WATCH, or the _MatrixWatch of matrix_check_every"""
    _refuse_structure_ecc(ctx, A, "cg_solve_block")
    _check_args(check_every, check_tol, max_rollbacks)
    if vector_ecc:
        if check_every:
            raise ValueError("vector_ecc with check_every > 0: the residual kernels write unencoded vectors")
        if precond is not None:
            raise ValueError("vector_ecc with a precond: the protected block loop has no Jacobi form")
        if not ctx.vecc_supported(A):
            raise ValueError("vector_ecc needs a CSR matrix in the streaming layout (this one: %s)"
                             % ("COO" if A.fmt != FMT_CSR else ctx.matrix_info(A)[0]))
    _check_protected_precond(precond, False)  # (a protected dinv has no block loop to go to)
    k = B.K
    if not k:
        raise ValueError("cg_solve_block wants block vectors (create_block)")
    if vector_ecc:
        return _cg_solve_block_vecc(ctx, A, B, X, R, P, W, k, max_itrs, conv_threshold, on_iteration, watch)
    ctx.copy_vector(R, B)
    rz = None
    if precond is None:
        ctx.copy_vector(P, R)
        rr = np.array(ctx.dot_block(R, R, k), dtype=np.float64)
    else:
        rz, rr = ctx.precond_start_block(R, precond, P, k, (1 << k) - 1)
        rz, rr = np.array(rz, dtype=np.float64), np.array(rr, dtype=np.float64)
    itrs = [0] * k
    noted = {}
    for j in range(k):
        note_threshold(rr[j], conv_threshold, noted)

    def still(j):
        return itrs[j] < max_itrs and rr[j] > conv_threshold

    if check_every:
        bb = rr.copy()  # R = B: ||b_j||^2
        own_ckpt = x_ckpt is None
        if own_ckpt:
            x_ckpt = ctx.create_block(B.N // k, k)
        ctx.copy_vector(x_ckpt, X)
        checked, ckpt, fails, records = [False] * k, [-1] * k, [0] * k, []

        def check(due):
            watch.before_check()
            gap2, tt2 = ctx.residual_gap_block(A, B, X, R, W, k, due)
            passed = failed = 0
            events = []
            for j in range(k):
                if not (due >> j) & 1:
                    continue
                ok = _check_passes(gap2[j], tt2[j], bb[j], check_tol)
                gap = math.sqrt(gap2[j]) if gap2[j] >= 0 else float(gap2[j])
                events.append((itrs[j] - 1, gap, ok, None if ok else ckpt[j], j))
                checked[j] = True
                if ok:
                    passed |= 1 << j
                    ckpt[j] = itrs[j] - 1
                else:
                    failed |= 1 << j
                    fails[j] += 1
            if passed:
                ctx.copy_block(x_ckpt, X, k, passed)
            if failed:
                ctx.copy_block(X, x_ckpt, k, failed)
                rr_new = ctx.residual_restart_block(A, B, X, R, P, W, k, failed)
                if precond is not None:
                    rz_new, rr_new = ctx.precond_start_block(R, precond, P, k, failed)
                    for j in range(k):
                        if (failed >> j) & 1:
                            rz[j] = rz_new[j]
                for j in range(k):
                    if (failed >> j) & 1:
                        rr[j] = rr_new[j]
                        note_threshold(rr[j], conv_threshold, noted)
            for e in events:
                records.append(e)
                if on_check is not None:
                    on_check(*e)
            for i, gap, ok, back, j in events:
                if not ok and (fails[j] > max_rollbacks or itrs[j] >= max_itrs):
                    raise ResidualCheckFailed(
                        "rhs %d: residual check failed at iteration %d (gap %.3e > %.3e) %s; x holds the "
                        "checkpoint of %s" % (j, i, gap, check_tol * math.sqrt(bb[j]),
                                              "after %d rollbacks" % (fails[j] - 1) if itrs[j] < max_itrs
                                              else "at max_itrs", _ckpt_name(back)), records)

    itr = 0
    try:
        while True:
            if check_every:
                # due: every column that has just finished a multiple of check_every iterations, and every
                # column about to stop on a state no check has seen
                due = sum(1 << j for j in range(k)
                          if not checked[j] and (not still(j) or (itrs[j] and itrs[j] % check_every == 0)))
                if due:
                    check(due)
            active = sum(1 << j for j in range(k) if still(j))
            if not active:
                break
            on = [(active >> j) & 1 for j in range(k)]
            num = rr if precond is None else rz
            extra = () if precond is None else (precond,)
            if fused:
                pw = ctx.spmm_dot(A, P, W, k, drain=False)
                alpha = [fdiv(num[j], pw[j]) if on[j] else 0.0 for j in range(k)]
                sums = ctx.calc_r_block(R, W, k, alpha, active, *extra)
                rz_new, rr_new = (None, sums) if precond is None else sums
                num_new = rr_new if precond is None else rz_new
                beta = [fdiv(num_new[j], num[j]) if on[j] else 0.0 for j in range(k)]
                ctx.calc_px_block(X, P, R, k, alpha, beta, active, *extra)
            elif precond is None:
                ctx.spmm(A, P, W, k, drain=False)
                pw = ctx.dot_block(P, W, k)
                alpha = [fdiv(rr[j], pw[j]) if on[j] else 0.0 for j in range(k)]
                rr_new = ctx.calc_xr_block(X, R, P, W, k, alpha, active)
                beta = [fdiv(rr_new[j], rr[j]) if on[j] else 0.0 for j in range(k)]
                ctx.calc_p_block(P, R, k, beta, active)
            else:
                ctx.spmm(A, P, W, k, drain=False)
                pw = ctx.dot_block(P, W, k)
                alpha = [fdiv(rz[j], pw[j]) if on[j] else 0.0 for j in range(k)]
                rz_new, rr_new = ctx.calc_xr_precond_block(X, R, P, W, precond, k, alpha, active)
                beta = [fdiv(rz_new[j], rz[j]) if on[j] else 0.0 for j in range(k)]
                ctx.calc_p_precond_block(P, R, precond, k, beta, active)
            for j in range(k):
                if on[j]:
                    if precond is not None:
                        rz[j] = rz_new[j]
                    rr[j] = rr_new[j]
                    itrs[j] += 1
                    note_threshold(rr[j], conv_threshold, noted)
                    if check_every:
                        checked[j] = False
            if on_iteration is not None:
                on_iteration(itr, rr.copy(), active)
            itr += 1
            watch.ran(itr)
        watch.final()
    finally:
        if check_every and own_ckpt:
            ctx.destroy_vector(x_ckpt)
    return itrs, rr


cg_solve_block = _with_matrix_check(cg_solve_block, _cg_solve_block)
