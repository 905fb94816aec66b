"""cg.py -- the reference driver's command line (cg.cpp:38-309) for the hip target on one
GPU, through the ctypes mirror of the plugin interface (context.HIPContext):

    python -m abft_sparse_cg_amd.cg -t hip -s laplace5:3162,3162 -m secded -i 200 -c 0

Same flags, defaults and stdout as cg-csr / cg-coo; additions: --format csr|coo (the
reference picks the format by executable), -s/--synthetic, --seed, --flip-at
INDEX:BIT[,BIT...], -q/--quiet.  It drives HIPContext call for call like the C++ driver.
Several GPUs: the C++ executables (host/cg-csr, host/cg-coo under host/mgpu-run or
torch.distributed.run --no-python) are the one multi-process implementation.
"""
import ctypes
import math
import os
import sys
import time

import numpy as np

DEFAULT_MTX = "matrices/shallow_water1/shallow_water1.mtx"

USAGE = """
Usage: %s [OPTIONS]

Options:
  -h  --help                  Print this message
  -b  --num-blocks      B     Number of times to block input matrix
  -c  --convergence     C     Convergence threshold
  -f  --matrix-file     M     Path to matrix-market format file
  -i  --iterations      I     Maximum number of iterations
  -l  --list                  List available implementations
  -m  --mode            MODE  ABFT mode
  -t  --target          TARG  Implementation target
  -x  --inject-bitflip        Inject a random bit-flip into A

  The -l|--list argument will provide a list of tuples that describe
  which implementations are available to be passed to the
  -t|--target and -m|--mode arguments.

  The -x|--inject-bitflip argument optionally takes a number to
  control how many bits to flip, and either INDEX or VALUE to
  restrict the region of bits in the matrix element to target.

Additional options of this build:
      --format          F     csr (default) or coo
  -s  --synthetic       SPEC  Generate the matrix in memory instead of -f:
                              laplace5:NX,NY | random:N,K,SEED | powerlaw:N,SEED
      --seed            N     Seed for the -x draws (default: time)
      --flip-at  I:B[,B...]   Flip the given bit(s) of matrix element I (may be repeated)
  -q  --quiet                 Do not print the per-iteration residual
      --rhs             K     Solve K right-hand sides (1-8) at once, one pass over the
                              matrix per iteration (CSR only); column j of b is the
                              reference's b drawn with seed 1+j
      --check-every     N     Check r against b - Ax every N iterations and before
                              stopping; roll back to the last good x on a failure
                              (0 = off, the default)
      --check-tol       T     A check fails when ||b - Ax - r|| > T ||b|| (default 1e-7)
      --max-rollbacks   M     Give up (exit 1) after more than M failed checks (default 3)
      --flip-vector I:V:J:B[,B...]
                              After iteration I, flip bit(s) B (0-63) of entry J of
                              vector V (x, r or p; with --rhs K, J = row * K + column;
                              with --vector-ecc secded also w or b) (may be repeated)
      --precond         P     Preconditioner: none (default) or jacobi (the inverse
                              diagonal of A, applied inside the vector kernels)
      --block-fused           With --rhs K: the fused block iteration (P.W formed inside
                              the SpMM, x and p updated in one pass)
      --vector-ecc      E     Protect the CG vectors: none (default) or secded, a (64, 57)
                              code in each double's low 7 mantissa bits (CSR, one
                              right-hand side, no --precond / --check-every)
      --device-loop     S     Keep alpha, beta and the stop test on the device and look
                              at the residuals every S iterations (S >= 1) instead of
                              twice per iteration: same iterations, residuals and x; the
                              lines of a batch are printed after it.  Not with --rhs,
                              --precond, --check-every, --vector-ecc or --flip-vector
      --structure-ecc   E     Protect the CSR row structure: none (default) or secded --
                              row extents under a (64, 57) code, row-block descriptors
                              under a (128, 120) code (CSR, one right-hand side)
      --flip-structure I:K:J:B[,B...]
                              After iteration I, flip bit(s) B of stored structure word
                              J of kind K: row (a row extent, bits 0-63) or block (a
                              row-block descriptor, bits 0-127); needs --structure-ecc
                              secded (may be repeated)
      --trail-ecc       E     Protect the device loop's scalar trail: none (default) or
                              secded -- every word a slot under the (128, 120) code;
                              needs --device-loop S
      --flip-trail I:W:B[,B...]
                              Flip bit(s) B (0-127) of word W (0 r.r, 1 events) of the
                              record handed to the batch after iteration I's; needs
                              --trail-ecc secded (may be repeated)
      --verify-matrix   M     Verify the digests of every stored array of the matrix
                              every M iterations (M >= 1) and before stopping; a
                              mismatch prints its line and exits 1
      --flip-matrix I:S:W:B[,B...]
                              After iteration I (with --device-loop: after I's batch),
                              flip bit(s) B of the stored array S (cols, vals, pal,
                              wbase, ...: a segment the matrix has), counted from bit 0
                              of its 32-bit word W (bit 40 is bit 8 of word W + 1) (may
                              be repeated)

"""


FLIP_VECTOR_MSG = "Invalid --flip-vector (want ITER:VEC:INDEX:BIT[,BIT...], VEC one of x, r, p)"
FLIP_STRUCTURE_MSG = "Invalid --flip-structure (want ITER:row|block:INDEX:BIT[,BIT...])"
FLIP_MATRIX_MSG = "Invalid --flip-matrix (want ITER:SEGMENT:WORD:BIT[,BIT...])"
FLIP_TRAIL_MSG = "Invalid --flip-trail (want ITER:WORD:BIT[,BIT...], WORD 0 or 1, bits 0-127)"


def fail(msg):
    print(msg)
    raise SystemExit(1)


def parse(argv):
    o = dict(num_blocks=25, max_itrs=1000, conv=0.001, matrix_file=DEFAULT_MTX, synthetic=None, target="cpu",
             mode="none", flips=0, kind="ANY", seed=None, quiet=False, flip_at=None, fmt="csr", list=False,
             rhs=1, check_every=0, check_tol=1e-7, max_rollbacks=3, flip_vector=[], precond="none",
             vector_ecc="none", block_fused=False, device_loop=0, structure_ecc="none", flip_structure=[],
             trail_ecc="none", flip_trail=[], verify_matrix=0, flip_matrix=[])

    def num(s, conv):
        try:
            return conv(s)
        except ValueError:
            return -1

    i = 1
    while i < len(argv):
        a = argv[i]

        def arg(msg):
            nonlocal i
            i += 1
            if i >= len(argv):
                fail(msg)
            return argv[i]

        if a in ("--convergence", "-c"):
            o["conv"] = num(arg("Invalid convergence threshold"), float)
            if o["conv"] < 0:
                fail("Invalid convergence threshold")
        elif a in ("--iterations", "-i"):
            o["max_itrs"] = num(arg("Invalid number of iterations"), int)
            if o["max_itrs"] < 0:
                fail("Invalid number of iterations")
        elif a in ("--list", "-l"):
            o["list"] = True
        elif a in ("--num-blocks", "-b"):
            o["num_blocks"] = num(arg("Invalid number of blocks"), int)
            if o["num_blocks"] < 1:
                fail("Invalid number of blocks")
        elif a in ("--matrix-file", "-f"):
            o["matrix_file"] = arg("Matrix filename required")
        elif a in ("--mode", "-m"):
            o["mode"] = arg("ABFT mode required")
        elif a in ("--target", "-t"):
            o["target"] = arg("Implementation target required")
        elif a in ("--inject-bitflip", "-x"):
            o["flips"] = 1
            while i + 1 < len(argv) and not argv[i + 1].startswith("-"):
                i += 1
                if argv[i] in ("INDEX", "VALUE"):
                    o["kind"] = argv[i]
                else:
                    o["flips"] = num(argv[i], int)
                    if o["flips"] < 1:
                        fail("Invalid bit-flip parameter")
        elif a in ("--synthetic", "-s"):
            o["synthetic"] = arg("Synthetic matrix specification required")
        elif a == "--format":
            o["fmt"] = arg("Format required")
            if o["fmt"] not in ("csr", "coo"):
                fail("Invalid format")
        elif a == "--seed":
            o["seed"] = num(arg("Invalid seed"), int)
            if o["seed"] < 0:
                fail("Invalid seed")
        elif a == "--flip-at":
            try:
                idx, bits = arg("Invalid --flip-at (want INDEX:BIT[,BIT...])").split(":")
                o["flip_at"] = (o["flip_at"] or []) + [(int(idx), [int(b) for b in bits.split(",")])]  # repeatable: one element each
            except ValueError:
                fail("Invalid --flip-at (want INDEX:BIT[,BIT...])")
        elif a == "--rhs":
            o["rhs"] = num(arg("Invalid number of right-hand sides"), int)
            if not 1 <= o["rhs"] <= 8:
                fail("Invalid number of right-hand sides")
        elif a == "--check-every":
            o["check_every"] = num(arg("Invalid residual check interval"), int)
            if o["check_every"] < 0:
                fail("Invalid residual check interval")
        elif a == "--check-tol":
            o["check_tol"] = num(arg("Invalid residual check tolerance"), float)
            if not (0 < o["check_tol"] < math.inf):
                fail("Invalid residual check tolerance")
        elif a == "--max-rollbacks":
            o["max_rollbacks"] = num(arg("Invalid number of rollbacks"), int)
            if o["max_rollbacks"] < 0:
                fail("Invalid number of rollbacks")
        elif a == "--flip-vector":
            msg = FLIP_VECTOR_MSG
            try:
                itr, vec, idx, bits = arg(msg).split(":")
                flip = (int(itr), vec, int(idx), [int(b) for b in bits.split(",")])
            except ValueError:
                fail(msg)
            if flip[0] < 0 or flip[1] not in ("x", "r", "p", "w", "b") or flip[2] < 0 or \
                    not all(0 <= b < 64 for b in flip[3]):
                fail(msg)  # (w and b: only with --vector-ecc secded, checked once every argument is read)
            o["flip_vector"] = o["flip_vector"] + [flip]
        elif a == "--precond":
            o["precond"] = arg("Invalid preconditioner (want none or jacobi)")
            if o["precond"] not in ("none", "jacobi"):
                fail("Invalid preconditioner (want none or jacobi)")
        elif a == "--vector-ecc":
            o["vector_ecc"] = arg("Invalid vector protection (want none or secded)")
            if o["vector_ecc"] not in ("none", "secded"):
                fail("Invalid vector protection (want none or secded)")
        elif a == "--structure-ecc":
            o["structure_ecc"] = arg("Invalid structure protection (want none or secded)")
            if o["structure_ecc"] not in ("none", "secded"):
                fail("Invalid structure protection (want none or secded)")
        elif a == "--flip-structure":
            msg = FLIP_STRUCTURE_MSG
            try:
                itr, kind, idx, bits = arg(msg).split(":")
                flip = (int(itr), kind, int(idx), [int(b) for b in bits.split(",")])
            except ValueError:
                fail(msg)
            if flip[0] < 0 or flip[1] not in ("row", "block") or flip[2] < 0 or \
                    not all(0 <= b < (64 if flip[1] == "row" else 128) for b in flip[3]):
                fail(msg)
            o["flip_structure"] = o["flip_structure"] + [flip]
        elif a == "--trail-ecc":
            o["trail_ecc"] = arg("Invalid trail protection (want none or secded)")
            if o["trail_ecc"] not in ("none", "secded"):
                fail("Invalid trail protection (want none or secded)")
        elif a == "--flip-trail":
            try:
                itr, word, bits = arg(FLIP_TRAIL_MSG).split(":")
                flip = (int(itr), int(word), [int(b) for b in bits.split(",")])
            except ValueError:
                fail(FLIP_TRAIL_MSG)
            if flip[0] < 0 or flip[1] not in (0, 1) or not all(0 <= b < 128 for b in flip[2]):
                fail(FLIP_TRAIL_MSG)
            o["flip_trail"] = o["flip_trail"] + [flip]
        elif a == "--verify-matrix":
            o["verify_matrix"] = num(arg("Invalid --verify-matrix interval (want a whole number >= 1)"), int)
            if o["verify_matrix"] < 1:
                fail("Invalid --verify-matrix interval (want a whole number >= 1)")
        elif a == "--flip-matrix":
            try:
                itr, seg, word, bits = arg(FLIP_MATRIX_MSG).split(":")
                flip = (int(itr), seg, int(word), [int(b) for b in bits.split(",")])
            except ValueError:
                fail(FLIP_MATRIX_MSG)
            if flip[0] < 0 or not flip[1] or flip[2] < 0 or not all(b >= 0 for b in flip[3]):
                fail(FLIP_MATRIX_MSG)
            o["flip_matrix"] = o["flip_matrix"] + [flip]
        elif a == "--block-fused":
            o["block_fused"] = True
        elif a == "--device-loop":
            o["device_loop"] = num(arg("Invalid --device-loop stride (want a whole number >= 1)"), int)
            if o["device_loop"] < 1:
                fail("Invalid --device-loop stride (want a whole number >= 1)")
        elif a in ("--quiet", "-q"):
            o["quiet"] = True
        elif a in ("--help", "-h"):
            sys.stdout.write(USAGE % os.path.basename(argv[0]))
            raise SystemExit(0)
        else:
            fail("Unrecognized argument '%s' (try '--help')" % a)
        i += 1
    if o["block_fused"] and o["rhs"] < 2:
        fail("--block-fused needs --rhs K with K of 2 to 8: it selects the block loop's fused iteration")
    if o["device_loop"]:
        for flag, on in (("--rhs", o["rhs"] > 1), ("--precond", o["precond"] != "none"),
                         ("--check-every", o["check_every"] > 0), ("--vector-ecc", o["vector_ecc"] != "none"),
                         ("--flip-vector", bool(o["flip_vector"]))):
            if on:
                fail("--device-loop cannot be combined with %s" % flag)
    if o["trail_ecc"] == "secded" and not o["device_loop"]:
        fail("--trail-ecc secded needs --device-loop S: it protects the scalar trail of the device loop")
    if o["flip_trail"] and o["trail_ecc"] != "secded":
        fail("--flip-trail needs --trail-ecc secded")
    if o["vector_ecc"] == "none":
        if any(f[1] in ("w", "b") for f in o["flip_vector"]):
            fail(FLIP_VECTOR_MSG)  # (known only here: --vector-ecc may follow --flip-vector)
    else:
        for flag, on in (("--rhs", o["rhs"] > 1), ("--precond", o["precond"] != "none"),
                         ("--check-every", o["check_every"] > 0), ("--format coo", o["fmt"] != "csr")):
            if on:
                fail("--vector-ecc secded cannot be combined with %s" % flag)
    if o["structure_ecc"] == "none":
        if o["flip_structure"]:
            fail("--flip-structure needs --structure-ecc secded")
    else:
        for flag, on in (("--rhs", o["rhs"] > 1), ("--format coo", o["fmt"] != "csr")):
            if on:
                fail("--structure-ecc secded cannot be combined with %s" % flag)
    return o


def header(o, n, block, nnz):
    print()
    print("implementation        = %s-%s" % (o["target"], o["mode"]))
    print("matrix size           = %u x %u" % (n, n))
    print("matrix block size     = %u x %u" % (block, block))
    print("number of non-zeros   = %u (%.4f%%)" % (nnz, nnz / (float(n) * float(n)) * 100))
    print("maximum iterations    = %u" % o["max_itrs"])
    print("convergence threshold = %g" % o["conv"])
    print()


def bit_range(fmt, kind):
    if fmt == "csr":
        return {"ANY": (0, 96), "VALUE": (0, 64), "INDEX": (64, 96)}[kind]
    return {"ANY": (0, 128), "VALUE": (64, 128), "INDEX": (0, 64)}[kind]


def draw_flips(o, nnz):
    """-> [(index, [bits]), ...]: --flip-at's elements in the order given, or one element drawn in the reference's rand() order"""
    if o["flip_at"] is not None:
        return o["flip_at"]
    if not o["flips"]:
        return []
    libc = ctypes.CDLL(None)
    libc.srand(o["seed"] if o["seed"] is not None else int(time.time()))
    index = libc.rand() % nnz
    lo, hi = bit_range(o["fmt"], o["kind"])
    return [(index, [libc.rand() % (hi - lo) + lo for _ in range(o["flips"])])]


def vector_flips(o, length, vecs):
    """--flip-vector's flips as {iteration: [(vector, index, bits)]}, each index checked against the length"""
    out = {}
    for itr, name, index, bits in o["flip_vector"]:
        if index >= length:
            fail("Invalid --flip-vector: index %d outside a vector of %d entries" % (index, length))
        out.setdefault(itr, []).append((name, vecs[name], index, bits))
    return out


def apply_vector_flips(ctx, flips, itr):
    for name, v, index, bits in flips.get(itr, ()):
        for bit in bits:
            print("*** flipping bit %d of %s[%d] ***" % (bit, name, index))
        ctx.flip_vector(v, index, bits)


def structure_flips(o, ctx, A):
    """--flip-structure's flips as {iteration: [(kind, index, bits)]}, each index checked against the stored words"""
    out = {}
    if not o["flip_structure"]:
        return out
    ext, blk = ctx.read_structure(A)
    for itr, kind, index, bits in o["flip_structure"]:
        count = len(ext) if kind == "row" else len(blk)
        if index >= count:
            fail("Invalid --flip-structure: %s %d outside the matrix's %d" % (kind, index, count))
        out.setdefault(itr, []).append((kind, index, bits))
    return out


def apply_structure_flips(ctx, A, flips, itr):
    for kind, index, bits in flips.get(itr, ()):
        for bit in bits:
            print("*** flipping bit %d of row %s %d ***" % (bit, "extent" if kind == "row" else "block", index))
        ctx.flip_structure(A, kind, index, bits)


def matrix_flips(o, ctx, A):
    """--flip-matrix's flips in the order of their iterations, [(iteration, segment, {word: [bits 0..31]})], each
    checked against the segments the matrix has"""
    out = []
    if not o["flip_matrix"]:
        return out
    sizes = dict(ctx.matrix_segments(A))
    for itr, seg, word, bits in o["flip_matrix"]:
        if seg not in sizes:
            fail("Invalid --flip-matrix: the matrix has no segment '%s' (it has %s)" % (seg, ", ".join(sizes)))
        words = {}
        for b in bits:  # a bit past 31 lies in a following word
            words.setdefault(word + b // 32, []).append(b % 32)
        if 4 * max(words) >= sizes[seg]:
            fail("Invalid --flip-matrix: word %d outside segment '%s' of %d bytes" % (max(words), seg, sizes[seg]))
        out.append((itr, seg, words))
    return sorted(out, key=lambda f: f[0])


def apply_matrix_flips(ctx, A, flips, reached):
    """the flips whose iteration `reached` says has been run, taken off the list"""
    while flips and reached(flips[0][0]):
        _, seg, words = flips.pop(0)
        for word, bits in sorted(words.items()):
            for bit in bits:
                print("*** flipping bit %d of word %d of matrix segment %s ***" % (bit, word, seg))
            ctx.flip_segment(A, seg, word, bits)


def print_matrix_digests(o, ctx, A):
    if o["verify_matrix"]:
        ctx.arm_matrix(A)  # behind the injected element flips, as the preconditioner: the matrix the solve runs on
        segs = ctx.matrix_segments(A)
        print("matrix digests: %d segments, %d bytes, every %d iterations"
              % (len(segs), sum(size for _, size in segs), o["verify_matrix"]))


def report_check(checks, prefix, itr, gap, ok, back, bound):
    """one line per failed residual check; the counts for print_check_summary"""
    checks[ok] = checks.get(ok, 0) + 1
    if not ok:
        print("%s[ABFT] residual check failed at iteration %d: gap %.1e > %.1e; rolled back to %s"
              % (prefix, itr, gap, bound, "the start" if back < 0 else "iteration %d" % back))


def print_check_summary(checks):
    print("residual checks: %d passed, %d failed" % (checks.get(True, 0), checks.get(False, 0)))


def make_preconditioner(o, ctx, A):
    """--precond: None, or the Jacobi vector (after the injected flips: it sees the matrix the solve runs on)"""
    if o["precond"] == "none":
        return None
    try:
        dinv = ctx.jacobi(A)
    except ValueError as e:
        ctx.close()
        fail(str(e))
    print("preconditioner: jacobi")
    return dinv


def main(argv=None):
    argv = sys.argv if argv is None else argv
    o = parse(argv)
    from . import MODES
    if o["list"]:
        print("\nRegistered contexts:")
        for m in list(MODES) + ["sec"]:
            print("\thip-%s" % m)
        print()
        return 0
    if o["target"] != "hip" or o["mode"] not in list(MODES) + ["sec"]:
        sys.stderr.write("\nNo implementation found for %s-%s\n\n" % (o["target"], o["mode"]))
        return 1
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        fail("several ranks: run host/cg-csr or host/cg-coo under this launcher (--no-python); "
             "this Python driver is single-GPU")
    if o["rhs"] > 1:
        if o["fmt"] != "csr":
            fail("--rhs with more than one right-hand side needs --format csr")
        return run_block(o)
    return run_single(o)


def load_matrix(o, row0=0, row1=None):
    from . import generators
    if o["synthetic"]:
        try:
            n = generators.dim(o["synthetic"])
        except ValueError:
            fail("Invalid synthetic matrix '%s'" % o["synthetic"])
        cols, rows, vals, n = generators.generate(o["synthetic"], row0, n if row1 is None else row1)
        return cols, rows, vals, n, n
    try:
        cols, rows, vals, n, block = generators.load_mtx(o["matrix_file"], o["num_blocks"])
    except FileNotFoundError:
        fail("Failed to open '%s'" % o["matrix_file"])
    except ValueError as e:
        fail(str(e))
    if row1 is not None:
        m = (rows >= row0) & (rows < row1)
        cols, rows, vals = cols[m], rows[m], vals[m]
    return cols, rows, vals, n, block


def run_single(o):
    from . import HIPContext, generators
    from . import capi
    from .context import ResidualCheckFailed, cg_solve, cg_solve_device
    cols, rows, vals, n, block = load_matrix(o)
    nnz = len(vals)
    ctx = HIPContext(o["mode"], o["fmt"])
    ecc = o["vector_ecc"] == "secded"
    secc = o["structure_ecc"] == "secded"
    # (protected vectors and a protected row structure run on the streaming layout only)
    try:
        A = ctx.create_matrix(cols, rows, vals, n, nnz, layout="stream" if ecc or secc else None,
                              **({"structure_ecc": True} if secc else {}))
    except capi.AbftError as e:
        if not secc or e.code != capi.ERR_RANGE:
            raise
        ctx.close()
        fail(str(e))
    del cols, rows, vals
    header(o, n, block, nnz)
    b, x, r, p, w = (ctx.create_vector(n) for _ in range(5))
    ctx.upload(b, generators.reference_rhs(n))
    ctx.upload(x, np.zeros(n))
    for index, bits in draw_flips(o, nnz):
        for bit in bits:
            print("*** flipping bit %d at index %d ***" % (bit, index))
        ctx.inject_at(A, index, bits)
    vecs = vector_flips(o, n, {"x": x, "r": r, "p": p, "w": w, "b": b})
    sflips = structure_flips(o, ctx, A)
    mflips = matrix_flips(o, ctx, A)
    dinv = make_preconditioner(o, ctx, A)
    if ecc:
        print("vector protection: secded (64, 57)")
    if secc:
        print("structure protection: secded (row extents (64, 57), row blocks (128, 120))")
    bound = o["check_tol"] * float(np.linalg.norm(generators.reference_rhs(n)))
    checks = {}

    def line(itr, rr):
        if not o["quiet"]:
            print("iteration %5u :  rr = %12.4f" % (itr, rr))
        apply_vector_flips(ctx, vecs, itr)
        apply_structure_flips(ctx, A, sflips, itr)
        if not o["device_loop"]:
            apply_matrix_flips(ctx, A, mflips, lambda i: i <= itr)

    if o["device_loop"]:
        print("iteration loop: device scalars, stride %d" % o["device_loop"])
    tecc = o["trail_ecc"] == "secded"
    if tecc:
        print("scalar trail: secded (128, 120)")
    tflips = sorted(o["flip_trail"])

    def flip_trail(done, trail):
        # the record handed to the batch after iteration I's: record `stride` of pairs, once I's batch is behind us
        while tflips and tflips[0][0] < done:
            _, word, bits = tflips.pop(0)
            ctx.flip_trail(trail, 2 * o["device_loop"] + word, bits)

    def after_batch(done, trail):
        if tecc:
            flip_trail(done, trail)
        apply_matrix_flips(ctx, A, mflips, lambda i: i < done)  # after iteration I's batch, as --flip-trail

    print_matrix_digests(o, ctx, A)
    mcheck = {"matrix_check_every": o["verify_matrix"]} if o["verify_matrix"] else {}
    t0 = time.perf_counter()
    try:
        if o["device_loop"]:
            itr, rr = cg_solve_device(ctx, A, b, x, r, p, w, o["max_itrs"], o["conv"], on_iteration=line,
                                      stride=o["device_loop"], **mcheck,
                                      **({"trail_ecc": True} if tecc else {}),
                                      **({"on_batch": after_batch} if tecc or mflips else {}))
        else:
            itr, rr = cg_solve(ctx, A, b, x, r, p, w, o["max_itrs"], o["conv"], on_iteration=line,
                               check_every=o["check_every"], check_tol=o["check_tol"],
                               max_rollbacks=o["max_rollbacks"],
                               on_check=lambda i, gap, ok, back: report_check(checks, "", i, gap, ok, back, bound),
                               precond=dinv, **({"vector_ecc": True} if ecc else {}), **mcheck)
    except ResidualCheckFailed as e:
        print("[ABFT] %s" % e)
        ctx.close()
        return 1
    ms = (time.perf_counter() - t0) * 1e3
    print("\nran for %u iterations" % itr)
    if o["check_every"]:
        print_check_summary(checks)
    if o["verify_matrix"]:
        print("matrix verifications: %d passed" % ctx.matrix_verifications)
    if secc:  # every stored word once more, those no SpMV reads as well
        print("structure scrub: %d corrected" % ctx.scrub_structure(A)[0])
    print("\ntime taken = %7.2f ms\n" % ms)
    if ecc:
        from .context import vecc_strip
        ctx.spmv_vecc(A, x, r)
        err = np.abs(vecc_strip(ctx.download(b)) - vecc_strip(ctx.download(r)))
    else:
        ctx.spmv(A, x, r)
        err = np.abs(ctx.download(b) - ctx.download(r))
    print("total error = %f" % math.sqrt(float((err * err).sum())))
    print("max error   = %f" % (float(err.max()) if n else 0.0))
    print()
    ctx.destroy_matrix(A)
    ctx.close()
    return 0


def run_block(o):
    """run_single for o["rhs"] right-hand sides at once (cg_solve_block): the matrix in the streaming
    layout, one line of K residuals per iteration, a `ran for` line and the errors per column."""
    from . import HIPContext, generators
    from .context import ResidualCheckFailed, cg_solve_block
    K = o["rhs"]
    cols, rows, vals, n, block = load_matrix(o)
    nnz = len(vals)
    ctx = HIPContext(o["mode"], "csr")
    A = ctx.create_matrix(cols, rows, vals, n, nnz, layout="stream")
    del cols, rows, vals
    header(o, n, block, nnz)
    b, x, r, p, w = (ctx.create_block(n, K) for _ in range(5))
    ctx.upload(b, np.stack([generators.reference_rhs(n, seed=1 + j) for j in range(K)], axis=1))
    ctx.upload(x, np.zeros((n, K)))
    for index, bits in draw_flips(o, nnz):
        for bit in bits:
            print("*** flipping bit %d at index %d ***" % (bit, index))
        ctx.inject_at(A, index, bits)

    vecs = vector_flips(o, n * K, {"x": x, "r": r, "p": p})
    mflips = matrix_flips(o, ctx, A)
    dinv = make_preconditioner(o, ctx, A)
    if o["block_fused"]:
        print("block iteration: fused")
    bounds = [o["check_tol"] * float(np.linalg.norm(generators.reference_rhs(n, seed=1 + j))) for j in range(K)]
    checks = {}

    def line(itr, rr, active):
        if not o["quiet"]:
            print("iteration %5u :  rr = %s" % (itr, " ".join("%12.4f" % v for v in rr)))
        apply_vector_flips(ctx, vecs, itr)
        apply_matrix_flips(ctx, A, mflips, lambda i: i <= itr)

    def on_check(i, gap, ok, back, j):
        report_check(checks, "rhs %u: " % j, i, gap, ok, back, bounds[j])

    print_matrix_digests(o, ctx, A)
    t0 = time.perf_counter()
    try:
        itrs, _ = cg_solve_block(ctx, A, b, x, r, p, w, o["max_itrs"], o["conv"], on_iteration=line,
                                 check_every=o["check_every"], check_tol=o["check_tol"],
                                 max_rollbacks=o["max_rollbacks"], on_check=on_check, precond=dinv,
                                 **({"fused": True} if o["block_fused"] else {}),
                                 **({"matrix_check_every": o["verify_matrix"]} if o["verify_matrix"] else {}))
    except ResidualCheckFailed as e:
        print("[ABFT] %s" % e)
        ctx.close()
        return 1
    ms = (time.perf_counter() - t0) * 1e3
    print()
    for j in range(K):
        print("rhs %u: ran for %u iterations" % (j, itrs[j]))
    if o["check_every"]:
        print_check_summary(checks)
    if o["verify_matrix"]:
        print("matrix verifications: %d passed" % ctx.matrix_verifications)
    print("\ntime taken = %7.2f ms (%u right-hand sides)\n" % (ms, K))
    ctx.spmm(A, x, r, K)
    err = np.abs(ctx.download(b) - ctx.download(r))
    for j in range(K):
        e = err[:, j]
        print("rhs %u: total error = %f" % (j, math.sqrt(float((e * e).sum()))))
        print("rhs %u: max error   = %f" % (j, float(e.max()) if n else 0.0))
    print()
    ctx.destroy_matrix(A)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
