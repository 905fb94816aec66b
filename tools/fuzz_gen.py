"""The case generators of tools/fuzz_parity.py, apart from its GPU half: numpy only, importable
without the library (tests/test_fuzz_generator.py classifies their draws on the CPU).

`legacy_draw` is the campaign's first family, draw for draw (a seed means what it always meant).

`packed_case` is the second family: matrices whose row blocks *pack* (CsrPacked: at most 16
distinct value patterns per block and a column span that fits the bits the palette index leaves),
sit on either side of every span threshold, or are built never to pack; and sequences of up to 40
flips that move the planner's state (abft_hip_inject re-plans the block it flips).

What the generator knows about the library is the documented rule only: a block is a contiguous run
of whole rows of at most one tile of elements (ABFT_CSR_TILE).  It has no copy of the cutting of
blocks; where it wants "the same block" it takes elements a few positions apart, and its two
one-sided predictions (`mark`) are statements about every window of WINDOW consecutive elements."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _ieee import csr_tile  # noqa: E402  (reads ABFT_BLOCK * ABFT_CFG_CSR_EPT from abft_internal.h)

CSR, COO = 0, 1
MODES = ["none", "constraints", "sed", "sec7", "sec8", "secded"]
NBITS = {CSR: 96, COO: 128}

TILE = csr_tile()
# The one-sided rules look at the aligned stretches [j * TILE, (j + 2) * TILE): every window of TILE
# consecutive elements lies inside one of them, so a bound that holds for each stretch holds for every
# window (an upper bound on the tile only makes the rule stricter).
WINDOW = 2 * TILE

M_CHOICES = [1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 18, 40]
M_OF_K = {0: [1], 1: [2], 2: [3, 4], 3: [5, 8], 4: [9, 15, 16]}

# distinct bit patterns are distinct palette entries: +-0.0 are two, every NaN payload is one
SPECIALS = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                     0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x80002E0000000000,
                     0x7FF8000000000001, 0xFFF0000000000123, 0x7FF0000000000001, 0xFFF8000000001234,
                     0x7FF800000000BEEF], np.uint64)

# what the campaign's summary counts; a short run must reach every one of them
CLASSES = ["packed_at_creation", "k0", "k1", "k2", "k3", "k4", "replan_kept", "demoted_by_palette",
           "demoted_by_span", "inject_before_parts", "shard", "spmm"]


# ------------------------------------------------------------------ first family --

def legacy_matrix(rng):
    sizes = [1, 2, 7, 64, 300, 1000, 3000, 6000]
    if os.environ.get("ABFT_FUZZ_BIG") == "1":  # fewer, larger cases (several row blocks per XCD, long sweeps)
        sizes = [20000, 60000, 150000]
    n = int(rng.choice(sizes))
    kind = rng.integers(0, 3)
    rows, cols = [], []
    if n >= 20000:  # vectorised draw for the large cases: k entries per row, duplicates removed
        k = rng.choice([0, 1, 2, 3, 5, 8, 30], size=n)
        r = np.repeat(np.arange(n), k)
        c = rng.integers(0, n, size=len(r))
        key = np.unique(r.astype(np.int64) * n + c)
        rows, cols = [key // n], [key % n]
    else:
        for r in range(n):
            if kind == 0:
                k = int(rng.choice([0, 1, 2, 3, 5, 8]))
            elif kind == 1:
                k = int(rng.choice([0, 0, 1, 4, 30, 200])) if rng.random() < 0.98 else int(rng.integers(1000, 4000))
            else:
                k = int(rng.integers(0, 12))
            k = min(k, n)
            c = np.sort(rng.choice(n, size=k, replace=False))
            rows.append(np.full(k, r))
            cols.append(c)
    rows = np.concatenate(rows) if rows else np.zeros(0)
    cols = np.concatenate(cols) if cols else np.zeros(0)
    vals = rng.standard_normal(len(rows)) * 10.0 ** rng.integers(-3, 4, size=len(rows))
    return cols.astype(np.uint32), rows.astype(np.uint32), vals, n


def legacy_draw(rng):
    """Everything a case of the first family draws before it touches the GPU, in the order it always
    drew it -> dict(cols, rows, vals, n, fmt, mode, layout, env, flips, x).  (The SpMV-in-two-parts
    draws follow from the same generator, in fuzz_parity.one_case.)"""
    cols, rows, vals, n = legacy_matrix(rng)
    nnz = len(vals)
    fmt = CSR if rng.random() < 0.6 else COO
    mode = str(rng.choice(MODES))
    if os.environ.get("ABFT_FUZZ_ONLY"):  # e.g. coo:constraints -- a campaign on one format and mode
        f, mode = os.environ["ABFT_FUZZ_ONLY"].split(":")
        fmt = COO if f == "coo" else CSR
    layout = str(rng.choice(["stream", "panels", "sweep", "slice", "slice", "auto"]))
    env = {}
    env["ABFT_HIP_SLICE_ROWS"] = str(int(rng.choice([16, 64, 256, 1024])))
    env["ABFT_HIP_SLICE_LAG"] = str(int(rng.choice([0, 1, 2, 3])))
    env["ABFT_HIP_SWEEP_RPT"] = str(int(rng.choice([8, 16])))
    env["ABFT_HIP_SWEEP_LAG"] = str(int(rng.choice([0, 1, 2, 3])))
    env["ABFT_HIP_LAYOUT"] = layout
    env["ABFT_HIP_PANEL_WIDTH"] = str(int(rng.choice([16, 100, 257, 4096])))
    env["ABFT_HIP_PANEL_CHUNK"] = str(int(rng.choice([0, 1, 2, 3])))
    # round 4, COO panel layout: all panels in one launch paced by the per-XCD board (lag > 0; overrides the chunking),
    # workgroups that take several groups in turn, and the opt-in kernels (producer / consumer waves, cold paths out of
    # the hot loop, the x prefetch)
    env["ABFT_HIP_PANEL_LAG"] = str(int(rng.choice([0, 0, 1, 2, 3])))
    env["ABFT_HIP_PANEL_GRID"] = str(int(rng.choice([1, 2, 3, 1000000])))
    kern = int(rng.integers(0, 4))
    env["ABFT_HIP_COO_PC"] = "1" if kern == 1 else "0"
    env["ABFT_HIP_COO_LEAN"] = "1" if kern == 2 else "0"
    env["ABFT_HIP_PANEL_XPF"] = str(int(rng.integers(0, 2)))
    flips = random_flips(rng, fmt, mode, n, nnz)
    x = rng.standard_normal(n)
    return dict(cols=cols, rows=rows, vals=vals, n=n, fmt=fmt, mode=mode, layout=layout, env=env, flips=flips, x=x)


def random_flips(rng, fmt, mode, n, nnz):
    """the first family's flips: 0..3 single or double flips anywhere in the stored words"""
    flips = []
    if nnz and (mode not in ("none", "constraints") or rng.random() < 0.7):
        near = int(rng.integers(0, nnz))
        for _ in range(int(rng.integers(0, 4))):
            idx = int(rng.integers(0, nnz))
            if rng.random() < 0.3:  # neighbours in the caller's order (the constraints checks compare those)
                idx = min(nnz - 1, near + int(rng.integers(0, 3)))
            nb = 1 if rng.random() < 0.7 else 2
            if fmt == COO and rng.random() < 0.5:
                # low column bits: the element lands in another output of the vector (the
                # reference scatters there; undetected in none / as a double flip in sec7, sec8)
                hi_bit = max(2, int(n).bit_length())
                nb = min(nb if mode in ("none", "constraints") else 2, hi_bit)
                flips.append((idx, [int(b) for b in rng.choice(hi_bit, size=nb, replace=False)]))
            else:
                flips.append((idx, [int(b) for b in rng.choice(NBITS[fmt], size=nb, replace=False)]))
    return flips


# ----------------------------------------------------------------- second family --

class Case:
    """One case of the packed family.  Matrix as sorted (row, col) triplets (a shard: its rows
    re-based, `n_in` columns, `index_base` the global index of its first element).  `flips`:
    [(element, bits, class)] in order, `checks`: the flip counts after which everything is compared.
    `mark`: "all" / "none" / None -- the one-sided prediction the case was built for.  `classes`:
    what the generator's model says the case reaches, `eligible`: what it could have reached."""


def _bits_of(word):
    return [int(b) for b in range(64) if (int(word) >> b) & 1]


def value_pool(rng, m, salted):
    """m distinct 64-bit patterns: small multiples of 1/4 (whose pairwise XORs have few set bits: one
    inject turns one into another), random magnitudes, and in a salted pool the IEEE specials"""
    simple = (rng.integers(-16, 17, size=3 * m + 8) * 0.25).view(np.uint64)
    wide = (rng.standard_normal(3 * m + 8) * 10.0 ** rng.integers(-3, 4, size=3 * m + 8)).view(np.uint64)
    cand = np.where(rng.random(3 * m + 8) < 0.5, simple, wide)
    if salted:
        cand = np.concatenate([rng.permutation(SPECIALS)[:int(rng.integers(1, min(m, 6) + 1))], cand])
    cand = np.concatenate([cand, rng.standard_normal(m).view(np.uint64)])  # (enough distinct ones whatever came before)
    _, first = np.unique(cand, return_index=True)
    return cand[np.sort(first)][:m]


def _band(rng, n, offs, ragged, empty, long_row):
    """rows r with columns r + offs inside [0, n); some elements of `ragged` row ranges dropped, whole
    rows dropped, one row widened to `long_row` consecutive columns -> sorted keys row * n + col"""
    offs = np.asarray(sorted(set(int(o) for o in offs)), np.int64)
    r = np.repeat(np.arange(n, dtype=np.int64), len(offs))
    c = r + np.tile(offs, n)
    keep = (c >= 0) & (c < n)
    if ragged:
        for _ in range(int(rng.integers(1, 4))):
            a = int(rng.integers(0, n))
            b = min(n, a + int(rng.integers(1, max(2, n // 3))))
            keep &= ~((r >= a) & (r < b) & (rng.random(len(r)) < 0.4))
    if empty:
        gone = np.zeros(n, bool)
        gone[rng.random(n) < 0.01] = True
        a = int(rng.integers(0, n))
        gone[a:a + int(rng.integers(1, 40))] = True
        keep &= ~gone[r]
    key = r[keep] * n + c[keep]
    if long_row and n > long_row + 2:
        lr = int(rng.integers(0, n))
        c0 = int(rng.integers(0, n - long_row))
        key = np.union1d(key, lr * n + np.arange(c0, c0 + long_row, dtype=np.int64))
    return key


def _structure(rng, kind):
    """-> (keys, n, band spread or None)"""
    if kind == "tiny":
        n = int(rng.choice([1, 2, 7, 40, 300]))
        r = np.repeat(np.arange(n, dtype=np.int64), rng.choice([0, 1, 2, 3, 5, 8], size=n))
        return np.unique(r * n + rng.integers(0, n, size=len(r))), n, None
    if kind == "none_values":  # every row holds 17..40 elements (their values all distinct, see _values)
        n = int(rng.choice([50, 120, 400]))
        length = rng.integers(17, 41, size=n)
        r = np.repeat(np.arange(n, dtype=np.int64), length)
        j = np.arange(len(r)) - np.repeat(np.cumsum(length) - length, length)
        start = np.repeat(rng.integers(0, n - 40, size=n), length)
        return r * n + start + j, n, None
    if kind == "none_span":  # every row spans 65536 columns or more: r and r + D, wrapped around
        n = int(rng.integers(135000, 150001))
        d = int(rng.integers(65536, n - 65536 + 1)) if rng.random() < 0.5 else int(rng.choice([65536, n - 65536]))
        r = np.arange(n, dtype=np.int64)
        key = np.concatenate([r * n + r, r * n + (r + d) % n])
        if rng.random() < 0.5:
            key = np.concatenate([key, r * n + (r + 1) % n])
        return np.unique(key), n, None
    q = int(rng.choice([1, 2, 3, 5, 7, 9, 4]))  # an odd count: blocks start at odd element indices
    if kind == "all":  # narrow band: every stretch of WINDOW elements spans far fewer than 2^12 columns
        spread = int(rng.integers(0, 600))
        n = int(rng.choice([300, 3000, 20000, 70000])) + spread
        empty, long_row = rng.random() < 0.3, 0
    else:  # "band": the largest offset around a span threshold, for the diagonal alone and for a block of rows
        p = int(rng.integers(11, 17))
        rb = max(1, TILE // q)  # rows of a block of full rows
        adj = int(rng.choice([0, 0, rb - 1, rb, rb + 1, int(rng.integers(0, 2 * rb + 1))]))
        spread = max(q, (1 << p) + int(rng.integers(-3, 4)) - adj)
        n = spread + int(rng.integers(4 * rb, 30 * rb + 200))
        if rng.random() < 0.05:
            n = 150000
        empty, long_row = rng.random() < 0.4, (int(rng.choice([TILE + 1, 1500, 3000])) if rng.random() < 0.3 else 0)
    lo = -int(rng.integers(0, 4))
    offs = [lo, lo + spread] + [lo + int(v) for v in rng.integers(0, spread + 1, size=max(0, q - 2))]
    return _band(rng, n, offs[:max(1, q)], rng.random() < 0.6, empty, long_row), n, spread


def _values(rng, kind, rows, nnz, focus_k):
    """-> (value patterns, [(first, end, m, pool offset)] the value segments, the focus segment's index or None).
    Inside a segment of m values every m consecutive elements hold all m of them (in a drawn order), so a block
    of at least 2 m - 1 of its elements holds exactly m distinct patterns."""
    if kind == "none_values":  # element j of a row takes pool entry (row + j) mod 40: 17..40 distinct per row
        pool = value_pool(rng, 40, rng.random() < 0.5)
        j = np.arange(nnz) - np.searchsorted(rows, rows, side="left")
        return pool[(rows + j) % 40], [(0, nnz, 40, 0)], None
    choices = [v for v in M_CHOICES if v <= 16] if kind == "all" else M_CHOICES  # ("all": no stretch with 17 values)
    m = int(rng.choice(choices))
    cuts = np.unique(rng.integers(0, nnz + 1, size=int(rng.integers(0, 6)))) if nnz else np.zeros(0, np.int64)
    focus = None
    if focus_k is not None and nnz >= 4 * TILE:  # one segment of 3 tiles or more with k = focus_k
        f0 = int(rng.integers(0, nnz - 3 * TILE + 1))
        f1 = min(nnz, f0 + 3 * TILE + int(rng.integers(0, nnz)))
        cuts = np.unique(np.concatenate([cuts[(cuts <= f0) | (cuts >= f1)], [f0, f1]]))
        focus = (f0, int(rng.choice(M_OF_K[focus_k])))
        m = max(m, focus[1])
    pool = value_pool(rng, m, rng.random() < 0.5)
    bounds = np.unique(np.concatenate([[0], cuts, [nnz]])).astype(np.int64)
    segs, vb, fidx = [], np.zeros(nnz, np.uint64), None
    for a, b in zip(bounds[:-1], bounds[1:]):
        a, b = int(a), int(b)
        ms = min(m, int(rng.choice(choices)))
        if focus and a == focus[0]:
            ms, fidx = focus[1], len(segs)
        off = int(rng.integers(0, m))
        groups = -(-(b - a) // ms)
        idx = np.argsort(rng.random((groups, ms)), axis=1).reshape(-1)[:b - a]
        vb[a:b] = pool[(off + idx) % m]
        segs.append((a, b, ms, off))
    return vb, segs, fidx


def _window_rules(cols, vb, rowptr):
    """the two one-sided rules, by brute force -> "all", "none" or None"""
    nnz = len(cols)
    lens = np.diff(rowptr)
    all_ok = nnz == 0 or int(lens.max()) <= TILE
    j = 0
    while all_ok and j < max(1, nnz):
        c, v = cols[j:j + WINDOW], vb[j:j + WINDOW]
        all_ok = len(c) == 0 or (len(np.unique(v)) <= 16 and int(c.max()) - int(c.min()) < 4096)
        j += TILE
    if all_ok:
        return "all"
    if nnz == 0 or int(lens.min()) == 0:
        return None
    first, last = cols[rowptr[:-1]].astype(np.int64), cols[rowptr[1:] - 1].astype(np.int64)  # columns ascend in a row
    wide = last - first >= 65536
    many = np.zeros(len(lens), bool)
    cand = np.flatnonzero(~wide & (lens > 16))
    if len(cand) == np.count_nonzero(~wide):
        for r in cand:  # (only the none_values kind comes here with more than a few rows)
            many[r] = len(np.unique(vb[rowptr[r]:rowptr[r + 1]])) > 16
    return "none" if bool(np.all(wide | many)) else None


def _plan_flips(rng, c, target):
    """The flips of a mode-none CSR case.  `target`: (first, end, m) of a value segment the model says packs,
    or None.  Works on copies of the columns and value patterns, so that a later flip sees the earlier ones."""
    nnz, n_in = len(c.vals), c.n_in
    if nnz == 0:
        return [], set()
    vb, cb = c.vals.view(np.uint64).copy(), c.cols.astype(np.int64).copy()
    budget = 40 if nnz <= 200000 else 12
    flips, reached, done = [], set(), []

    def emit(i, bits, cls):
        bits = sorted(set(int(b) for b in bits))[:32]
        if not bits:
            return
        for b in bits:
            if b < 64:
                vb[i] ^= np.uint64(1) << np.uint64(b)
            else:
                cb[i] ^= 1 << (b - 64)
        flips.append((int(i), bits, cls))
        done.append((int(i), bits))

    def place():
        if target and rng.random() < 0.85:
            a, b = target[0] + min(50, (target[1] - target[0]) // 4), target[1] - min(50, (target[1] - target[0]) // 4)
            return int(rng.integers(a, max(a + 1, b)))
        edge = rng.random()
        if edge < 0.1:
            return 0
        if edge < 0.2:
            return nnz - 1
        if edge < 0.4:  # the first or last element of a row: blocks begin and end there
            r = int(rng.integers(0, c.n))
            return int(min(nnz - 1, c.rowptr[r] if rng.random() < 0.5 else max(int(c.rowptr[r + 1]), 1) - 1))
        return int(rng.integers(0, nnz))

    def in_palette(i):
        """the bits that turn element i's value into that of an element a few places away"""
        for j in rng.permutation(np.arange(max(0, i - 12), min(nnz, i + 13))):
            bits = _bits_of(vb[i] ^ vb[j])
            if 0 < len(bits) <= 32:
                return bits
        return None

    def new_value(i):
        return [int(rng.integers(0, 52))]

    def column(i, how):
        if how == "inside":
            return [64 + int(rng.integers(0, 3))]
        if how == "past_shift":  # 2^10 .. 2^15: past the span of some shifts, inside that of others
            return [64 + int(rng.integers(10, 16))]
        if how == "below_base":  # clears the column's highest set bit
            return [64 + max(0, int(cb[i]).bit_length() - 1)]
        if how == "past_65535":
            return [64 + int(rng.integers(16, 18))]
        return [64 + int(rng.integers(min(31, int(n_in).bit_length()), 32))]  # past n_in

    def burst(i0, count):
        """`count` new values within 40 consecutive elements around i0: whichever blocks share them, one gets half"""
        a = max(0, min(i0, nnz - 40))
        for j, i in enumerate(rng.permutation(np.arange(a, min(nnz, a + 40)))[:count]):
            emit(i, [j % 52], "new_value")

    scenario = str(rng.choice(["mixed", "keep", "demote_palette", "demote_span", "column_then_values"]))
    if target is None and scenario != "mixed" and rng.random() < 0.5:
        scenario = "mixed"
    m = target[2] if target else 16
    i0 = place()
    if scenario == "keep":
        for _ in range(int(rng.integers(2, 9))):
            i = min(nnz - 1, i0 + int(rng.integers(0, 30)))
            bits = in_palette(i)
            if bits is None or (rng.random() < 0.3 and m <= 8):
                emit(i, new_value(i), "new_value")
            else:
                emit(i, bits, "in_palette")
            if rng.random() < 0.4:  # the same flip again: back to a palette that exists
                emit(*done[int(rng.integers(0, len(done)))], "repeat")
        if target and m <= 8:
            reached.add("replan_kept")
    elif scenario in ("demote_palette", "column_then_values"):
        if scenario == "column_then_values":  # the compact offset rewritten (or the block wide) before the palette overflows
            emit(i0, column(i0, str(rng.choice(["inside", "inside", "below_base", "past_shift"]))), "column")
        need = 2 * (17 - min(m, 16)) + 2
        if need <= budget - 2:
            burst(i0, need)
            if target and scenario == "demote_palette":
                reached.add("demoted_by_palette")
        else:
            burst(i0, budget - 2)
    elif scenario == "demote_span":
        for _ in range(int(rng.integers(1, 4))):
            i = min(nnz - 1, i0 + int(rng.integers(0, 30)))
            emit(i, column(i, "past_65535"), "column")
        if target:
            reached.add("demoted_by_span")
    while len(flips) < budget and (scenario == "mixed" or rng.random() < 0.5):
        if scenario == "mixed" and rng.random() < 0.1:
            break
        i = place() if rng.random() < 0.4 else min(nnz - 1, i0 + int(rng.integers(0, 60)))
        what = rng.random()
        if what < 0.2 and in_palette(i) is not None:
            emit(i, in_palette(i), "in_palette")
        elif what < 0.4:
            emit(i, new_value(i), "new_value")
        elif what < 0.5 and done:
            emit(*done[int(rng.integers(0, len(done)))], "repeat")
        elif what < 0.85:
            emit(i, column(i, str(rng.choice(["inside", "past_shift", "below_base", "past_65535", "past_n"]))), "column")
        else:
            emit(i, new_value(i) + column(i, "inside" if rng.random() < 0.5 else "past_shift"), "value_and_column")
    return flips, reached


def sequence_flip(rng, cols, vb, i, n_in, done):
    """One flip of tools/fuzz_sequence.py's `inject` operation into element i of a mode-none CSR matrix with current
    columns `cols` and value patterns `vb` -> bits, of the classes of the packed family.  Value flips keep the value
    finite (another value from a few places away, a mantissa bit or the sign), so that the vectors of the sequence
    stay comparable bit for bit.  `done`: the (element, bits) made so far; one of them may come again."""
    what = rng.random()
    if what < 0.15 and done:  # the same flip again: back to a palette that exists
        return done[int(rng.integers(0, len(done)))]
    if what < 0.4:
        for j in rng.permutation(np.arange(max(0, i - 6), min(len(vb), i + 7))):
            bits = _bits_of(vb[i] ^ vb[j])
            if 0 < len(bits) <= 32 and np.isfinite(np.uint64(vb[j]).view(np.float64)):
                return i, bits
    value = [int(rng.choice([int(rng.integers(0, 52)), 63]))]
    if what < 0.6:
        return i, value
    column = [64 + int(rng.choice([int(rng.integers(0, 3)), int(rng.integers(10, 16)), max(0, int(cols[i]).bit_length() - 1),
                                   int(rng.integers(16, 18)), int(rng.integers(min(31, int(n_in).bit_length()), 32))]))]
    return i, (column if what < 0.9 else value + column)


def special_x(rng, n):
    x = rng.standard_normal(n)
    if n and rng.random() < 0.25:
        hit = rng.random(n) < 0.05
        sp = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 5e-324, -1e-310])
        x[hit] = sp[rng.integers(0, len(sp), size=int(hit.sum()))]
    return x


def packed_case(seed):
    """case `seed` of the packed family (its own seed space)"""
    rng = np.random.default_rng([0x9ACED, int(seed)])
    c = Case()
    c.seed = int(seed)
    other = rng.random() < 0.2  # the minority: another mode, or COO -- low-cardinality values are legal there, nothing packs
    c.fmt, c.mode = CSR, "none"
    if other:
        c.fmt = CSR if rng.random() < 0.5 else COO
        c.mode = str(rng.choice(MODES[1:] if c.fmt == CSR else MODES))
    c.layout = str(rng.choice(["stream", "auto"]))
    kind = str(rng.choice(["band"] * 11 + ["all"] * 4 + ["tiny"] * 2 + ["none_values"] * 2 + ["none_span"]))
    if c.fmt == COO and kind == "none_span":
        kind = "band"
    c.kind = kind
    key, n, spread = _structure(rng, kind)
    rows, cols = key // n, key % n
    nnz = len(key)
    focus_k = int(rng.integers(0, 5)) if kind in ("band", "all") else None
    vb, segs, fidx = _values(rng, kind, rows, nnz, focus_k)
    c.segs, c.spread = segs, spread
    # a shard: a row range of the matrix, its columns those of the whole (n_in = n)
    c.n, c.n_in, c.index_base, c.row0 = n, n, 0, 0
    shard = c.fmt == CSR and n >= 40 and rng.random() < 0.2
    if shard:
        r0 = int(rng.integers(0, n // 2))
        r1 = int(rng.integers(r0 + 1, n + 1))
        a, b = int(np.searchsorted(rows, r0)), int(np.searchsorted(rows, r1))
        rows, cols, vb = rows[a:b] - r0, cols[a:b], vb[a:b]
        segs = [(max(s0, a) - a, min(s1, b) - a, ms, off) for s0, s1, ms, off in segs]
        c.segs = segs
        c.n, c.index_base, c.row0, nnz = r1 - r0, a, r0, b - a
    c.cols, c.rows, c.vals = cols.astype(np.uint32), rows.astype(np.uint32), vb.view(np.float64).copy()
    c.rowptr = np.searchsorted(rows, np.arange(c.n + 1)).astype(np.int64)
    c.x = special_x(rng, c.n_in)
    c.mark = _window_rules(c.cols, vb, c.rowptr) if (c.fmt, c.mode) == (CSR, "none") else None

    # the model: a value segment of 3 tiles or more holds a whole block, which has the segment's m values; it packs
    # for certain if the band plus the 4 * 256 rows a block holds at the most fit the span its k leaves
    def k_of(ms):
        return int(np.ceil(np.log2(ms))) if ms > 1 else 0
    big = [(a, b, ms) for a, b, ms, _ in segs if b - a >= 3 * TILE and ms <= 16]
    sure = [s for s in big if spread is not None and spread + 1024 < (1 << (16 - k_of(s[2])))]
    c.classes, c.eligible = set(), set()
    none_csr = (c.fmt, c.mode) == (CSR, "none")
    c.flips, c.path, c.interior, c.spmm_k = [], "spmv", None, 0
    if none_csr:
        c.eligible.add("packed_at_creation")
        c.eligible.add("shard")
        if sure or (c.mark == "all" and nnz):
            c.classes.add("packed_at_creation")
        if kind in ("band", "all") and not shard and nnz >= 4 * TILE:  # (a shard may cut the focus segment short)
            c.eligible |= {"k0", "k1", "k2", "k3", "k4"}
        c.classes |= {"k%d" % k_of(s[2]) for s in big}
        target = None
        if sure:  # the focus segment if it packs, else any that does
            target = next((s for s in sure if fidx is not None and s[0] == segs[fidx][0]), sure[int(rng.integers(0, len(sure)))])
            c.eligible |= {"replan_kept", "demoted_by_palette", "demoted_by_span"}
        c.flips, reached = _plan_flips(rng, c, target)
        c.classes |= reached
        c.path = str(rng.choice(["spmv", "dot", "parts"]))
        c.eligible.add("inject_before_parts")
        if c.path == "parts":
            # the two parts are cut at row-block granularity (include/abft_hip.h: "whole row blocks of those rows"),
            # so which rows the interior part computes is not the caller's to know: every inject comes before the
            # interior part, never between the two
            lo = int(rng.integers(0, c.n + 1))
            c.interior = (lo, int(rng.integers(lo, c.n + 1)))
            if c.flips:
                c.classes.add("inject_before_parts")
        if shard:
            c.classes.add("shard")
    else:
        c.flips = [(i, b, "random") for i, b in random_flips(rng, c.fmt, c.mode, c.n, nnz)]
    # flips between two comparisons: few for the large cases (a comparison downloads the whole matrix)
    step = (1, 5) if nnz <= 200000 else (3, 7)
    c.checks, at = [], 0
    while at < len(c.flips):
        at = min(len(c.flips), at + int(rng.integers(*step)))
        c.checks.append(at)
    if c.fmt == CSR and c.layout == "stream" and not shard and c.n > 0:
        c.eligible.add("spmm")
        if rng.random() < 0.4:
            c.spmm_k = int(rng.integers(2, 9))
            c.classes.add("spmm")
    return c


# ------------------------------------------------- third family: CG-shaped call sequences --
# tools/fuzz_loop.py plays these.  A case is one context: one to three solves (a matrix, the loop's x r p w, the
# spares q s t u, the right-hand side b), a mode, and a flat script of calls.  The script's items:
#     ("spmv", s)  ("dot", s) | ("dot_copies", s)  ("calc_xr", s, how, v)  ("calc_p", s, how, v)
#         the four calls of an iteration of solve s.  how "q": the quotient of the scalars handed back, moved by v
#         ulps; how "c": the constant v.  dot_copies: p.w from dot(q, s) of copies q <- p, s <- w, no dot(p, w).
#     ("extra", s, kind, args, gap)
#         one more call on solve s's vectors in front of call number `gap` of its iteration (gap 0: between two
#         iterations).  LOOP_EXTRAS names the kinds; what each does, and to the model, is fuzz_loop.Player.extra.
# `tags` are computed from the script alone (loop_tags): what the script must reach whatever the library does.

LOOP_EXTRAS = ["download", "upload", "copy_in", "copy_out", "map_unmap", "view", "ptr", "dot", "dot_rr", "dot_pw",
               "spmv_other", "spmv_second", "calc_xr_again", "calc_p_other", "drain", "synchronize", "residual_gap",
               "block", "precond", "profile", "graph", "respare", "inject"]
LOOP_SCALES = [480, -480, -530]  # powers of two: r.r near 2^960 and 2^-960 (normal), r.r and p.w subnormal
LOOP_NAMED = ["one", "lap3", "diag23", "diag1", "arrow", "holes"]
LOOP_MAIN = ["spmv", "dot", "calc_xr", "calc_p"]
INJECT_MODES = ["none", "constraints", "sec7", "sec8", "secded"]  # (sed only detects: fatal)
# the seeds tests/test_gpu_fuzz.py plays, in blocks of LOOP_BLOCK per child process; tests/test_fuzz_generator.py holds the
# coverage conditions over exactly these
LOOP_SEEDS = range(1, 193)
LOOP_BLOCK = 48


class LoopCase:
    """seed, mode, solves [dict(spec, n, nnz, scale, rhs_seed)], script, iterations, tags (loop_tags)"""


def loop_matrix(spec):
    """-> (cols, rows, vals, n) of a solve's matrix spec"""
    from _matrices import matrix
    from _oracle import laplace5, random_spd
    if spec[0] == "laplace5":
        return laplace5(spec[1], spec[2])
    if spec[0] == "random_spd":
        return random_spd(spec[1], spec[2], seed=spec[3])
    return matrix(spec[1])


def _loop_spec(rng):
    what = rng.random()
    if what < 0.4:
        return ("laplace5", int(rng.integers(3, 41)), int(rng.integers(3, 41)))
    if what < 0.7:
        return ("random_spd", int(rng.choice([50, 300, 2000, 3001])), int(rng.integers(2, 12)), int(rng.integers(0, 1000)))
    return ("named", str(rng.choice(LOOP_NAMED)))


def _slow(spec):
    """CG on it neither converges to an exact zero nor leaves the normal range within 40 iterations from a right-hand
    side of scale 1 (Laplacians of 8 x 8 and more, the diagonally dominant random matrices, arrow, holes)"""
    if spec[0] == "laplace5":
        return min(spec[1], spec[2]) >= 8
    return spec[0] == "random_spd" or spec[1] in ("arrow", "holes")


def _order_flip(rng, cols, rowptr, n):
    """constraints mode: (element, [bit]) -- one column bit that lifts a column to or past its row successor's, inside
    the vector (the order check fails at that element at every SpMV from then on) -- or None"""
    nnz = len(cols)
    for _ in range(200):
        i = int(rng.integers(0, max(1, nnz - 1)))
        r = int(np.searchsorted(rowptr, i, side="right")) - 1
        if i + 1 >= int(rowptr[r + 1]):
            continue
        for b in rng.permutation(max(1, int(n).bit_length())):
            new = int(cols[i]) ^ (1 << int(b))
            if int(cols[i + 1]) <= new < n:
                return i, [64 + int(b)]
    return None


def loop_tags(c):
    """The structural tags of a case, from its script alone.
    clean iteration: the four calls of one solve as written -- quotients, no extra call, no call of another solve
    since the solve's previous iteration began -- on vectors only the library sees into (no pointer read so far, no
    capture so far), with no event due at its SpMV.  in_flight: (kind, gap) of every extra call that is the first
    disturbance behind two clean iterations of its solve.  must_commit: three clean iterations of one solve in a row
    whose scalars are sure to be normal numbers (`steady`: a matrix CG neither finishes nor overflows on within 40
    iterations; at 2^+-480 only the first six iterations of an undisturbed solve; never at 2^-530).  plain_loop: one
    solve, scale 1, no extra call -- the counters are those of the arming rule (tests/_ahead.py: expected)."""
    mode, S = c.mode, range(len(c.solves))
    run_s, run_len, run_steady = None, 0, 0
    open_it, pre_dirty = {}, {s: False for s in S}
    exposed, pristine = {s: False for s in S}, {s: True for s in S}
    pending, standing, count = {s: False for s in S}, {s: False for s in S}, {s: 0 for s in S}
    graph_seen = False
    tags = dict(must_commit=False, in_flight=[], switch_inside=False, event_every_spmv=False)

    def calm(s):
        return not (exposed[s] or graph_seen or standing[s])

    def steady(s):
        v = c.solves[s]
        if not _slow(v["spec"]):
            return False
        return v["scale"] == 0 or (abs(v["scale"]) == 480 and pristine[s] and count[s] < 6)

    for item in c.script:
        s = item[1]
        others = [t for t in open_it if t != s]
        if others:
            tags["switch_inside"] = True
            for t in open_it:
                open_it[t] = True
            run_len = run_steady = 0
        if item[0] == "extra":
            kind, args, gap = item[2], item[3], item[4]
            dirty = open_it[s] if s in open_it else pre_dirty[s]
            if run_s == s and run_len >= 2 and not others and not dirty and calm(s):
                tags["in_flight"].append((kind, gap))
            if s in open_it:
                open_it[s] = True
            else:
                pre_dirty[s] = True
            pristine[s] = False
            if kind == "ptr" and args[0] in "xrpw":
                exposed[s] = True
            if kind == "graph":
                graph_seen = True
            if kind == "inject" and mode != "none":
                pending[s] = True
                if mode == "constraints":
                    standing[s] = True
                    tags["event_every_spmv"] = True
            continue
        op = LOOP_MAIN.index("dot" if item[0] == "dot_copies" else item[0])
        if op == 0:
            if run_s != s:
                run_s, run_len, run_steady = s, 0, 0
            open_it[s] = bool(others) or pre_dirty[s] or not calm(s) or pending[s]
            if not steady(s):
                run_steady = 0
            pre_dirty[s] = False
            pending[s] = standing[s]
        if item[0] == "dot_copies" or (op >= 2 and (item[2], item[3]) != ("q", 0)):
            open_it[s] = True
        if op == 3:
            if open_it.pop(s):
                run_len = run_steady = 0
                pristine[s] = False
            else:
                run_len += 1
                run_steady += 1
                if run_steady >= 3:
                    tags["must_commit"] = True
            count[s] += 1
    lengths = [v["n"] for v in c.solves]
    tags["three_lengths"] = len(set(lengths)) == 3
    tags["same_length_pair"] = len(lengths) == 2 and lengths[0] == lengths[1]
    tags["scaled"] = sorted(set(v["scale"] for v in c.solves if v["scale"]))
    tags["plain_loop"] = len(c.solves) == 1 and not tags["scaled"] and not any(i[0] == "extra" for i in c.script)
    tags["in_flight"] = sorted(set(tags["in_flight"]))
    return tags


def loop_case(seed):
    """case `seed` of the CG-loop family (its own seed space)"""
    rng = np.random.default_rng([0xC6100, int(seed)])
    c = LoopCase()
    c.seed = int(seed)
    c.mode = str(rng.choice(MODES))
    # three extra calls the case is built around: the (kind, gap) pairs come round with the seeds
    npairs = 4 * len(LOOP_EXTRAS)
    focus = [divmod((3 * int(seed) + 31 * j) % npairs, 4) for j in range(3)]  # (31: three kinds far apart)
    focus = [(LOOP_EXTRAS[k], g) for k, g in focus]
    plain = int(seed) % 12 == 0  # one solve, scale 1, scalars perturbed, no extra call
    if plain:
        focus = []
    if c.mode == "sed" and any(k == "inject" for k, _ in focus):
        c.mode = "secded"
    # the solves: one; two of equal length; two of different lengths; three of different lengths
    pattern = "one" if plain else str(rng.choice(["one"] * 9 + ["equal"] * 3 + ["two"] * 4 + ["three"] * 4))
    specs = [_loop_spec(rng)]
    if pattern == "equal":
        a = specs[0]
        twin = {"diag1": "diag23", "diag23": "diag1"}
        specs.append(("laplace5", a[2], a[1]) if a[0] == "laplace5" and rng.random() < 0.5 else
                     ("named", twin[a[1]]) if a[0] == "named" and a[1] in twin else a)
    while len(specs) < {"one": 1, "equal": 2, "two": 2, "three": 3}[pattern]:
        b = _loop_spec(rng)
        if all(loop_matrix(b)[3] != loop_matrix(a)[3] for a in specs):
            specs.append(b)
    scale = 0 if rng.random() < 0.7 or plain else int(rng.choice(LOOP_SCALES))
    c.solves, mats = [], []
    for spec in specs:
        cols, rows, vals, n = loop_matrix(spec)
        mats.append(dict(cols=cols.astype(np.int64), vb=vals.view(np.uint64).copy(), n=n, done=[], used=set(),
                         rowptr=np.searchsorted(rows, np.arange(n + 1)), standing=False))
        c.solves.append(dict(spec=spec, n=int(n), nnz=int(len(vals)), scale=scale if rng.random() < 0.8 else 0,
                             rhs_seed=int(rng.integers(0, 1 << 30))))
    ns = len(c.solves)

    def extra(s, kind, gap):
        """-> the script item (an inject that cannot be made becomes a drain)"""
        m, pick = mats[s], lambda names: str(rng.choice(list(names)))
        args = ()
        if kind in ("download", "map_unmap", "view"):
            args = (pick("xrpwqs"),)
        elif kind == "upload":
            args = (pick("xrpwq"), int(rng.integers(0, 1 << 30)))
        elif kind == "copy_in":
            args = (pick("xrpw"), pick("qs"))
        elif kind == "copy_out":
            args = (pick("qs"), pick("xrpw"))
        elif kind == "ptr":
            args = (pick("qstub") if rng.random() < 0.7 else pick("xrpw"),)
        elif kind == "dot":
            args = (pick("xrpwqs"), pick("xrpwqs"))
        elif kind == "spmv_other":
            args = [("q", "s"), ("r", "s"), ("p", "s"), ("x", "u"), ("q", "w"), ("w", "t")][int(rng.integers(0, 6))]
        elif kind == "spmv_second":
            args = (pick(["coo", "sweep", "panels"]), pick("pq"), "s")
        elif kind == "calc_p_other":
            args = (("q", "r") if rng.random() < 0.5 else ("p", "q")) + (float(rng.choice([0.5, -0.25, 0.0, 1.0])),)
        elif kind == "block":
            args = (int(rng.integers(2, 5)), int(rng.integers(0, 1 << 30)))
        elif kind == "precond":
            args = (float(rng.choice([0.37, -0.5, 0.0])), float(rng.choice([0.61, 1.0, 0.0])))
        elif kind == "respare":
            args = (int(rng.integers(0, 1 << 30)),)
        elif kind == "inject":
            flip = None
            if c.mode == "none":
                i = int(rng.integers(0, len(m["vb"])))
                i, bits = sequence_flip(rng, m["cols"], m["vb"], i, m["n"], m["done"])
                for b in bits:
                    if b < 64:
                        m["vb"][i] ^= np.uint64(1) << np.uint64(b)
                    else:
                        m["cols"][i] ^= 1 << (b - 64)
                m["done"].append((i, bits))
                flip = (int(i), [int(b) for b in bits])
            elif c.mode == "constraints":
                if not m["standing"]:  # one violation per matrix: it stays
                    flip = _order_flip(rng, m["cols"], m["rowptr"], m["n"])
                    m["standing"] = flip is not None
            elif c.mode in INJECT_MODES:
                i = int(rng.integers(0, len(m["vb"])))
                if i not in m["used"]:  # a second flip in one codeword would be a double-bit error
                    m["used"].add(i)
                    flip = (i, [int(rng.integers(0, NBITS[CSR]))])
            if flip is None:
                kind = "drain"
            else:
                args = (flip[0], tuple(flip[1]))
        return ("extra", s, kind, tuple(args), gap)

    def iteration(s, what=None, plant=None):
        """the items of one iteration of solve s -> [[items before and with call 0], ..., [... call 3]]"""
        what = what if what is not None else str(rng.choice(["clean"] * 12 + ["alpha_ulp", "beta_ulp", "alpha_const",
                                                                              "beta_const", "nodot"] + ([] if plain else ["extras"] * 3)))
        calls = [[("spmv", s)], [("dot", s)], [("calc_xr", s, "q", 0)], [("calc_p", s, "q", 0)]]
        if what == "alpha_ulp":
            calls[2] = [("calc_xr", s, "q", int(rng.choice([-1, 1])))]
        elif what == "beta_ulp":
            calls[3] = [("calc_p", s, "q", int(rng.choice([-1, 1])))]
        elif what == "alpha_const":
            calls[2] = [("calc_xr", s, "c", float(rng.choice([0.0, 0.37, -0.5])))]
        elif what == "beta_const":
            calls[3] = [("calc_p", s, "c", float(rng.choice([0.0, 0.61, 1.0])))]
        elif what == "nodot":
            calls[1] = [("dot_copies", s)]
        elif what == "extras":
            for _ in range(int(rng.integers(1, 4))):
                g = int(rng.integers(0, 4))
                kind = str(rng.choice(LOOP_EXTRAS))
                if kind == "graph" and rng.random() < 0.7:  # (the first capture ends x-in-SpMV for the context)
                    kind = "synchronize"
                calls[g].insert(len(calls[g]) - 1, extra(s, kind, g))
        if plant:
            calls[plant[1]].insert(0, extra(s, plant[0], plant[1]))
        return calls

    # stretches of whole iterations of one solve, the solves taking turns; two of them end in a planted extra call
    # behind two clean iterations, some are three clean iterations, some interleave two solves inside an iteration
    kinds = ["plant%d" % j for j in range(len(focus))] + (["commit"] if rng.random() < 0.6 else []) + \
            ["free"] * int(rng.integers(1 if plain else 0, 5))
    if ns > 1:
        kinds += ["inside"] * int(rng.integers(0, 3))
    kinds = [kinds[i] for i in rng.permutation(len(kinds))]
    last = [k for k in kinds if k.startswith("plant") and focus[int(k[-1])][0] == "graph"]  # (nothing is in flight behind it)
    kinds = [k for k in kinds if k not in last] + last
    c.script, total, s = [], 0, int(rng.integers(0, ns))
    if c.mode == "constraints" and not plain and rng.random() < 0.5:  # a violation that stands from the start
        c.script.append(extra(s, "inject", 0))
    for kind in kinds:
        s = (s + int(rng.integers(1, ns))) % ns if ns > 1 else 0
        if kind.startswith("plant"):
            its = [iteration(s, "clean"), iteration(s, "clean"), iteration(s, "clean", focus[int(kind[-1])])]
        elif kind == "commit":
            its = [iteration(s, "clean") for _ in range(3)]
        elif kind == "inside":
            # solve s up to call g, then solve t: whole iterations, or up to its call h, s's rest, t's rest
            t, g = (s + int(rng.integers(1, ns))) % ns, int(rng.integers(1, 4))
            a = iteration(s)
            if rng.random() < 0.5:
                inner = [x for _ in range(int(rng.integers(1, 3))) for call in iteration(t) for x in call]
                flat = [x for call in a[:g] for x in call] + inner + [x for call in a[g:] for x in call]
                total += 1 + sum(1 for x in inner if x[0] == "spmv")
            else:
                b, h = iteration(t), int(rng.integers(1, 4))
                flat = [x for call in a[:g] for x in call] + [x for call in b[:h] for x in call] + \
                       [x for call in a[g:] for x in call] + [x for call in b[h:] for x in call]
                total += 2
            c.script += flat
            continue
        else:
            its = [iteration(s) for _ in range(int(rng.integers(1, 7)))]
        if total + len(its) > 40:
            continue
        total += len(its)
        c.script += [x for it in its for call in it for x in call]
    while total < 10:
        c.script += [x for call in iteration(s) for x in call]
        total += 1
    c.iterations = total
    c.tags = loop_tags(c)
    return c
