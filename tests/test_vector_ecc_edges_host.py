"""The inputs of tests/test_gpu_vector_ecc_edges.py and the numpy model on them, without a GPU: a failure
there must not be able to come from the fixture.  The crafted elements give the stored values the table
states, the operand families hold the classes they name, the flip lists reach every way the vector kernels
walk n = 4099, the arrow matrices are what the hub-column test needs, and the model's serial sum is too far
from the exact one at 133121 elements to serve as the reference of a tree sum."""
from fractions import Fraction

import numpy as np

import _ieee as I
import _vecc

U = np.uint64


def same_value(got_word, want):
    """the stored word is the codeword of `want` (any NaN codeword for a NaN)"""
    got = _vecc.strip(np.array([got_word], U))[0]
    if want != want:
        return bool(np.isnan(got)) and _vecc.decode(np.array([got_word], U))[1][0] == 0
    return int(got_word) == int(_vecc.encode(np.array([want]))[0])


def test_crafted_rows_give_the_stated_stored_values():
    for x, p, alpha, want, what in _vecc.CRAFTED:
        ops = np.array([x, p, -p])
        assert np.array_equal(_vecc.strip(_vecc.encode(ops)).view(U), ops.view(U)), what  # codeword values
        xw, pw, ww = (_vecc.encode(np.array([v])) for v in (x, p, -p))
        xs, rs, rr = _vecc.calc_xr(xw, xw, pw, ww, alpha)  # x += alpha p and r -= alpha (-p)
        assert same_value(xs[0], want) and same_value(rs[0], want), (what, hex(int(xs[0])), hex(int(rs[0])))
        assert same_value(_vecc.calc_p(pw, xw, alpha)[0], want), what  # p' = r + beta p
    # the overflow row by its bits, and the sign of the truncated zero
    stored = {what: _vecc.calc_xr(*(_vecc.encode(np.array([v])) for v in (x, x, p, -p)), alpha)[0][0]
              for x, p, alpha, _, what in _vecc.CRAFTED}
    assert int(stored["overflow"]) == 0x7FF000000000007F
    assert int(stored["the sign of a truncated zero"]) == int(_vecc.encode(np.array([-0.0]))[0])
    assert int(stored["the sign of a truncated zero"]) & ~0x7F == 1 << 63
    assert int(stored["a subnormal below the cut"]) == 0 and int(stored["exact cancellation"]) == 0
    # what the wrong kernels of the table would store is something else
    a = Fraction(1.0 + 2.0 ** -30)
    assert 1.0 + 2.0 ** -46 != 1.0 and a * a - Fraction(1.0 + 2.0 ** -29) == Fraction(2.0 ** -60)  # an FMA's result


def test_crafted_calls_place_every_row():
    for n in _vecc.EDGE_LENGTHS:
        calls = _vecc.crafted_calls(n)
        placed = [row for _, rows in calls for row in rows.values()]
        assert sorted(placed, key=str) == sorted(_vecc.CRAFTED, key=str), n
        for alpha, rows in calls:
            assert set(rows) <= set(_vecc.crafted_positions(n)) and all(r[2] == alpha for r in rows.values())
    assert _vecc.crafted_positions(1) == [0] and _vecc.crafted_positions(2) == [0, 1]
    assert _vecc.crafted_positions(3) == [0, 1, 2] and _vecc.crafted_positions(4099) == [0, 1, 4097, 4098]


def test_families_hold_the_classes_they_name():
    for n in (255, 257, 4099):
        for seed in range(4):  # the four operands of a call of the GPU test
            cls = {name: {I.value_class(v) for v in _vecc.strip(_vecc.family(name, n, _vecc.operand_seed(n, seed)))}
                   for name in _vecc.FAMILIES}
            assert cls["finite"] == {"finite"} and cls["huge"] == {"finite"}, (n, seed)
            assert cls["inf"] == {"finite", "+inf", "-inf"}, (n, seed)
            assert cls["nan"] == {"finite", "+inf", "-inf", "nan"}, (n, seed)
            v = _vecc.strip(_vecc.family("finite", n, _vecc.operand_seed(n, seed)))
            assert np.abs(v).max() < 1e201 and (v == 0).any() and (np.signbit(v) & (v == 0)).any()
            v = _vecc.strip(_vecc.family("huge", n, _vecc.operand_seed(n, seed)))
            assert (v >= 2.0 ** 1023).any() and (v <= -2.0 ** 1023).any() and not (v.view(U) & U(0x7F)).any()
    for name in _vecc.FAMILIES:  # operands are codewords
        w = _vecc.family(name, 4099, 1)
        assert not _vecc.decode(w)[1].any()
    assert int(np.array([_vecc.HUGE]).view(U)[0]) & 0x7F == 0 and _vecc.HUGE == float.fromhex("0x1.fffffffffff80p+1023")


def test_nan_with_its_payload_in_the_cut_bits_stays_a_nan():
    w = _vecc.encode(np.array([0x7FF0000000000041], U).view(np.float64))
    assert np.isnan(_vecc.strip(w))[0] and _vecc.decode(w)[1][0] == 0
    assert int(w[0]) & ~0x7F == 0x7FF8000000000000


def test_flip_lists_reach_every_walk_class():
    n = _vecc.FLIP_N
    assert I.reduce_blocks(n) == 3
    sweep, walk = [i for i, _ in _vecc.SWEEP], [i for i, _ in _vecc.WALK]
    assert len(set(sweep)) == 64 and max(sweep) < n and min(sweep) >= 0
    assert sorted(b for _, b in _vecc.SWEEP) == list(range(64))
    bits = [b for _, b in _vecc.WALK]
    assert len(set(walk)) == len(walk) and len(set(bits)) == len(bits) and max(walk) < n
    assert {0, 63} <= set(bits) and set(bits) & set(range(1, 7))
    for vec, rounds in ((2, 3), (1, 6)):
        cls = [_vecc.walk_class(i, n, vec) for i in walk]
        assert {c[2] for c in cls} >= {0, 1, 2}, vec
        # three rounds of ONE thread (0, 1, 2 in pairs; 0, 2, 4 element by element): several noted steps in a chain
        assert {c[2] for c in cls if c[1] == 0} == ({0, 1, 2} if vec == 2 else {0, 2, 4}), vec
        assert {c[0] for c in cls} | {_vecc.walk_class(i, n, vec)[0] for i in sweep} == {0, 1, 2}, vec
        assert {_vecc.walk_class(i, n, vec)[0] for i in sweep} == {0, 1, 2}, vec
        assert max(_vecc.walk_class(i, n, vec)[2] for i in range(n)) == rounds - 1, vec
        if vec == 2:
            assert {c[3] for c in cls} == {"first", "second", "single"}
            # both elements of one pair, and the odd tail is the last element alone
            assert cls[walk.index(0)][:3] == cls[walk.index(1)][:3] and cls[walk.index(4096)][:3] == cls[walk.index(4097)][:3]
            assert [i for i in range(n) if _vecc.walk_class(i, n, 2)[3] == "single"] == [4098]
        else:
            assert {c[3] for c in cls} == {"single"}
    # the double flips of the GPU test sit in a pair, not in the tail
    assert _vecc.walk_class(1537, n, 2)[3] == "second"
    # A5: 66 workgroups, i.e. ticket groups of 32, 32 and 2, with threads that took the cold path in two of them
    assert I.reduce_blocks(_vecc.MANY_N) == 66 and I.config_value("ABFT_TICKET_GROUP") == 32
    groups = {_vecc.walk_class(i, _vecc.MANY_N, vec)[0] // 32 for i, _ in _vecc.MANY_FLIPS for vec in (1, 2)}
    assert [i for i, _ in _vecc.MANY_FLIPS] == [0, 65535, 65536, _vecc.MANY_N - 1] and groups == {0, 1}


def test_arrow_builders():
    cap = _vecc.event_cap()
    assert cap == 65536
    n = cap + 64
    for dense in (1, 2):
        cols, rows, vals, m = _vecc.arrow(n, dense)
        assert m == n and np.all(np.diff(rows.astype(np.int64)) >= 0)
        key = rows.astype(np.int64) * n + cols
        assert np.all(np.diff(key) > 0)  # rows sorted, columns ascending inside a row, no duplicates
        for c in range(dense):
            assert np.count_nonzero(cols == c) > cap
        assert np.count_nonzero(cols == dense) == 1 and np.bincount(rows, minlength=n).max() == 1 + dense
    cols, rows, vals, m = _vecc.arrow_spd(n)
    key = rows.astype(np.int64) * n + cols
    assert np.all(np.diff(key) > 0) and np.count_nonzero(cols == 0) > cap and np.count_nonzero(rows == 0) == n
    a = dict(zip(key.tolist(), vals.tolist()))
    assert all(a[c * n + r] == v for r, c, v in zip(rows.tolist(), cols.tolist(), vals.tolist()))  # symmetric
    diag = vals[rows == cols]
    off = np.bincount(rows, weights=np.abs(vals), minlength=n) - np.abs(diag)
    assert len(diag) == n and np.all(diag > off)  # strictly diagonally dominant, positive diagonal: SPD


def test_model_spmv_on_the_arrow_repairs_a_flip_in_the_hub_entry():
    cols, rows, vals, n = _vecc.arrow(_vecc.event_cap() + 64)
    A = _vecc.csr_of(cols, rows, vals, n)
    xw = _vecc.encode(np.random.default_rng(1).standard_normal(n))
    y0, pw0 = _vecc.spmv(*A, xw)
    hit = xw.copy()
    hit[0] ^= U(1 << 30)
    y1, pw1 = _vecc.spmv(*A, hit)
    assert np.array_equal(y0, y1) and np.float64(pw0).view(U) == np.float64(pw1).view(U)
    assert not _vecc.decode(y0)[1].any()


def test_serial_sum_is_no_reference_at_many_workgroups():
    """|serial - exact| stays below the tree's bound, but is of its size: against the serial sum a correct tree
    sum could be off by the bound plus this -- hence the exact sum in the many-workgroups test"""
    n = _vecc.MANY_N
    rng = np.random.default_rng(n)
    r = _vecc.strip(_vecc.encode(rng.standard_normal(n)))
    terms = r * r
    bound = I.sum_bound(terms, I.dot_depth(n))
    gap = abs(_vecc.serial_sum(terms) - I.exact_sum(terms))
    print("serial - exact: %.3e, bound %.3e" % (gap, bound))
    assert gap < bound
    assert gap > 0.01 * bound
