"""The walk of the protected vector kernels (abft_sparse_cg_amd/csrc/vecc_walk.h) without a GPU: tests/host/
vecc_walk_play.cpp compiles the header and ecc_device.h -- the text the kernels compile -- for the host, with
AddressSanitizer and UBSan, and runs every operation at VEC 1 and 2 over the chains of two toy grids.  The expectation
is formed here with the model of tests/_vecc.py (written from DESIGN.md section 5e, not from the device code): an
undamaged call on the repaired inputs.  Everything is compared bit for bit."""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import _vecc as V

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "abft_sparse_cg_amd", "csrc")
U = np.uint64
ALPHA, BETA = 0.37251, -1.59375
LENGTHS = [0, 1, 2, 3, 5, 6, 7, 13]
GRIDS = [(3, 1), (2, 2)]  # (threads in a block, blocks)
# operation -> (operands in the order of its struct, the ones it reads, the read-only one whose repair is stored back,
# its sums)
OPS = {
    "dot": ("ab", "ab", "", 1), "xr": ("xrpw", "xrpw", "", 1), "p": ("pr", "pr", "", 0), "r": ("rw", "rw", "", 1),
    "r_precond": ("rwd", "rwd", "d", 2), "px_precond": ("xprd", "xprd", "d", 0), "scrub": ("v", "v", "v", 0),
}
WRITTEN = {"dot": "", "xr": "xr", "p": "p", "r": "r", "r_precond": "r", "px_precond": "xp", "scrub": ""}
# the ordinals handed in: not 0, 1, 2, ... so that a mixed-up operand shows
ORD = {name: 3 + 2 * k for k, name in enumerate("abxrpwdv")}


def model(op, W):
    """one undamaged call on the repaired inputs -> (the operands' words after it, the terms of its sums per element)"""
    names, read, back, _ = OPS[op]
    rep = {k: V.decode(W[k])[0] for k in read}
    v = {k: V.strip(rep[k]) for k in read}
    out = {k: W[k].copy() for k in names}
    terms = []
    with np.errstate(all="ignore"):
        if op == "dot":
            terms = [v["a"] * v["b"]]
        if op in ("xr", "px_precond"):
            out["x"] = V.encode(v["x"] + ALPHA * v["p"])
        if op in ("xr", "r", "r_precond"):
            out["r"] = V.encode(v["r"] - ALPHA * v["w"])
            rs = V.strip(out["r"])
            terms = [rs * (v["d"] * rs), rs * rs] if op == "r_precond" else [rs * rs]
        if op == "p":
            out["p"] = V.encode(v["r"] + BETA * v["p"])
        if op == "px_precond":
            out["p"] = V.encode(v["d"] * v["r"] + BETA * v["p"])
    for k in back:  # one flipped bit: stored back repaired; two: the word stays
        out[k] = np.where(V.decode(W[k])[1] == 1, rep[k], W[k])
    return out, terms


def chains(vec, n, threads, blocks):
    """per chain of the grid, in thread order: its steps, each the list of its element indices"""
    out = []
    for t in range(threads * blocks):
        steps, i = [], t * vec
        while i < n:
            steps.append([i, i + 1] if vec == 2 and i + 1 < n else [i])
            i += threads * blocks * vec
        out.append(steps)
    return out


def plans(op, vec, n, threads, blocks):
    """[(category, [(operand, element, [bits])])]: the flips of one case each"""
    read = OPS[op][1]
    ch = chains(vec, n, threads, blocks)
    long_ = max(ch, key=len) if ch else []
    out = [("none", [])]
    if not long_:
        return out
    first, tail = long_[0][0], n - 1
    for k in read:
        out.append(("first_step", [(k, first, [30])]))
        if len(long_) >= 3:
            out.append(("middle_step", [(k, long_[len(long_) // 2][-1], [41])]))
        out.append(("tail_element", [(k, tail, [63])]))
        out.append(("double", [(k, first, [9, 33])]))
        if k in OPS[op][2]:
            out.append(("double_dinv_tail", [(k, tail, [0, 7])]))
    pair = next((s for c in ch for s in c if len(s) == 2), None)
    if pair:
        out.append(("both_words_of_a_pair", [(read[0], pair[0], [12]), (read[0], pair[1], [50])]))
        out.append(("pair_first_word_only", [(read[-1], pair[0], [8])]))
        out.append(("pair_second_word_only", [(read[-1], pair[1], [62])]))
    if vec == 2 and n % 2:
        out.append(("odd_tail_under_vec2", [(read[0], tail, [21])]))
    if len(read) >= 2:
        out.append(("two_operands_one_step", [(read[0], first, [17]), (read[1], first, [55])]))
        out.append(("every_operand_one_element", [(k, first, [10 + j]) for j, k in enumerate(read)]))
    if len(long_) >= 2:
        out.append(("two_steps_one_chain", [(read[0], long_[0][0], [25]), (read[-1], long_[1][-1], [44])]))
    if len(long_) >= 3:  # the step between them was carried out by the first walk
        out.append(("carried_out_between", [(read[0], long_[0][0], [26]), (read[-1], long_[2][0], [45])]))
    for name, bit in (("code_bit", 3), ("bit_0", 0), ("data_bit", 40)):
        out.append((name, [(read[0], first, [bit])]))
        out.append((name, [(read[-1], tail, [bit])]))
    return out


def build_cases():
    cases = []
    for op in OPS:
        for vec in (1, 2):
            for n in LENGTHS:
                for threads, blocks in GRIDS:
                    for cat, flips in plans(op, vec, n, threads, blocks):
                        rng = np.random.default_rng(len(cases))
                        W = {k: V.encode(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)) for k in OPS[op][0]}
                        for k, i, bits in flips:
                            for b in bits:
                                W[k][i] ^= U(1 << b)
                        cases.append(dict(op=op, vec=vec, n=n, threads=threads, blocks=blocks, cat=cat, flips=flips, W=W))
    return cases


def bits_of(x):
    return "%016x" % int(np.float64(x).view(U))


@pytest.fixture(scope="module")
def played(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vecc_walk") / "vecc_walk_play")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-I", CSRC, os.path.join(HERE, "host", "vecc_walk_play.cpp"), "-o", exe], check=True)
    cases = build_cases()
    text = []
    for c in cases:
        text.append("%s %d %d %d %d 2 %s %s" % (c["op"], c["vec"], c["n"], c["threads"], c["blocks"], bits_of(ALPHA), bits_of(BETA)))
        for k in OPS[c["op"]][0]:
            text.append("%d %s" % (ORD[k], " ".join("%016x" % int(w) for w in c["W"][k])))
    # (the leak check at exit needs ptrace rights a sandbox may withhold; the program frees through destructors)
    p = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0, p.stderr[-3000:]
    got, run = [], None
    for line in p.stdout.splitlines():
        w = line.split()
        if w[0] == "case":
            got.append([])
        elif w[0] == "run":
            run = dict(v={}, s=[], e=[], c=None)
            got[-1].append(run)
        elif w[0] == "v":
            run["v"][int(w[1])] = np.array([int(t, 16) for t in w[2:]], dtype=U)
        elif w[0] == "s":
            run["s"].append(w[2:])
        elif w[0] == "e":
            run["e"].append(tuple(int(t) for t in w[1:]))
        else:
            run["c"] = int(w[1])
    assert len(got) == len(cases)
    return cases, got


def expect(c, W):
    """-> (the words after one call on W, the sums of every chain as hex bits, the events, sorted)"""
    names, read, _, nsums = OPS[c["op"]]
    out, terms = model(c["op"], W)
    sums = []
    for steps in chains(c["vec"], c["n"], c["threads"], c["blocks"]):
        at = [i for s in steps for i in s]
        sums.append([bits_of(V.serial_sum(t[at])) for t in terms[:nsums]])
    events = []
    for k in read:
        _, status, bit = V.decode(W[k])
        events += [(1 if status[i] == 1 else -1, int(i), int(bit[i]) if status[i] == 1 else 0, ORD[k])
                   for i in np.flatnonzero(status)]
    return out, sums, sorted(events)


def test_every_case_leaves_what_an_undamaged_call_on_the_repaired_inputs_leaves(played):
    cases, got = played
    for c, runs in zip(cases, got):
        tag = (c["op"], c["vec"], c["n"], c["threads"], c["blocks"], c["cat"])
        names, read, back, _ = OPS[c["op"]]
        W = c["W"]
        assert len(runs) == 2
        for r, run in enumerate(runs):
            out, sums, events = expect(c, W)
            for j, k in enumerate(names):
                assert np.array_equal(run["v"][j], out[k]), (tag, r, k)
            assert run["s"] == sums, (tag, r)
            assert sorted(run["e"]) == events, (tag, r)
            assert run["c"] == len(events), (tag, r)  # one cold decode per failing word, none on a clean run
            W = out


def test_read_only_operands_keep_every_bit_and_the_events_are_the_planted_flips(played):
    cases, got = played
    for c, runs in zip(cases, got):
        tag = (c["op"], c["vec"], c["n"], c["cat"])
        names, read, back, _ = OPS[c["op"]]
        written = WRITTEN[c["op"]]
        planted = sorted((-1 if len(bits) == 2 else 1, i, 0 if len(bits) == 2 else bits[0], ORD[k]) for k, i, bits in c["flips"])
        assert sorted(runs[0]["e"]) == planted, tag
        for j, k in enumerate(names):
            if k in read and k not in written and k not in back:
                assert np.array_equal(runs[0]["v"][j], c["W"][k]), (tag, k)
        for k, i, bits in c["flips"]:
            j = names.index(k)
            if len(bits) == 2 and (k in back or k not in written):  # two flips: the word as it is, never written back
                assert runs[1]["v"][j][i] == c["W"][k][i], (tag, k)
            if len(bits) == 1 and k in back:  # stored back once, gone on the second run of the same call
                assert runs[0]["v"][j][i] == c["W"][k][i] ^ U(1 << bits[0]), (tag, k)
                assert not [e for e in runs[1]["e"] if e[3] == ORD[k]], (tag, k)
        if not c["flips"]:
            assert runs[0]["e"] == [] and runs[0]["c"] == 0, tag


def test_every_category_was_reached(played):
    cases, _ = played
    seen = Counter((c["op"], c["vec"], c["cat"]) for c in cases)
    cats = {"none", "first_step", "middle_step", "tail_element", "double", "two_steps_one_chain", "carried_out_between",
            "code_bit", "bit_0", "data_bit"}
    for op in OPS:
        many = len(OPS[op][1]) >= 2
        for vec in (1, 2):
            want = set(cats) | ({"two_operands_one_step", "every_operand_one_element"} if many else set())
            want |= {"both_words_of_a_pair", "pair_first_word_only", "pair_second_word_only", "odd_tail_under_vec2"} if vec == 2 else set()
            want |= {"double_dinv_tail"} if OPS[op][2] else set()
            missing = [cat for cat in want if not seen[op, vec, cat]]
            assert not missing, (op, vec, missing)
    # chains of 0, 1 and several steps, and a last pair that is a single
    lengths = {len(s) for c in cases for s in chains(c["vec"], c["n"], c["threads"], c["blocks"])}
    assert {0, 1, 2, 3} <= lengths
    assert any(len(s[-1]) == 1 and len(s) > 1 for c in cases if c["vec"] == 2
               for s in chains(c["vec"], c["n"], c["threads"], c["blocks"]) if s)
    print("%d cases, %d operations x 2 walks, %d categories" % (len(cases), len(OPS), len({c["cat"] for c in cases})))
    assert len(cases) == sum(seen.values()) and len(cases) > 2000
