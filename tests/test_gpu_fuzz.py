"""A short run of the randomised parity campaign (tools/fuzz_parity.py): random matrices,
formats, ABFT modes, layouts (streaming / forced panels), SpMV in one or two parts, single
and double bit flips -- stored words, y (bit for bit, two passes) and event streams against
the CPU oracle.  The long form (`python tools/fuzz_parity.py 300`: ~20 000 cases) is run by
hand; its last result is quoted in DESIGN.md.  The same for its packed family, for the
call-sequence campaign, without and with injects, and for the CG-loop campaign (tools/fuzz_loop.py)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_gen  # noqa: E402  (numpy only: the seeds of the CG-loop campaign and their blocks)


def test_short_fuzz_campaign():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_parity.py"), "20", "100000"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-1000:]
    assert "0 failures" in p.stdout


def test_short_call_sequence_campaign():
    """tools/fuzz_sequence.py: random interleavings of spmv / dot / calc_xr / calc_p / copy /
    map / unmap against a numpy model -- the fused dot and the deferred x update must never
    show (vectors bit-identical whenever read)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_sequence.py"), "15", "500000"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-1000:]
    assert " 0 failures" in p.stdout


def test_short_call_sequence_campaign_with_injects():
    """The same with ABFT_FUZZ_SEQ_INJECT=1: in mode none an `inject` operation flips bits of an element
    between the other calls (in a packed block that re-plans the block); the fused dot, the deferred x
    update and the device-scalar iteration must hold across it."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_sequence.py"), "15", "700000"],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, ABFT_FUZZ_SEQ_INJECT="1"))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-1000:]
    assert " 0 failures" in p.stdout
    assert int(re.search(r"injects: (\d+)", p.stdout).group(1)) > 100, p.stdout[-500:]


def test_short_packed_family_campaign():
    """tools/fuzz_parity.py with ABFT_FUZZ_FAMILY=packed: matrices whose row blocks pack, spans around
    every threshold of the planner, shards, up to 40 flips that re-plan blocks, the block SpMV.  A
    campaign that stops reaching one of the classes its summary counts is a failure too, and so is
    one that skips a mode-none case, or more than half of the others (a fatal event ends a case: the
    reference stops there; tests/test_fuzz_generator.py measures that share from the oracle alone)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_parity.py"), "20", "100000"],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, ABFT_FUZZ_FAMILY="packed"))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-1000:]
    assert " 0 failures" in p.stdout
    reached = dict(re.findall(r"(\w+)=(\d+)", re.search(r"^reached: (.*)$", p.stdout, re.M).group(1)))
    assert set(reached) == {"packed_at_creation", "k0", "k1", "k2", "k3", "k4", "replan_kept", "demoted_by_palette",
                            "demoted_by_span", "inject_before_parts", "shard", "spmm"}
    assert all(int(v) > 0 for v in reached.values()), reached
    skipped, others = (int(v) for v in re.search(r"skipped after a fatal event: (\d+) of the (\d+) cases in other modes",
                                                 p.stdout).groups())
    assert "none of the" in p.stdout and others > 0 and 2 * skipped <= others, p.stdout[-500:]


@pytest.mark.parametrize("block", range(len(fuzz_gen.LOOP_SEEDS) // fuzz_gen.LOOP_BLOCK))
def test_short_loop_campaign(block):
    """tools/fuzz_loop.py on one block of the seeds whose coverage tests/test_fuzz_generator.py holds on the CPU: CG-shaped
    call sequences (alpha and beta the quotients of the scalars handed back, so that the run-ahead, the speculation and
    x-in-SpMV arm) with perturbed scalars, extra calls in every gap, several solves taking turns, injects and scaled
    right-hand sides, against a numpy model and across the six settings of the switches.  A block that never drops a
    run-ahead in flight (levels 1 and 2), never flushes a pending x update or never drops a speculation fails, and so
    does one whose counters stay zero where the switch is on."""
    first = fuzz_gen.LOOP_SEEDS[0] + block * fuzz_gen.LOOP_BLOCK
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_loop.py"), str(first), str(fuzz_gen.LOOP_BLOCK)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-1000:]
    assert "fuzz_loop: %d cases, 0 failures" % fuzz_gen.LOOP_BLOCK in p.stdout
    reached = dict(re.findall(r"(\w+)=(\d+)", re.search(r"^reached: (.*)$", p.stdout, re.M).group(1)))
    assert set(reached) == {"dropped_level1", "dropped_level2", "flushed", "spec_dropped"}
    assert all(int(v) > 0 for v in reached.values()), reached
    sums = {name: {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", rest)}
            for name, rest in re.findall(r"^config (\w+): (.*)$", p.stdout, re.M)}
    assert set(sums) == {"x_in_spmv_off", "ahead0", "ahead1", "ahead2", "unset", "speculate"}
    assert not any(sums["x_in_spmv_off"].values())
    for name, live in (("ahead0", ["absorbed", "flushed"]), ("ahead1", ["committed_p", "dropped", "absorbed", "flushed"]),
                       ("ahead2", ["committed_p", "committed_r", "dropped", "absorbed", "flushed"]),
                       ("unset", ["committed_p", "absorbed"]), ("speculate", ["spec_commits", "spec_drops"])):
        for k, v in sums[name].items():
            assert (v > 0) if k in live else (v == 0 or name == "unset"), (name, sums[name])
