"""The decision behind ABFT_HIP_DEFER_FINISH that needs no GPU: `xr_can_defer_finish` (csrc/loop_state.h), asked before
calc_xr's kernel is launched, answers what `ahead_wants_p` answers behind it, over every combination of what the two
read; never with the switch off; and the switch settles to off where the run-ahead is off.  The checker
(tests/host/defer_finish_check.cpp) is built with the address and undefined-behaviour sanitizers and run on its own."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "abft_sparse_cg_amd", "csrc")


def test_decision_before_the_launch_is_the_decision_behind_it(tmp_path):
    exe = str(tmp_path / "defer_finish_check")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-I", CSRC, os.path.join(HERE, "host", "defer_finish_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # (no heap use; the leak check needs ptrace rights)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, (p.stdout, p.stderr[-2000:])
    checked, deferred = (int(v) for v in p.stdout.split())
    assert checked == 1024 and 0 < deferred < checked // 2
