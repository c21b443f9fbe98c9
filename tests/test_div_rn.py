"""div_rn (parallel_amg_amd/csrc/div_rn.h — the text kernels.hip compiles) is IEEE division,
bit for bit, over its whole domain: tools/div_check.c, built with the host compiler and
-ffp-contract=off as its header comment says, on random operands over 2^-1074 .. 2^1023, the
guard's edges, near-midpoint quotients, overflowing quotients and constructed subnormal ties.
(With the [2^-900, 2^900] guard the same run reports mismatches in the full-range, guard-edge
and constructed classes: every overflowing quotient was NaN.)"""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = 2_000_000  # ~5.5e6 checked quotients, well under a second of host time


def _build(tmp_path):
    exe = str(tmp_path / "div_check")
    cmd = ["gcc", "-O2", "-ffp-contract=off", "-Wall", "-Werror",
           os.path.join(ROOT, "tools", "div_check.c"), "-lm", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_div_rn_is_ieee_division(tmp_path):
    out = subprocess.run([_build(tmp_path), str(CASES)], capture_output=True, text=True, timeout=120)
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["cases"] > 2 * CASES
    assert res["mismatches"] == 0, res
    assert out.returncode == 0


def test_kernels_use_the_checked_text():
    """kernels.hip includes div_rn.h and keeps no copy of its own; neither does the tool."""
    for rel in ("parallel_amg_amd/csrc/kernels.hip", "tools/div_check.c"):
        src = open(os.path.join(ROOT, rel)).read()
        assert "div_rn.h\"" in src, rel
        assert "double div_rn(" not in src, rel
