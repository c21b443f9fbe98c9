"""The V-cycle planner (csrc/cycle_plan.h: plain C++, which vector every step reads and writes) under
ASan/UBSan: tools/cycle_plan_check.cpp runs every plan symbolically — no aliasing, no stale read, no
write to b, the result where the plan says, the step counts, the spare vector's rule — and prints the
plans of the recorded cases, which must equal tests/golden/cycle_plan_parent.jsonl: the step lists the
cycle driver issued before the planner existed (recorded from that code compiled against logging stubs).
CPU only, no HIP runtime."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cycle_plan_parent.jsonl")
SAN = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "cycle_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", *SAN, os.path.join(ROOT, "tools", "cycle_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _clean(r):
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_every_plan_holds_the_invariants(checker):
    r = subprocess.run([checker], capture_output=True, text=True, env=ENV, timeout=300)
    _clean(r)
    got = json.loads(r.stdout.strip().splitlines()[-1])
    # 3 depths x 64 x 64 degrees x 2 families x 2 guesses, the fused and pipeline variants, 128 polynomials
    assert got["bad"] == 0 and got["plans"] >= 3 * 64 * 64 * 4, got


def test_plans_equal_the_recorded_step_lists(checker):
    r = subprocess.run([checker, "--cases", GOLDEN], capture_output=True, text=True, env=ENV, timeout=120)
    _clean(r)
    want = open(GOLDEN).read().splitlines()
    got = r.stdout.splitlines()
    assert len(want) == 218 and len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    # the recorded set: both families, nu1, nu2 in {1, 2, 3, 4, 6}, both guesses, 2 and 3 levels, the
    # fused level-0 pass, and the pipeline's head and two steady segments
    cases = [json.loads(w) for w in want]
    whole = {(c["L"], c["cheb"], c["zero0"], c["nu1"], c["nu2"]) for c in cases if c["post"] == 1 and c["fused"] == 0}
    assert len(whole) == 2 * 2 * 2 * 25
    assert sum(c["fused"] for c in cases if c["post"] == 1) == 2 * 5
    assert {(c["L"], c["fused"], c["given"]) for c in cases if c["post"] == 0} == {
        (L, f, g) for L in (2, 3) for f, g in ((0, "-"), (1, "-"), (0, "T"), (0, "U0"))}
