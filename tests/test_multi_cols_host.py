"""The two layout rules of several right-hand sides (csrc/multi_cols.h, SPEC §S13) on the CPU:
tools/multi_cols_check.cpp, built stand-alone with g++ under ASan/UBSan, checks for every column count
1..8 that the launch chunks are 4, then 2, then 1 wide, cover each column exactly once and are at most two
wide ones plus a single, and that a multi-vector's column stride is a multiple of 32 doubles that holds
n_own + n_ghost. No HIP runtime."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mcols") / "multi_cols_check")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", *SAN, os.path.join(ROOT, "tools", "multi_cols_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_chunks_and_stride_rules(checker):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([checker], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["bad"] == 0 and got["cases"] > 300, got
