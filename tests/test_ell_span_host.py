"""The windowed ELL's group-pair pass (csrc/ell_span.h: plain C++ over the groups' column runs) under
ASan/UBSan: tools/ell_span_check.cpp pairs the windows of generated band operators and checks every
union window and carried lof word; any sanitizer report aborts it. CPU only, no HIP runtime."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("span") / "ell_span_check")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", *SAN, os.path.join(ROOT, "tools", "ell_span_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


# (rows, capacity, offsets) -> (groups, pairs): bands that pair two and two, an odd group left over and a
# partial last slice, a capacity under the inner unions (512 + 120; the two end pairs, their windows cut
# at the matrix's edge, still fit: 572) and one under the windows, windows that share
# two columns, blocks 1024 apart (runs far from the rows, several per window)
CASES = [((2048, 4096, -60, -1, 0, 1, 60), (8, 4)), ((1448, 4096, -60, -1, 0, 1, 60), (6, 3)),
         ((1280, 4096, -60, -1, 0, 1, 60), (5, 2)), ((2048, 620, -60, -1, 0, 1, 60), (8, 2)),
         ((2048, 300, -60, -1, 0, 1, 60), (8, 0)), ((2048, 4096, -1, 0, 1), (8, 0)),
         ((8192, 4096, -1024, -40, 0, 40, 1024), (32, 16))]


@pytest.mark.parametrize("args,want", CASES)
def test_pair_pass_clean_under_asan_ubsan(checker, args, want):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([checker, *map(str, args)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["bad"] == 0 and (got["groups"], got["pairs"]) == want, got
