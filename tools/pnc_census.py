#!/usr/bin/env python3
"""Host census of the level-0 prolongation's row lengths as k_rows_pnct's gather trimming sees them
(CPU only, no GPU): the rows per length, the longest row of every wave (64 consecutive points of a
grid line — a wave of the 64 x 4 tile and of the line-block march alike), and the longest row of
every wave and step, a step taking one plane of each of the two z-streams of a 32-plane unit (planes
z and z + 16). The means are the gather instructions per stream a wave issues where the line-block
march issues 7. P0 comes from the library's own host setup, as in tools/pattern_census.py.

    python tools/pnc_census.py --n 128            # seconds
    python tools/pnc_census.py --n 512            # ~2 min, ~30 GB of host memory
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import parallel_amg_amd as pa  # noqa: E402
from parallel_amg_amd import hcsr as H  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    a = ap.parse_args()
    n = a.n
    be = pa.SequentialBackend(1)
    A, offs, xs = pa.generate_problem(be, "poisson3d", n)
    A0 = A[0]
    omega = 4.0 / (3.0 * H.gershgorin(A0, 0))
    agg, nc = H.aggregate(A0, 0, 0.02)
    T = H.tentative(agg, nc, 0, nc)
    AT = H.spgemm(A0, 0, T, np.zeros(0, np.int64), None)
    P = H.smooth(A0, 0, T, AT, omega)
    lens = np.diff(P.rowptr).astype(np.int64)
    del A, A0, T, AT, P
    out = {"n": n, "rows": int(lens.size), "mean_row_length": round(float(lens.mean()), 4),
           "rows_by_length": {str(k): int(v) for k, v in enumerate(np.bincount(lens, minlength=8)) if k}}
    wave = lens.reshape(-1, 64).max(axis=1)                     # (plane, line, 64-point piece)
    out["waves_by_longest_row"] = {str(k): int(v) for k, v in enumerate(np.bincount(wave, minlength=8)) if v}
    out["mean_wave_longest_row"] = round(float(np.maximum(wave, 3).mean()), 4)  # (the shortest body issues 3)
    # a step: planes z and z + 16 of a 32-plane unit (two streams of 16 planes)
    w = wave.reshape(n, -1)                                     # (plane, wave of the plane)
    zlen, part = min(32, n), (min(32, n) + 1) // 2
    steps = []
    for z0 in range(0, n, zlen):
        lo = w[z0:z0 + part]
        hi = w[z0 + part:z0 + zlen]
        m = min(len(lo), len(hi))
        steps.append(np.maximum(lo[:m], hi[:m]).ravel())
        steps.append(lo[m:].ravel())
    step = np.maximum(np.concatenate(steps), 3)
    out["steps_by_longest_row"] = {str(k): int(v) for k, v in enumerate(np.bincount(step, minlength=8)) if v}
    out["mean_step_longest_row"] = round(float(step.mean()), 4)
    out["needed_gather_lanes_of_7"] = round(float(lens.mean()) / 7.0, 4)
    out["needed_gather_lanes_of_issued"] = round(float(lens.mean()) / float(step.mean()), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
