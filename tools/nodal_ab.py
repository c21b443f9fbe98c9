#!/usr/bin/env python3
"""Same-box A/B of the nodal hierarchy (SPEC §S14) with every operator in block rows against the scalar
hierarchy with level 0 in block rows (the best path before it), on the node-major operators of tools/bsr_ab.py:
three unknowns per node of an n^3 grid, 27-point neighbours; problem a: elastic3d's constant coefficients,
b: variable coefficients in grid order, c: the same with the nodes renumbered at random.

--mode kernels: R_0 (SpMV) and P_0 (prolongate-add) of the nodal hierarchy in the layouts of a plain upload
("tiles"), in block rows with a lane per node ("node") and, R_0 only, with a lane per scalar row ("row";
PAMG_BSR_ROW_LANES selects the form at upload), for k = 1 (pamg_bench_rowop), 2 and 4 columns
(pamg_bench_rowop_multi), alternating round by round in one process; medians of --rounds.

--mode pcg: PCG to --rtol with block Jacobi V(1,1), lmax="estimate": the scalar hierarchy with block_layout=3
and block data on level 0 against the nodal hierarchy with block_layout="all" and block data on every level,
for one right-hand side (pcg) and four (pcg_multi), alternating; ms and iterations. Also the host's setup times.

    python tools/nodal_ab.py --n 80 --problems b --mode kernels,pcg > out.jsonl
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import parallel_amg_amd as pa  # noqa: E402
from bsr_ab import BS, node_matrix  # noqa: E402
from parallel_amg_amd import _lib  # noqa: E402
from parallel_amg_amd import hcsr as HC  # noqa: E402
from parallel_amg_amd.partitioned import Context, MultiVector, PSparseMatrix, PVector, mul  # noqa: E402
from parallel_amg_amd.solver import AMGSolver  # noqa: E402

SEED = 20240807


def emit(**kw):
    print(json.dumps(kw), flush=True)


def upload(ctx, M, form):
    """M in the layouts of a plain upload ("tiles") or in block rows, a lane per node or per scalar row."""
    if form == "tiles":
        return PSparseMatrix(ctx, M)
    os.environ["PAMG_BSR_ROW_LANES"] = "1" if form == "row" else "0"
    try:
        D = PSparseMatrix(ctx, M, block_rows=BS)
    finally:
        del os.environ["PAMG_BSR_ROW_LANES"]
    if not D.blocked or D.row_lanes != (form == "row"):
        raise SystemExit(f"{form}: the block-row layout declined")
    return D


def rowop_ms(ctx, D, op, x, y, reps, multi):
    ms = ctypes.c_double()
    _lib.call("pamg_bench_rowop_multi" if multi else "pamg_bench_rowop", ctx.handle, D.handle, op, x.handle, None,
              y.handle, 0.0, reps, ctypes.byref(ms))
    return ms.value


def kernels(ctx, a, H, tag):
    lp = H.levels[0][0]
    rng = np.random.default_rng(3)
    for name, M, op, forms in (("R0", lp.R, 0, ("tiles", "node", "row")), ("P0", lp.P, 3, ("tiles", "node"))):
        ups = {f: upload(ctx, M, f) for f in forms}
        for k in (1, 2, 4):
            if k == 1:
                x, y = PVector(ctx, M.ncols, 0, rng.standard_normal(M.ncols)), PVector(ctx, M.nrows)
            else:
                x, y = MultiVector.from_numpy(ctx, rng.standard_normal((M.ncols, k))), MultiVector(ctx, M.nrows, k)
            rec = {f: [] for f in forms}
            for r in range(-1, a.rounds):  # (-1: warm-up)
                for f in forms:
                    t = rowop_ms(ctx, ups[f], op, x, y, a.reps, k > 1)
                    if r >= 0:
                        rec[f].append(t)
            emit(problem=tag, n=a.n, mode="kernel", operator=name, rows=M.nrows, cols=M.ncols, nnz=M.nnz, k=k,
                 ms={f: round(float(np.median(v)), 5) for f, v in rec.items()},
                 spread={f: [round(min(v), 5), round(max(v), 5)] for f, v in rec.items()},
                 stream_bytes={f: ups[f].stream_bytes for f in forms}, rounds=a.rounds)
        del ups


def pcg(ctx, a, H, Hs, tag):
    n = H.levels[0][0].A.nrows
    sides = {}
    S = AMGSolver(ctx, Hs, graph=True, reorder="off", block_layout=BS)
    S.set_block_size(BS)
    sides["scalar+level0"] = S
    S = AMGSolver(ctx, H, graph=True, reorder="off", block_layout="all")
    S.set_block_size(BS, levels="all")
    sides["nodal+all"] = S
    for S in sides.values():
        S.set_smoother("block_jacobi", ratio=4.0, lmax="estimate")
        S.set_sweeps(1, 1)
    k = 4
    Ball, xs = MultiVector(ctx, n, k), PVector(ctx, n)
    for c in range(k):
        xs.fill_xstar(0, SEED + c)
        mul(Ball.column(c), sides["nodal+all"].A_dev[0], xs)
    b0 = PVector(ctx, n, 0, Ball.to_numpy()[:, 0])
    rec = {s: {"ms1": [], "ms4": []} for s in sides}
    its = {}
    for r in range(-1, a.rounds):  # (-1: warm-up and graph capture)
        for s, S in sides.items():
            x = S.new_vector()
            ctx.sync()
            ts = time.perf_counter()
            it1, _h = S.pcg(x, b0, a.rtol, 300)
            d1 = time.perf_counter() - ts
            X = S.new_multivector(k)
            ctx.sync()
            ts = time.perf_counter()
            it4, _h = S.pcg_multi(X, Ball, a.rtol, 300)
            d4 = time.perf_counter() - ts
            its[s] = (int(it1), [int(v) for v in it4])
            if r >= 0:
                rec[s]["ms1"].append(d1 * 1e3)
                rec[s]["ms4"].append(d4 * 1e3)
    for s, S in sides.items():
        emit(problem=tag, n=a.n, rows=n, mode="pcg", side=s, smoother="block_jacobi", sweeps=[1, 1],
             levels=[int(v) for v in S.level_rows], iterations_k1=its[s][0], iterations_k4=its[s][1],
             ms_k1=round(float(np.median(rec[s]["ms1"])), 3), ms_k4=round(float(np.median(rec[s]["ms4"])), 3),
             spread_k1=[round(min(rec[s]["ms1"]), 3), round(max(rec[s]["ms1"]), 3)],
             spread_k4=[round(min(rec[s]["ms4"]), 3), round(max(rec[s]["ms4"]), 3)],
             blocked={w: [bool(q.blocked) for q in ops] for w, ops in (("A", S.A_dev), ("P", S.P), ("R", S.R))},
             rounds=a.rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80)
    ap.add_argument("--problems", default="b", help="a: elastic3d; b: elastic3d_var in grid order; c: nodes permuted")
    ap.add_argument("--mode", default="kernels,pcg")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--max-coarse", type=int, default=1000)
    a = ap.parse_args()
    ctx = Context(0)
    be = pa.SequentialBackend(1)
    for p in a.problems.split(","):
        if p not in ("a", "b", "c"):
            ap.error("--problems takes a, b and c")
        tag = {"a": "elastic3d", "b": "elastic3d_var", "c": "elastic3d_var+node_permute1"}[p]
        rp, col, val = node_matrix(a.n, p != "a", 1 if p == "c" else None)
        A = HC.HCSR.from_arrays(rp, col, val, len(rp) - 1)
        del rp, col, val
        offs = np.array([0, A.nrows], np.int64)
        t0 = time.perf_counter()
        H = pa.build_hierarchy(be, {0: A}, offs, pa.SAParams(max_coarse=a.max_coarse, block_size=BS))
        t_nodal = time.perf_counter() - t0
        modes = a.mode.split(",")
        Hs, t_scalar = None, None
        if "pcg" in modes:
            t0 = time.perf_counter()
            Hs = pa.build_hierarchy(be, {0: A}, offs, pa.SAParams(max_coarse=a.max_coarse))
            t_scalar = time.perf_counter() - t0
        emit(problem=tag, n=a.n, rows=A.nrows, nnz=A.nnz, mode="setup", host_setup_s_nodal=round(t_nodal, 2),
             host_setup_s_scalar=None if t_scalar is None else round(t_scalar, 2),
             levels_nodal=[int(H.levels[l][0].A.nrows) for l in range(H.nlevels)],
             levels_scalar=None if Hs is None else [int(Hs.levels[l][0].A.nrows) for l in range(Hs.nlevels)])
        if "kernels" in modes:
            kernels(ctx, a, H, tag)
        if "pcg" in modes:
            pcg(ctx, a, H, Hs, tag)


if __name__ == "__main__":
    main()
