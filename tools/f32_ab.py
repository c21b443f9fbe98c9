#!/usr/bin/env python3
"""Same-box A/B of operator values stored in binary32 (SPEC §S15; pamg_mat_upload_f32, AMGSolver(values="f32"))
against fp64 values, on the node-major operators of tools/bsr_ab.py: three unknowns per node of an n^3 grid,
27-point neighbours, variable coefficients; problem b: in grid order, c: the nodes renumbered at random.

--mode kernels: the level-0 operator in block rows — SpMV, residual, Jacobi and the fused block-Jacobi sweep — and
R_0 (SpMV) and P_0 (prolongate-add) of the nodal hierarchy, for k = 1, 2 and 4 columns (pamg_bench_rowop_multi), the
fp64 and the f32 upload alternating round by round in one process; medians of --rounds, --reps launches per figure,
and each side's stream_bytes (the byte model: (4 + 4/9) / (8 + 4/9) = 0.53 of the matrix stream).

--mode pcg: PCG to --rtol with block Jacobi V(1,1), lmax="estimate", values="f64" against "f32", alternating: the
scalar hierarchy with block_layout=3 and the nodal hierarchy with block_layout="all"; ms, iterations and the final
||b - A x|| / ||b|| with the exact operator.

    python tools/f32_ab.py --n 80 --problems b,c --mode kernels,pcg > profiles/f32_values/f32_ab_80.jsonl
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
from parallel_amg_amd.hierarchy import round_f32  # noqa: E402
from parallel_amg_amd.partitioned import Context, MultiVector, PSparseMatrix, PVector, mul, residual  # noqa: E402
from parallel_amg_amd.solver import AMGSolver  # noqa: E402

SEED = 20240807
SIDES = ("f64", "f32")


def emit(**kw):
    print(json.dumps(kw), flush=True)


def rowop_ms(ctx, D, op, X, B, Y, omega, reps):
    ms = ctypes.c_double()
    _lib.call("pamg_bench_rowop_multi", ctx.handle, D.handle, op, X.handle, B.handle if B is not None else None,
              Y.handle, omega, reps, ctypes.byref(ms))
    return ms.value


def ab(ctx, a, ups, ops, tag, name, M):
    """ms per launch of every (op, k), the two uploads alternating round by round."""
    rng = np.random.default_rng(3)
    for opname, op, needs_b in ops:
        for k in (1, 2, 4):
            X = MultiVector.from_numpy(ctx, rng.standard_normal((M.ncols, k)))
            Y = MultiVector(ctx, M.nrows, k)
            B = MultiVector.from_numpy(ctx, rng.standard_normal((M.nrows, k))) if needs_b else None
            rec = {s: [] for s in SIDES}
            for r in range(-1, a.rounds):  # (-1: warm-up)
                for s in SIDES:
                    t = rowop_ms(ctx, ups[s], op, X, B, Y, 0.6, a.reps)
                    if r >= 0:
                        rec[s].append(t)
            med = {s: float(np.median(v)) for s, v in rec.items()}
            emit(problem=tag, n=a.n, mode="kernel", operator=name, op=opname, rows=M.nrows, cols=M.ncols, nnz=M.nnz,
                 k=k, ms={s: round(med[s], 5) for s in SIDES},
                 spread={s: [round(min(v), 5), round(max(v), 5)] for s, v in rec.items()},
                 ratio=round(med["f32"] / med["f64"], 3),
                 stream_bytes={s: ups[s].stream_bytes for s in SIDES},
                 stream_ratio=round(ups["f32"].stream_bytes / ups["f64"].stream_bytes, 3),
                 row_lanes=bool(ups["f32"].row_lanes), rounds=a.rounds, reps=a.reps)


def kernels(ctx, a, A, H, tag):
    ups = {"f64": PSparseMatrix(ctx, A, block_size=BS), "f32": PSparseMatrix(ctx, A, block_size=BS, value_bits=32)}
    if not (ups["f64"].blocked and ups["f32"].f32_storage):
        raise SystemExit("A0: the block-row layout declined")
    ups["f64"].set_block_diag(BS, *HC.block_diag(A, 0, BS)[:2])
    ups["f32"].set_block_diag(BS, *HC.block_diag(round_f32(A), 0, BS)[:2])
    ab(ctx, a, ups, (("spmv", 0, False), ("residual", 1, True), ("jacobi", 2, True), ("block_jacobi_fused", 7, True)),
       tag, "A0", A)
    del ups
    lp = H.levels[0][0]
    for name, M, ops in (("R0", lp.R, (("spmv", 0, False),)), ("P0", lp.P, (("prolong_add", 3, False),))):
        ups = {"f64": PSparseMatrix(ctx, M, block_rows=BS), "f32": PSparseMatrix(ctx, M, block_rows=BS, value_bits=32)}
        if not (ups["f64"].blocked and ups["f32"].f32_storage):
            raise SystemExit(f"{name}: the block-row layout declined")
        ab(ctx, a, ups, ops, tag, name, M)
        del ups


def pcg(ctx, a, A, hiers, tag):
    n = A.nrows
    for cfg, (H, layout, levels) in hiers.items():
        sides = {}
        for s in SIDES:
            S = AMGSolver(ctx, H, graph=True, reorder="off", block_layout=layout, values=s)
            S.set_block_size(BS, levels=levels)
            S.set_smoother("block_jacobi", ratio=4.0, lmax="estimate")
            S.set_sweeps(1, 1)
            sides[s] = S
        xs, b = PVector(ctx, n), PVector(ctx, n)
        xs.fill_xstar(0, SEED)
        mul(b, sides["f64"].A[0], xs)
        rec, its, rel = {s: [] for s in SIDES}, {}, {}
        for r in range(-1, a.rounds):  # (-1: warm-up and graph capture)
            for s, S in sides.items():
                x = S.new_vector()
                ctx.sync()
                ts = time.perf_counter()
                it, _h = S.pcg(x, b, a.rtol, 300, lookahead=0)
                d = time.perf_counter() - ts
                if r >= 0:
                    rec[s].append(d * 1e3)
                its[s] = int(it)
                rr = PVector(ctx, n)
                rel[s] = residual(rr, sides["f64"].A[0], x, b, with_norm=True)  # with the exact fp64 operator
        bn = float(np.linalg.norm(b.own_values()))
        for s, S in sides.items():
            emit(problem=tag, n=a.n, rows=n, mode="pcg", hierarchy=cfg, values=s, smoother="block_jacobi", sweeps=[1, 1],
                 levels=[int(v) for v in S.level_rows], iterations=its[s], ms=round(float(np.median(rec[s])), 3),
                 spread=[round(min(rec[s]), 3), round(max(rec[s]), 3)], final_rel_residual=rel[s] / bn,
                 lmax=[round(float(v), 6) for v in S.lmax],
                 f32_storage={w: [bool(q.f32_storage) for q in ops] for w, ops in (("A", S.A_dev), ("P", S.P), ("R", S.R))},
                 matrix_stream_bytes=int(sum(q.stream_bytes for ops in (S.A_dev[:-1], S.P, S.R) for q in ops)),
                 rounds=a.rounds)
        del sides


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80)
    ap.add_argument("--problems", default="b,c", help="b: elastic3d_var in grid order; c: nodes permuted")
    ap.add_argument("--mode", default="kernels,pcg")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--max-coarse", type=int, default=1000)
    a = ap.parse_args()
    ctx = Context(0)
    be = pa.SequentialBackend(1)
    modes = a.mode.split(",")
    for p in a.problems.split(","):
        if p not in ("b", "c"):
            ap.error("--problems takes b and c")
        tag = {"b": "elastic3d_var", "c": "elastic3d_var+node_permute1"}[p]
        rp, col, val = node_matrix(a.n, True, 1 if p == "c" else None)
        A = HC.HCSR.from_arrays(rp, col, val, len(rp) - 1)
        del rp, col, val
        offs = np.array([0, A.nrows], np.int64)
        H = pa.build_hierarchy(be, {0: A}, offs, pa.SAParams(max_coarse=a.max_coarse, block_size=BS))
        if "kernels" in modes:
            kernels(ctx, a, A, H, tag)
        if "pcg" in modes:
            Hs = pa.build_hierarchy(be, {0: A}, offs, pa.SAParams(max_coarse=a.max_coarse))
            pcg(ctx, a, A, {"scalar+level0": (Hs, BS, (0,)), "nodal+all": (H, "all", "all")}, tag)
            del Hs
        del H, A


if __name__ == "__main__":
    main()
