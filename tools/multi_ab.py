#!/usr/bin/env python3
"""Same-box A/B of several right-hand sides in one pass (SPEC §S13) against one call per right-hand side, on
the variable-coefficient node-major operator of tools/bsr_ab.py (three unknowns per node of an n^3 grid, 27-point
neighbours, values that do not repeat) in the block-row layout, in grid order (problem b) and with the nodes
randomly renumbered (problem c), for k = 1, 2, 4, 8 columns.

--mode kernels: pamg_bench_rowop_multi on k columns against k x pamg_bench_rowop on one, for SpMV, residual,
Jacobi (ops 0, 1, 2) and the fused block Jacobi sweep (op 7; the single-column side is pamg_block_jacobi's wall
time per sweep), alternating round by round. Beside each ratio the byte model's: (stream_bytes + k V) / (k
(stream_bytes + V)), V the operation's vector bytes per column.

--mode pcg: pcg_multi against k successive pcg calls on the same solver (block Jacobi V(1,1), lmax="estimate"),
alternating round by round, identical right-hand sides (column c: A x* of seed 20240807 + c); medians of
--rounds. Also the share of a single-column iteration that the multi-column call still runs once per column:
everything but level 0's three matrix passes and q = A p, from the per-operation profile of one cycle.

    python tools/multi_ab.py --n 80 --problems b,c --mode kernels,pcg > out.jsonl
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
from parallel_amg_amd.partitioned import Context, MultiVector, PSparseMatrix, PVector, block_jacobi, mul  # noqa: E402
from parallel_amg_amd.solver import AMGSolver  # noqa: E402

KS = (1, 2, 4, 8)
SEED = 20240807
# vector bytes per row and column: SpMV x + y; residual + b; Jacobi + the diagonal; the fused block sweep x, b, y
# and the inverse blocks
VEC = {"spmv": 16, "residual": 24, "jacobi": 32, "block_jacobi": 24 + 8 * BS}
OPS = {"spmv": 0, "residual": 1, "jacobi": 2, "block_jacobi": 7}


def emit(**kw):
    print(json.dumps(kw), flush=True)


def rowop_ms(ctx, M, op, x, b, y, omega, reps, multi):
    ms = ctypes.c_double()
    _lib.call("pamg_bench_rowop_multi" if multi else "pamg_bench_rowop", ctx.handle, M.handle, op, x.handle,
              b.handle if op else None, y.handle, omega, reps, ctypes.byref(ms))
    return ms.value


def kernels(ctx, a, A, tag):
    n = A.nrows
    M = PSparseMatrix(ctx, A, block_size=BS)
    if not M.blocked:
        raise SystemExit(f"{tag}: the block-row layout declined")
    blocks, inv, rho_b = HC.block_diag(A, 0, BS)
    M.set_block_diag(BS, blocks, inv)
    om = 4.0 / (3.0 * rho_b)
    rng = np.random.default_rng(3)
    x1, b1, y1, tmp = (PVector(ctx, n, 0, rng.standard_normal(n)) for _ in range(4))
    for k in KS:
        X, Bv, Y = (MultiVector.from_numpy(ctx, rng.standard_normal((n, k))) for _ in range(3))
        rec = {name: {"multi": [], "single": []} for name in OPS}
        for r in range(-1, a.rounds):  # (-1: warm-up)
            for name, op in OPS.items():
                tm = rowop_ms(ctx, M, op, X, Bv, Y, om, a.reps, True)
                if op == 7:
                    x1.fill(0.0)
                    ctx.sync()
                    ts = time.perf_counter()
                    block_jacobi(x1, M, b1, tmp, om, a.sweeps)
                    t1 = (time.perf_counter() - ts) * 1e3 / a.sweeps
                else:
                    t1 = rowop_ms(ctx, M, op, x1, b1, y1, om, a.reps, False)
                if r >= 0:
                    rec[name]["multi"].append(tm)
                    rec[name]["single"].append(t1)
        for name in OPS:
            tm, t1 = float(np.median(rec[name]["multi"])), float(np.median(rec[name]["single"]))
            V = VEC[name] * n
            emit(problem=tag, n=a.n, rows=n, mode="kernel", op=name, k=k, ms_multi=round(tm, 5), ms_single=round(t1, 5),
                 ms_k_singles=round(k * t1, 5), ratio=round(tm / (k * t1), 4),
                 byte_model_ratio=round((M.stream_bytes + k * V) / (k * (M.stream_bytes + V)), 4),
                 stream_bytes=M.stream_bytes, vector_bytes_per_column=V, rounds=a.rounds)


def pcg(ctx, a, A, tag):
    be = pa.SequentialBackend(1)
    n = A.nrows
    t0 = time.time()
    H = pa.build_hierarchy(be, {0: A}, np.array([0, n], np.int64), pa.SAParams(max_coarse=1000), device=ctx)
    S = AMGSolver(ctx, H, graph=True, reorder="off", block_layout=BS)
    print(f"# {tag}: setup + uploads {time.time() - t0:.1f}s, levels {H.nlevels}", file=sys.stderr, flush=True)
    if not S.A_dev[0].blocked:
        raise SystemExit(f"{tag}: the block-row layout declined")
    S.set_block_size(BS)
    S.set_smoother("block_jacobi", ratio=4.0, lmax="estimate")
    S.set_sweeps(1, 1)
    kmax = max(KS)
    Ball = MultiVector(ctx, n, kmax)
    xs = PVector(ctx, n)
    for c in range(kmax):
        xs.fill_xstar(0, SEED + c)
        mul(Ball.column(c), S.A_dev[0], xs)
    bh = Ball.to_numpy()
    cols = [PVector(ctx, n, 0, bh[:, c]) for c in range(kmax)]
    its1 = None
    for k in KS:
        Bv = MultiVector.from_numpy(ctx, bh[:, :k])
        tm, t1, its_m, its_s = [], [], None, None
        for r in range(-1, a.rounds):  # (-1: warm-up and graph capture)
            X = S.new_multivector(k)
            ctx.sync()
            ts = time.perf_counter()
            its_m, _h = S.pcg_multi(X, Bv, a.rtol, 200)
            dm = time.perf_counter() - ts
            xv = [S.new_vector() for _ in range(k)]
            ctx.sync()
            ts = time.perf_counter()
            its_s = [S.pcg(xv[c], cols[c], a.rtol, 200)[0] for c in range(k)]
            d1 = time.perf_counter() - ts
            if r >= 0:
                tm.append(dm * 1e3)
                t1.append(d1 * 1e3)
        same = all(np.array_equal(X.to_numpy()[:, c], xv[c].own_values()) for c in range(k))
        its1 = its_s[0]
        emit(problem=tag, n=a.n, rows=n, mode="pcg", smoother="block_jacobi", sweeps=[1, 1], k=k,
             iterations_multi=[int(v) for v in its_m], iterations_single=[int(v) for v in its_s], same_bits=bool(same),
             ms_multi=round(float(np.median(tm)), 3), ms_k_singles=round(float(np.median(t1)), 3),
             ratio=round(float(np.median(tm) / np.median(t1)), 4), rounds=a.rounds)
    # what still runs once per column: one iteration less level 0's three matrix passes and q = A p
    x, ms = S.new_vector(), ctypes.c_double()
    ctx.sync()
    ts = time.perf_counter()
    it, _h = S.pcg(x, cols[0], a.rtol, 200)
    t_iter = (time.perf_counter() - ts) * 1e3 / max(it, 1)
    prof = S.profile(S.new_vector(), cols[0], 10) / 10.0
    y = PVector(ctx, n)
    _lib.call("pamg_bench_rowop", ctx.handle, S.A_dev[0].handle, 0, cols[1].handle, None, y.handle, 0.0, a.reps,
              ctypes.byref(ms))
    a0 = float(prof[0, 0] + prof[0, 1] + prof[0, 4]) + ms.value
    emit(problem=tag, n=a.n, rows=n, mode="share", iterations=int(its1), ms_per_iteration=round(t_iter, 4),
         ms_level0_matrix_passes=round(a0, 4), ms_cycle_profiled=round(float(prof.sum()), 4),
         ms_p0_r0=round(float(prof[0, 2] + prof[0, 3]), 4), ms_coarse_levels=round(float(prof[1:].sum()), 4),
         per_column_share=round(max(0.0, 1.0 - a0 / t_iter), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80)
    ap.add_argument("--problems", default="b,c", help="b: elastic3d_var in grid order; c: the same, nodes permuted")
    ap.add_argument("--mode", default="kernels,pcg")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--rtol", type=float, default=1e-8)
    a = ap.parse_args()
    ctx = Context(0)
    for p in a.problems.split(","):
        if p not in ("b", "c"):
            ap.error("--problems takes b and c")
        tag = "elastic3d_var" + ("" if p == "b" else "+node_permute1")
        t0 = time.time()
        rp, col, val = node_matrix(a.n, True, None if p == "b" else 1)
        A = HC.HCSR.from_arrays(rp, col, val, len(rp) - 1)
        del rp, col, val
        print(f"# {tag}: matrix built in {time.time() - t0:.1f}s, {A.nrows} rows, {A.nnz} nonzeros", file=sys.stderr,
              flush=True)
        for mode in a.mode.split(","):
            {"kernels": kernels, "pcg": pcg}[mode](ctx, a, A, tag)


if __name__ == "__main__":
    main()
