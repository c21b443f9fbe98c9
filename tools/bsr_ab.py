#!/usr/bin/env python3
"""Same-box A/B of the block-row layout (pamg_mat_upload_blocked) against the layout pamg_mat_upload picks, on
vector-valued operators with three unknowns per node of an n^3 grid with 27-point neighbours:

  --kind elastic3d       SPEC §S2's L27 (x) B: four distinct values, which the dictionary tiles swallow
  --kind elastic3d_var   L_w (x) B, diagonal block 39 B, off-diagonal block (m, k) = -w B with w = 0.5 + the §S2
                         hash of the unordered pair: symmetric, SPD, no repeating values
  --node-permute SEED    a random permutation of the nodes that keeps each node's unknowns together (the shape
                         of a finite-element numbering)

--mode kernels: level-0 SpMV, residual, Jacobi (pamg_bench_rowop) and the block-Jacobi sweep (pamg_block_jacobi,
wall time of --sweeps sweeps) per layout, the layouts alternating round by round; ms and the fraction of 8 TB/s
on the layout's own stream_bytes plus the vector bytes of the operation (x, y and b, the diagonal for Jacobi,
the inverse blocks and — on the two-pass path — the residual written and read back for the block sweep).

--mode pcg: PCG to --rtol with block Jacobi V(1,1) and block Chebyshev V(2,2) over estimated bounds, on a solver
built with block_layout=3 and one without, alternating; ms and iterations (which must agree).

    python tools/bsr_ab.py --kind elastic3d_var --n 80 --node-permute 1 --mode kernels,pcg > out.jsonl
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import parallel_amg_amd as pa  # noqa: E402
from parallel_amg_amd import _lib  # noqa: E402
from parallel_amg_amd import hcsr as HC  # noqa: E402
from parallel_amg_amd.partitioned import Context, PSparseMatrix, PVector, block_jacobi, mul  # noqa: E402
from parallel_amg_amd.solver import AMGSolver  # noqa: E402

BS = 3
HBM = 8e12


def mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hash_u(i, seed=20240807):
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (i.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        return (mix64(z) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def node_matrix(n, var, perm_seed=None):
    """(rowptr, col, val) of the node-major operator; node m of the grid becomes node inv[m] under the
    permutation. Each row's columns ascending, every block whole."""
    B = 4.0 * np.eye(BS) - np.ones((BS, BS))
    g = np.arange(n)
    z, y, x = (a.reshape(-1) for a in np.meshgrid(g, g, g, indexing="ij"))
    nb = n ** 3
    m = np.arange(nb)
    new = m if perm_seed is None else np.argsort(np.random.default_rng(perm_seed).permutation(nb))
    br, bc, bw = [m], [m], [np.full(nb, -(39.0 if var else 26.0))]
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == dy == dz == 0:
                    continue
                ok = (x + dx >= 0) & (x + dx < n) & (y + dy >= 0) & (y + dy < n) & (z + dz >= 0) & (z + dz < n)
                a = m[ok]
                k = a + dx + n * (dy + n * dz)
                br.append(a)
                bc.append(k)
                bw.append(0.5 + hash_u(np.minimum(a, k) * nb + np.maximum(a, k)) if var else np.ones(len(a)))
    brow, bcol, w = new[np.concatenate(br)], new[np.concatenate(bc)], np.concatenate(bw)
    order = np.lexsort((bcol, brow))
    brow, bcol, w = brow[order], bcol[order], w[order]
    cnt = np.bincount(brow, minlength=nb)
    start = np.concatenate(([0], np.cumsum(cnt)))[:-1]
    rp = np.zeros(nb * BS + 1, np.int64)
    rp[1:] = np.cumsum(np.repeat(cnt * BS, BS))
    k = np.arange(len(brow)) - start[brow]
    col = np.empty(rp[-1], np.int32)
    val = np.empty(rp[-1], np.float64)
    for d in range(BS):
        base = rp[brow * BS + d] + k * BS
        for e in range(BS):
            col[base + e] = bcol * BS + e
            val[base + e] = (-w) * B[d, e]
    return rp, col, val


def rowop_ms(ctx, M, op, x, b, y, reps):
    ms = ctypes.c_double()
    _lib.call("pamg_bench_rowop", ctx.handle, M.handle, op, x.handle, b.handle if op else None, y.handle, 0.6, reps,
              ctypes.byref(ms))
    return ms.value


def kernels(ctx, a, A, tag):
    n = A.nrows
    mats = {lay: PSparseMatrix(ctx, A, block_size=lay if lay else 1) for lay in a.layouts}
    blocks, inv, rho_b = HC.block_diag(A, 0, BS)
    rng = np.random.default_rng(3)
    x, b, y, tmp = (PVector(ctx, n, 0, rng.standard_normal(n)) for _ in range(4))
    for lay, M in mats.items():
        M.set_block_diag(BS, blocks, inv)
        if lay and not M.blocked:
            raise SystemExit(f"{tag}: the block-row layout declined")
    om = 4.0 / (3.0 * rho_b)
    # vector bytes per row: SpMV x + y; residual + b; Jacobi + the diagonal; the block sweep x, b, y and the
    # inverse blocks, plus on two passes the residual written and read back
    vec = {"spmv": 16, "residual": 24, "jacobi": 32}
    for r in range(-1, a.rounds):  # (-1: warm-up)
        for lay, M in mats.items():
            res = {}
            for name, op in (("spmv", 0), ("residual", 1), ("jacobi", 2)):
                res[name] = (rowop_ms(ctx, M, op, x, b, y, a.reps), M.stream_bytes + vec[name] * n)
            x.fill(0.0)
            ctx.sync()
            ts = time.perf_counter()
            block_jacobi(x, M, b, tmp, om, a.sweeps)
            dt = (time.perf_counter() - ts) * 1e3 / a.sweeps
            fused = bool(lay) and M.blocked
            res["block_jacobi"] = (dt, M.stream_bytes + (24 + 8 * BS + (0 if fused else 16)) * n)
            if r < 0:
                continue
            for name, (ms, nbytes) in res.items():
                print(json.dumps({"problem": tag, "n": a.n, "rows": n, "nnz": A.nnz, "block_layout": lay, "op": name,
                                  "round": r, "ms": round(ms, 5), "stream_bytes": M.stream_bytes, "bytes": nbytes,
                                  "frac_of_8TBs": round(nbytes / (ms * 1e-3) / HBM, 4)}), flush=True)


def pcg(ctx, a, A, tag):
    be = pa.SequentialBackend(1)
    offs = np.array([0, A.nrows], np.int64)
    t0 = time.time()
    H = pa.build_hierarchy(be, {0: A}, offs, pa.SAParams(max_coarse=1000), device=ctx)
    solvers = {lay: AMGSolver(ctx, H, graph=True, reorder="off", block_layout=lay if lay else None) for lay in a.layouts}
    print(f"# {tag}: setup + uploads {time.time() - t0:.1f}s, levels {H.nlevels}", file=sys.stderr, flush=True)
    xs = HC.gen_xstar(0, A.nrows, 20240807)
    A0 = solvers[a.layouts[0]].A_dev[0]
    b = PVector(ctx, A.nrows)
    mul(b, A0, PVector(ctx, A.nrows, 0, xs))
    for S in solvers.values():
        S.set_block_size(BS)
    for kind, nu in (("block_jacobi", (1, 1)), ("block_chebyshev", (2, 2))):
        for S in solvers.values():
            S.set_smoother(kind, ratio=4.0, lmax="estimate")
            S.set_sweeps(*nu)
        for r in range(-1, a.rounds):  # (-1: warm-up and graph capture)
            for lay, S in solvers.items():
                x = S.new_vector()
                ctx.sync()
                ts = time.perf_counter()
                its, hist = S.pcg(x, b, a.rtol, 200)
                dt = time.perf_counter() - ts
                if r >= 0:
                    print(json.dumps({"problem": tag, "n": a.n, "rows": A.nrows, "block_layout": lay,
                                      "blocked": bool(S.A_dev[0].blocked), "smoother": kind, "sweeps": list(nu),
                                      "round": r, "iterations": its, "ms": round(dt * 1e3, 3),
                                      "rel_residual": float(hist[-1] / hist[0])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=["elastic3d", "elastic3d_var"], default="elastic3d_var")
    ap.add_argument("--n", type=int, default=80)
    ap.add_argument("--node-permute", type=int, default=None, metavar="SEED")
    ap.add_argument("--block-layout", default="0,3", help="layouts to run: 0 (pamg_mat_upload's), 3, or both")
    ap.add_argument("--mode", default="kernels,pcg")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--rtol", type=float, default=1e-8)
    a = ap.parse_args()
    a.layouts = [int(v) for v in a.block_layout.split(",")]
    if any(v not in (0, BS) for v in a.layouts):
        ap.error("--block-layout takes 0 and 3")
    tag = a.kind + ("" if a.node_permute is None else f"+node_permute{a.node_permute}")
    t0 = time.time()
    rp, col, val = node_matrix(a.n, a.kind == "elastic3d_var", a.node_permute)
    A = HC.HCSR.from_arrays(rp, col, val, len(rp) - 1)
    del rp, col, val
    print(f"# {tag}: matrix built in {time.time() - t0:.1f}s, {A.nrows} rows, {A.nnz} nonzeros", file=sys.stderr, flush=True)
    ctx = Context(0)
    for mode in a.mode.split(","):
        {"kernels": kernels, "pcg": pcg}[mode](ctx, a, A, tag)


if __name__ == "__main__":
    main()
