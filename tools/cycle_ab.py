#!/usr/bin/env python3
"""Same-box A/B of a launch-time libpamg option on the bench's timed region: one 512^3 setup and
upload, then alternating values (a, b, a, b, ...), each timed as bench.py times it (graph replay
of --steps pipelined V-cycles, synchronised on both sides; the graphs are re-captured after every
switch) and checked for the same bits of x.

    python tools/cycle_ab.py --ab chain_store_x=1,0 --rounds 3 > ab.jsonl

--pcg compares smoothers instead, on the same upload: each variant — j or c (Jacobi, Chebyshev with
--ratio) followed by the two sweep counts / degrees — solves A x = b by PCG to --rtol once to warm up
(and capture) and --rounds times timed; one JSON line per solve with its time and iteration count.
A trailing e (j11e, c22e) runs the variant over the estimated bounds of SPEC §S10 (AMGSolver.estimate_lmax,
10 steps, boost 1.1; estimated once, its wall time per level on a line of its own) instead of Gershgorin's.

    python tools/cycle_ab.py --pcg j11,j22,j33,c22,c33 --rounds 3 > pcg.jsonl
    python tools/cycle_ab.py --pcg j11,j11e,c22,c22e --rounds 3 > pcg_estimate.jsonl

--lookahead (with --pcg) compares PCG entry points on each variant: none is pamg_pcg, an integer L
pamg_pcg_resident with that lookahead (SPEC §S11); one JSON line per solve, with the iterations
enqueued / run past convergence and whether x, the count and the history carry the first solve's bits.

    python tools/cycle_ab.py --pcg j11,c22 --lookahead none,0,1,2 --kind poisson3d --n 128 > pcg_resident.jsonl

A leading b (bj11, bc22e) is the point-block form of the variant (SPEC §S12) with --block-size unknowns per
node on level 0 (AMGSolver.set_block_size); its bounds are rho_b, or with a trailing e the block estimate.
--sweep-cost N times N level-0 Jacobi sweeps against N block Jacobi sweeps on the same upload.

    python tools/cycle_ab.py --kind elastic3d --n 80 --pcg j11e,bj11e,c22e,bc22e --rounds 3 > pcg_block.jsonl
    python tools/cycle_ab.py --kind elastic3d --n 80 --sweep-cost 50 --rounds 3 > sweep_cost.jsonl
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
from parallel_amg_amd.partitioned import Context, PVector, mul  # noqa: E402
from parallel_amg_amd.solver import AMGSolver  # noqa: E402


def set_opt(k, v):
    _lib.call("pamg_set_option", k.encode(), int(v))


def estimate_timed(ctx, S, a, block=False):
    """S.estimate_lmax() with its defaults; prints the bounds beside Gershgorin's and, from a second
    pass of the same calls one level at a time, the wall time of each level's estimate. block: the
    block estimate on the levels with block data."""
    from parallel_amg_amd.partitioned import estimate_lmax as scalar_estimate, estimate_lmax_block
    from parallel_amg_amd.hierarchy import SEED
    est = S.estimate_lmax(block=block)

    def estimate_lmax(A, v, y, steps):
        return (estimate_lmax_block if block and A.block_size > 1 else scalar_estimate)(A, v, y, steps)
    ms = []
    for l in range(S.L - 1):
        A = S.A_dev[l]
        v, y = A.new_input_vector(), A.new_output_vector()
        ctx.sync()
        ts = time.perf_counter()
        v.fill_xstar(0, SEED + l)
        estimate_lmax(A, v, y, 10)
        ms.append(round((time.perf_counter() - ts) * 1e3, 3))
    print(json.dumps({"kind": a.kind, "n": a.n, "estimate_lmax": est, "lambda_10": [float(h[-1]) for h in S.lmax_hist],
                      "gershgorin": [S._H.levels[l][S.part].rho for l in range(S.L - 1)],
                      "block": block, "rho_b": {str(l): v for l, v in S.rho_b.items()} if block else {},
                      "rows": S.level_rows[:-1], "estimate_ms_per_level": ms}), flush=True)
    return est


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--kind", default="poisson3d")
    ap.add_argument("--ab", default=None, help="KEY=a,b")
    ap.add_argument("--pcg", default=None, help="smoother variants, e.g. j11,j22,c22")
    ap.add_argument("--ratio", type=float, default=4.0)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--maxit", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lookahead", default=None,
                    help="with --pcg: entry points to compare, e.g. none,0,1,2 (none = pamg_pcg, an integer = "
                         "pamg_pcg_resident with that lookahead)")
    ap.add_argument("--block-size", type=int, default=3, help="unknowns per node of the b variants / --sweep-cost")
    ap.add_argument("--sweep-cost", type=int, default=0, metavar="N",
                    help="time N level-0 Jacobi sweeps against N block Jacobi sweeps")
    a = ap.parse_args()
    if (a.ab is None) + (a.pcg is None) + (a.sweep_cost == 0) != 2:
        ap.error("one of --ab, --pcg and --sweep-cost")
    looks = None
    if a.lookahead is not None:
        if not a.pcg:
            ap.error("--lookahead goes with --pcg")
        try:
            looks = [None if v == "none" else int(v) for v in a.lookahead.split(",")]
        except ValueError:
            ap.error(f"bad --lookahead list {a.lookahead!r}")
        if any(v is not None and v < 0 for v in looks):
            ap.error("--lookahead values are none or integers >= 0")
    t0 = time.time()
    ctx = Context(0)
    be = pa.SequentialBackend(1)
    A, offs, xs = pa.generate_problem(be, a.kind, a.n)
    H = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=1000), device=ctx)
    del A
    S = AMGSolver(ctx, H, graph=True)
    Af = S.fine_operator()
    b = PVector(ctx, Af.nrows)
    mul(b, Af, PVector(ctx, Af.n_own_cols, Af.n_ghost, xs[0]))
    print(f"# setup + upload {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    if a.sweep_cost:
        from parallel_amg_amd.partitioned import block_jacobi, jacobi
        S.set_block_size(a.block_size)
        A0, om = S.A_dev[0], S.omega[0]
        x, tmp = A0.new_input_vector(), A0.new_input_vector()
        for r in range(-1, a.rounds):  # (-1: warm-up)
            for name, fn in (("jacobi", jacobi), ("block_jacobi", block_jacobi)):
                x.fill(0.0)
                ctx.sync()
                ts = time.perf_counter()
                fn(x, A0, b, tmp, om, a.sweep_cost)
                dt = time.perf_counter() - ts
                if r >= 0:
                    print(json.dumps({"kind": a.kind, "n": a.n, "rows": A0.nrows, "nnz": A0.nnz, "sweep": name,
                                      "block_size": a.block_size, "round": r, "sweeps": a.sweep_cost,
                                      "ms_per_sweep": round(dt * 1e3 / a.sweep_cost, 5)}), flush=True)
        return
    if a.pcg:
        est = {}
        for full in a.pcg.split(","):
            blk, var = full.startswith("b"), full[1:] if full.startswith("b") else full
            if len(var) not in (3, 4) or var[0] not in "jc" or var[3:] not in ("", "e"):
                ap.error(f"bad --pcg variant {full!r}")
            if blk and not S.block_size:
                S.set_block_size(a.block_size)
            if var.endswith("e") and blk not in est:
                est[blk] = estimate_timed(ctx, S, a, block=blk)
            S.set_smoother(("block_" if blk else "") + {"j": "jacobi", "c": "chebyshev"}[var[0]], ratio=a.ratio,
                           lmax=est[blk] if var.endswith("e") else "gershgorin")
            S.set_sweeps(int(var[1]), int(var[2]))
            var = full
            if a.lookahead is None:
                for r in range(-1, a.rounds):  # (-1: warm-up and graph capture)
                    x = S.new_vector()
                    ctx.sync()
                    ts = time.perf_counter()
                    its, hist = S.pcg(x, b, a.rtol, a.maxit)
                    dt = time.perf_counter() - ts
                    if r >= 0:
                        print(json.dumps({"kind": a.kind, "n": a.n, "variant": var, "round": r, "iterations": its,
                                          "ms": round(dt * 1e3, 3), "rel_residual": float(hist[-1] / hist[0])}), flush=True)
                continue
            # --lookahead: the entry points round by round (none, 0, 1, ..., none, 0, 1, ...), every
            # solve into the same zeroed x, so that the resident graphs (keyed on x) are captured in
            # the warm-up round only
            x = S.new_vector()
            ref = None
            for r in range(-1, a.rounds):
                for la in looks:
                    x.fill(0.0)
                    ctx.sync()
                    ts = time.perf_counter()
                    its, hist = S.pcg(x, b, a.rtol, a.maxit, lookahead=la)
                    dt = time.perf_counter() - ts
                    # (x is compared too unless downloading it would dwarf the solve)
                    bits = (its, hist.tobytes(), x.own_values().tobytes() if Af.nrows <= 1 << 24 else None)
                    ref = ref or bits
                    if r >= 0:
                        print(json.dumps({"kind": a.kind, "n": a.n, "variant": var, "lookahead": "none" if la is None else la,
                                          "round": r, "iterations": its, "ms": round(dt * 1e3, 3),
                                          "rel_residual": float(hist[-1] / hist[0]), "stats": S.last_pcg_stats,
                                          "same_bits_as_first": bits == ref}), flush=True)
        return
    key, vals = a.ab.split("=")
    va, vb = (int(v) for v in vals.split(","))
    ref = None
    for r in range(a.rounds):
        for v in (va, vb):
            set_opt(key, v)
            S.set_graph(False)
            S.set_graph(True)
            x = S.new_vector()
            S.vcycle(x, b, 3)  # warm-up + capture
            x = S.new_vector()
            ctx.sync()
            ts = time.perf_counter()
            S.vcycle_async(x, b, a.steps)
            ctx.sync()
            dt = time.perf_counter() - ts
            bits = x.own_values().view(np.int64)
            same = None if ref is None else bool(np.array_equal(bits, ref))
            if ref is None:
                ref = bits.copy()
            print(json.dumps({key: v, "round": r, "ms_per_cycle": round(dt / a.steps * 1e3, 4),
                              "vcycles_per_s": round(a.steps / dt, 2), "same_bits_as_first": same}), flush=True)
    set_opt(key, va)


if __name__ == "__main__":
    main()
