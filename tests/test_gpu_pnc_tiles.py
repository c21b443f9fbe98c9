"""k_rows_pnct — the neighbour-coded prolongation marched over 64 x 4 tiles of a plane, the in-plane
neighbours' anchors staged in LDS and the gathers trimmed to the wave's longest row (option
``pnc`` = 1) — against k_rows_pnc, the line-block march (``pnc`` = 2), and the oracle: the same bits
on the smallest grids where the tiled march can go wrong.

A grid registers on the context only where nx % 64 == 0 and ny % 16 == 0 (the blocked level-0
layout's tile, kTbX x kTbY), so every neighbour-coded prolongation cuts into whole 64 x 4 (and
32 x 8) tiles: (96, 16, 4), the shape meant to send ``pnc`` = 1 to the line-block march, never takes
the layout, and no registered grid can. The case stays, asserting what such a grid does: no
neighbour coding, the tile layouts, the oracle's bits. ``launch_pnc`` keeps the line-block branch
for ``pnc`` = 2 and for a grid a later registration rule might admit."""
import ctypes

import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd._lib import call, layout_of, option
from parallel_amg_amd.hcsr import HCSR
from parallel_amg_amd.partitioned import LocalWorld, PSparseMatrix, PVector, mul, residual
from parallel_amg_amd.solver import AMGSolver

from test_gpu_parity import _grid_hierarchy_P0, _layout_ops_match_oracle, bits, upload

pytestmark = pytest.mark.gpu


def pnc_grid(shape):
    """k_rows_pnct's / k_rows_pnc's grid: a workgroup per 256 points of a plane and 32-plane chunk,
    rounded up to the 8 XCDs."""
    nx, ny, nz = shape
    zlen = min(32, nz)
    return (nx * ny // 256 * ((nz + zlen - 1) // zlen) + 7) // 8 * 8


def check_both_marches(ctx, shape, A0, P, seed):
    """P over the grid of A0: under both record forms the upload takes the layout, and SpMV, residual
    and prolongate-add under pnc = 1 and pnc = 2 are the oracle's bits (computed once)."""
    Ad = PSparseMatrix(ctx, A0)
    assert layout_of(Ad)["jr_fused"], layout_of(Ad)  # (the grid is registered on the context)
    rng = np.random.default_rng(seed)
    nr, nc = P.nrows, P.ncols
    xh, bh = rng.standard_normal(nc), rng.standard_normal(nr)
    ref = O.spmv(P, xh)
    # (pamg_bench_rowop runs the op once to warm up and once timed: y += P x twice)
    want = {"spmv": ref, "residual": O.residual(P, xh, bh), "prolong": (bh + ref) + ref}
    x, b = PVector(ctx, nc, 0, xh), PVector(ctx, nr, 0, bh)
    compact = []
    for cp in (0, 1):
        with option("pnc_compact", cp):
            D, _h = upload(ctx, P)
        lay = layout_of(D)
        assert lay["pnc"] and lay["pnc_tiled"] and lay["tiles"] == pnc_grid(shape), (cp, lay)
        assert not (cp == 0 and lay["pnc_compact"]), lay
        compact.append(lay["pnc_compact"])
        for pnc in (1, 2):
            with option("pnc", pnc):
                y = PVector(ctx, nr)
                mul(y, D, x)
                r = PVector(ctx, nr)
                residual(r, D, x, b)
                yy, ms = PVector(ctx, nr, 0, bh), ctypes.c_double()
                call("pamg_bench_rowop", ctx.handle, D.handle, 3, x.handle, None, yy.handle, 0.0, 1, ctypes.byref(ms))
            got = {"spmv": y.own_values(), "residual": r.own_values(), "prolong": yy.own_values()}
            for op, w in want.items():
                bad = np.flatnonzero(bits(got[op]) != bits(w))
                assert bad.size == 0, (shape, cp, pnc, op, bad.size, bad[:8].tolist())
        del D
    del Ad
    return compact


# what each shape exercises:
#   (64, 16, 2), (64, 16, 3)     fewer planes than two full streams: an empty or one-plane stream
#   (64, 16, 33), (64, 16, 65)   z neighbours across one and two 32-plane unit boundaries
#   (128, 16, 5), (192, 16, 4)   interior x tile edges (ring from the neighbour tile), both x faces
#   (64, 32, 34)                 interior y tile edges
SHAPES = [(64, 16, 2), (64, 16, 3), (64, 16, 33), (64, 16, 65), (128, 16, 5), (192, 16, 4), (64, 32, 34)]


@pytest.mark.parametrize("shape", SHAPES)
def test_tiled_march_bit_exact(ctx, shape):
    """The level-0 prolongation of the shape's SA hierarchy, uploaded after its grid operator: the
    layout, the reported grid, and the oracle's bits from both marches and both record forms."""
    A0, P = _grid_hierarchy_P0(*shape)
    check_both_marches(ctx, shape, A0, P, sum(shape))


def test_untiled_grid_keeps_tile_layouts(ctx):
    """(96, 16, 4): nx is no multiple of 64, so the grid never registers and the prolongation stays
    in the tile layouts under pnc = 1 (module docstring) — still the oracle's bits."""
    A0, P = _grid_hierarchy_P0(96, 16, 4)
    Ad = PSparseMatrix(ctx, A0)
    assert not layout_of(Ad)["jr_fused"], layout_of(Ad)
    D = _layout_ops_match_oracle(ctx, P, np.random.default_rng(116))
    lay = layout_of(D)
    assert not lay["pnc"] and not lay["pnc_tiled"] and lay["tiles"] > 0, lay
    del Ad


def synthetic_rows(shape, seed):
    """A neighbour-coded matrix made by hand over the grid: the anchor of point (x, y, z) is column
    (x + 3 y + 9 z) mod 27 — so a point's 7 stencil points have 7 distinct anchors — with the value
    1.0, the row's largest; each row adds one of 8 subsets of its in-grid neighbours' anchors (rows
    of 1 .. 7 entries; values from a palette of 12 below 1), columns sorted. Every 64-point piece of
    a line (a wave) draws a cap on its rows' subsets, so the waves' longest rows take every value
    from 1 to 7. 27 columns < rows: a prolongation. At most 8 subsets x 27 column orders = 216
    patterns and as many (pattern, values) combinations: both record forms."""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    pal = np.array([0.5, -0.25, 0.125, 0.75, -0.625, 0.3, 0.1, -0.7, 0.2, 0.9, -0.05, 0.45])
    subsets = [(), (2,), (0, 1), (4, 5), (0, 2, 4), (0, 1, 2, 3), (0, 1, 2, 3, 4), (0, 1, 2, 3, 4, 5)]  # by length
    n = nx * ny * nz
    cap = np.repeat(rng.integers(0, len(subsets), n // 64), 64)
    pick = np.minimum(rng.integers(0, len(subsets), n), cap)
    d = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    rp, ci, va = [0], [], []
    for i in range(n):
        x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
        ent = {(x + 3 * y + 9 * z) % 27: 1.0}
        for e in subsets[pick[i]]:
            xx, yy, zz = x + d[e][0], y + d[e][1], z + d[e][2]
            if 0 <= xx < nx and 0 <= yy < ny and 0 <= zz < nz:
                ent[(xx + 3 * yy + 9 * zz) % 27] = pal[(2 * pick[i] + e) % len(pal)]
        for c in sorted(ent):
            ci.append(c)
            va.append(ent[c])
        rp.append(len(ci))
    return O.CSR(np.array(rp, np.int64), np.array(ci, np.int64), np.array(va), 27)


def step_longest_rows(shape, ln):
    """The longest row of every wave and step of the tiled march: a wave is 64 consecutive points of
    a line; a step takes one plane of each of the two z-streams of a 32-plane unit."""
    nx, ny, nz = shape
    wave = ln.reshape(nz, -1, 64).max(axis=2)  # (plane, wave of the plane)
    out = []
    for z0 in range(0, nz, 32):
        z1 = min(nz, z0 + 32)
        part = (z1 - z0 + 1) // 2
        for j in range(part):
            za, zb = z0 + j, z0 + part + j
            out.append(np.maximum(wave[za], wave[zb]) if zb < z1 else wave[za])
    return np.concatenate(out)


def test_gather_trimming_every_body(ctx):
    """Rows of 7 entries are out of reach of these grids' SA hierarchies (no aggregate is one point
    wide in x, y and z at once), but not of build_pnc: the hand-made rows of ``synthetic_rows`` take
    the layout, every row length 1 .. 7 occurs, and the steps' longest rows — what picks the gather
    body — are 7, 6, 5, 4, and 3 or less (the 3-body with lanes of 1 and 2 entries); both marches
    give the oracle's bits; two tiles in x, four in y, two z units."""
    shape = (128, 16, 34)
    M = O.generate("poisson3d", *shape)
    A0 = HCSR.from_arrays(M.rowptr, M.col.astype(np.int32), M.val, M.nrows)
    P = synthetic_rows(shape, 9)
    ln = np.diff(P.rowptr)
    assert set(ln.tolist()) == set(range(1, 8)), np.bincount(ln)
    steps = step_longest_rows(shape, ln)
    assert set(steps.tolist()) == set(range(1, 8)), np.bincount(steps)
    compact = check_both_marches(ctx, shape, A0, P, 5)
    assert compact == [False, True], compact


def test_two_parts_interior_rows_tiled(built):
    """Two z-slabs of the 64^3 Poisson grid in the in-process device world: each part's level-0
    prolongation runs its interior rows in the tiled march (the boundary rows — ghost columns —
    carry the skip id, stay in tiles and are stored by no lane of k_rows_pnct); ghosts NaN-poisoned
    before every exchange. b = A x* and x after 2 V-cycles are the oracle's two-part bits under
    pnc = 1 and, on the same uploads, pnc = 2."""
    nparts, n, ncycles = 2, 64, 2
    got = {}
    with option("poison_ghosts", 1):
        W = LocalWorld(nparts)
        try:
            be = pa.SequentialBackend(nparts)
            A, offs, xs = pa.generate_problem(be, "poisson3d", n)
            H = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=1000, agglomerate=0), device=W.ctxs[0])
            S = [AMGSolver(W.ctxs[p], H, part=p) for p in range(nparts)]
            lays = [layout_of(s.P[0]) for s in S]
            assert all(la["pnc"] and la["pnc_tiled"] for la in lays), lays
            # (a part's boundary rows: its second set holds them)
            assert all(layout_of(s.P[0], 1)["tiles"] > 0 for s in S), [layout_of(s.P[0], 1) for s in S]
            A0 = [s.A[0] for s in S]
            xst = [PVector(W.ctxs[p], A0[p].n_own_cols, A0[p].n_ghost, xs[p]) for p in range(nparts)]
            b = [PVector(W.ctxs[p], A0[p].nrows) for p in range(nparts)]
            W.run(lambda p: mul(b[p], A0[p], xst[p]))
            got_b = np.concatenate([v.own_values() for v in b])
            for pnc in (1, 2):
                with option("pnc", pnc):
                    x = [s.new_vector() for s in S]
                    W.run(lambda p: S[p].vcycle(x[p], b[p], ncycles))
                    got[pnc] = np.concatenate([v.own_values() for v in x])
        finally:
            del S
            W.close()
    Ao = O.generate("poisson3d", n, n, n)
    bo = O.spmv(Ao, O.xstar(Ao.nrows))
    Ho = O.setup(Ao, nparts=nparts, max_coarse=1000, agglomerate=0)
    xo = Ho.solve(bo, ncycles)
    assert np.array_equal(bits(got_b), bits(bo))
    for pnc in (1, 2):
        assert np.array_equal(bits(got[pnc]), bits(xo)), pnc
