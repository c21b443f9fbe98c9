"""k_rows_pncv — the tiled march of the neighbour-coded prolongation with the coarse values
E(p) = x[anc[p]] staged in the tile's LDS plane (option ``pnc`` = 1) — beside k_rows_pnct, the same
march with the anchors staged (``pnc`` = 3), against the oracle: the same bits from SpMV, residual
and prolongate-add, under both record forms (``pnc_compact`` 0 and 1), on the smallest grids where
the march can go wrong. Every case asserts that the upload took the layout and that the grid cuts
into tiles, so a decline to another kernel cannot pass.

A 7-point grid registers on the context where it cuts into the march's 64 x 4 tiles (one plane of
it, a 5-point stencil, too), so the one-tile grids below take the layout."""
import ctypes

import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd import hierarchy as HH
from parallel_amg_amd._lib import call, layout_of, option
from parallel_amg_amd.partitioned import LocalWorld, PSparseMatrix, PVector, mul, residual
from parallel_amg_amd.solver import AMGSolver

from test_gpu_parity import _grid_hierarchy_P0, bits, upload
from test_gpu_pnc_tiles import synthetic_rows

pytestmark = pytest.mark.gpu

MODES = (1, 3)  # the values-staged and the anchors-staged tiled march


def run_ops(ctx, D, x, b, bh):
    """SpMV, residual and prolongate-add (pamg_bench_rowop runs the op once to warm up and once
    timed: y += P x twice) of the uploaded prolongation."""
    nr = D.nrows
    y = PVector(ctx, nr)
    mul(y, D, x)
    r = PVector(ctx, nr)
    residual(r, D, x, b)
    yy, ms = PVector(ctx, nr, 0, bh), ctypes.c_double()
    call("pamg_bench_rowop", ctx.handle, D.handle, 3, x.handle, None, yy.handle, 0.0, 1, ctypes.byref(ms))
    return {"spmv": y.own_values(), "residual": r.own_values(), "prolong": yy.own_values()}


def check_marches(ctx, shape, A0, P, seed):
    """P over the grid of A0: under both record forms the upload takes the layout, and the three ops
    under pnc = 1 and pnc = 3 are the oracle's bits (computed once)."""
    Ad = PSparseMatrix(ctx, A0)  # (registers the grid on the context)
    rng = np.random.default_rng(seed)
    nr, nc = P.nrows, P.ncols
    xh, bh = rng.standard_normal(nc), rng.standard_normal(nr)
    ref = O.spmv(P, xh)
    want = {"spmv": ref, "residual": O.residual(P, xh, bh), "prolong": (bh + ref) + ref}
    x, b = PVector(ctx, nc, 0, xh), PVector(ctx, nr, 0, bh)
    for cp in (0, 1):
        with option("pnc_compact", cp):
            D, _h = upload(ctx, P)
        lay = layout_of(D)
        assert lay["pnc"] and lay["pnc_tiled"], (shape, cp, lay)
        assert not (cp == 0 and lay["pnc_compact"]), lay
        for pnc in MODES:
            with option("pnc", pnc):
                got = run_ops(ctx, D, x, b, bh)
            for op, w in want.items():
                bad = np.flatnonzero(bits(got[op]) != bits(w))
                assert bad.size == 0, (shape, cp, pnc, op, bad.size, bad[:8].tolist())
        del D
    del Ad


# what each shape exercises:
#   (64, 4, 1), (64, 4, 2)   one tile, every ring point off the grid, fewer planes than streams
#   (64, 4, 3)               uneven streams
#   (128, 4, 4)              a left / right ring between two tiles
#   (64, 8, 5)               a below / above ring between two tiles
SMALL = [(64, 4, 1), (64, 4, 2), (64, 4, 3), (128, 4, 4), (64, 8, 5)]
# unit boundaries in z: the last unit shorter than 32 planes; a unit's first plane takes E of the
# plane below, inside another unit's range, and its last plane the plane above
UNITS = [(64, 4, 33), (64, 4, 70), (128, 8, 65)]


@pytest.mark.parametrize("shape", SMALL)
def test_smallest_tiles_and_z_clamps(ctx, shape):
    """(64, 4, 1): the SA prolongation of the one-plane grid (44 columns) is not neighbour-coded —
    in two of its rows the largest value is tied, the anchor is the first of the two columns, and
    the other column is then no neighbour's anchor, so build_pnc declines it. The case keeps its
    grid with the hand-made neighbour-coded rows of test_gpu_pnc_tiles (rows of 1 .. 5 entries
    there: no z neighbours), which the layout takes."""
    A0, P = _grid_hierarchy_P0(*shape)
    assert P.ncols < P.nrows, (shape, P.nrows, P.ncols)  # (max_coarse = 100 < 256 points: a second level)
    if shape == (64, 4, 1):
        P = synthetic_rows(shape, 3)
    check_marches(ctx, shape, A0, P, sum(shape))


@pytest.mark.parametrize("shape", UNITS)
def test_unit_boundaries_in_z(ctx, shape):
    A0, P = _grid_hierarchy_P0(*shape)
    check_marches(ctx, shape, A0, P, sum(shape))


@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_unused_coarse_entry_does_not_leak(ctx, poison):
    """(64, 16, 12) with one coarse entry c of the input NaN, then +Inf: a lane gathers E of every
    point of its tile and ring, used or not, so rows whose columns do not contain c must stay the
    oracle's bits and finite; rows that contain c are NaN (Inf: what the oracle gives)."""
    shape = (64, 16, 12)
    A0, P = _grid_hierarchy_P0(*shape)
    Ad = PSparseMatrix(ctx, A0)
    nr, nc = P.nrows, P.ncols
    c = nc // 2
    has = np.zeros(nr, bool)
    has[np.repeat(np.arange(nr), np.diff(P.rowptr))[P.col == c]] = True
    assert has.sum() > 0 and (~has).sum() > 0, (has.sum(), nr)
    rng = np.random.default_rng(92)
    xh, bh = rng.standard_normal(nc), rng.standard_normal(nr)
    xh[c] = poison
    with np.errstate(invalid="ignore"):
        ref = O.spmv(P, xh)
        want = {"spmv": ref, "residual": O.residual(P, xh, bh), "prolong": (bh + ref) + ref}
    x, b = PVector(ctx, nc, 0, xh), PVector(ctx, nr, 0, bh)
    for cp in (0, 1):
        with option("pnc_compact", cp):
            D, _h = upload(ctx, P)
        lay = layout_of(D)
        assert lay["pnc"] and lay["pnc_tiled"], (cp, lay)
        for pnc in MODES:
            with option("pnc", pnc):
                got = run_ops(ctx, D, x, b, bh)
            for op, w in want.items():
                g = got[op]
                assert np.isfinite(g[~has]).all(), (cp, pnc, op)
                assert np.array_equal(bits(g[~has]), bits(w[~has])), (cp, pnc, op)
                nan = np.isnan(w[has])
                if np.isnan(poison):
                    assert nan.all(), (cp, pnc, op)
                assert np.array_equal(np.isnan(g[has]), nan), (cp, pnc, op)
                assert np.array_equal(bits(g[has][~nan]), bits(w[has][~nan])), (cp, pnc, op)
        del D
    del Ad


def test_two_parts_ghost_anchors_never_summed(built):
    """Two z-slabs of the 64 x 8 x 12 Poisson grid in the in-process device world (host transport),
    ghosts NaN-poisoned before every exchange: each part's interior pass gathers E at boundary
    points whose anchor is a ghost slot before the exchange lands; no interior row names such a
    point, so b = A x* and x after 3 V-cycles are the oracle's two-part bits on every rank, under
    pnc = 1 and, on the same uploads, pnc = 3."""
    nparts, shape, ncycles = 2, (64, 8, 12), 3
    N = shape[0] * shape[1] * shape[2]
    offs = np.array([p * N // nparts for p in range(nparts + 1)], np.int64)
    got = {}
    with option("poison_ghosts", 1):
        W = LocalWorld(nparts)
        S = []
        try:
            be = pa.SequentialBackend(nparts)
            A = {p: HH.H.gen_grid(HH.KIND["poisson3d"], *shape, 1e-3, int(offs[p]), int(offs[p + 1])) for p in be.parts}
            xs = {p: HH.H.gen_xstar(int(offs[p]), int(offs[p + 1] - offs[p]), HH.SEED) for p in be.parts}
            H = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=100, agglomerate=0), device=W.ctxs[0])
            S = [AMGSolver(W.ctxs[p], H, part=p) for p in range(nparts)]
            lays = [layout_of(s.P[0]) for s in S]
            assert all(la["pnc"] and la["pnc_tiled"] for la in lays), lays
            A0 = [s.A[0] for s in S]
            xst = [PVector(W.ctxs[p], A0[p].n_own_cols, A0[p].n_ghost, xs[p]) for p in range(nparts)]
            b = [PVector(W.ctxs[p], A0[p].nrows) for p in range(nparts)]
            W.run(lambda p: mul(b[p], A0[p], xst[p]))
            got_b = [v.own_values() for v in b]
            for pnc in MODES:
                with option("pnc", pnc):
                    x = [s.new_vector() for s in S]
                    W.run(lambda p: S[p].vcycle(x[p], b[p], ncycles))
                    got[pnc] = [v.own_values() for v in x]
        finally:
            del S
            W.close()
    Ao = O.generate("poisson3d", *shape)
    bo = O.spmv(Ao, O.xstar(Ao.nrows))
    Ho = O.setup(Ao, nparts=nparts, max_coarse=100, agglomerate=0)
    xo = Ho.solve(bo, ncycles)
    for p in range(nparts):
        lo, hi = int(offs[p]), int(offs[p + 1])
        assert np.array_equal(bits(got_b[p]), bits(bo[lo:hi])), p
        for pnc in MODES:
            assert np.array_equal(bits(got[pnc][p]), bits(xo[lo:hi])), (pnc, p)
