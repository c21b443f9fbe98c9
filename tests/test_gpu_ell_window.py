"""The windowed sliced-ELL layout (ell_xwin; k_rows_ellw): groups of 4 coupled slices whose x
neighbourhood is staged in LDS. Every case is bit-exact against the oracle and against the same
matrix uploaded with ell_xwin 0 (k_rows_ell), and asserts through layout_of which path ran."""
import contextlib
import ctypes

import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd._lib import call, layout_of
from parallel_amg_amd.hcsr import HCSR
from parallel_amg_amd.partitioned import PSparseMatrix, PVector, jacobi, mul, residual

pytestmark = pytest.mark.gpu


def bits(a):
    return np.asarray(a, np.float64).view(np.int64)


@contextlib.contextmanager
def options(**opts):
    old = {}
    for k in opts:
        v = ctypes.c_int64()
        call("pamg_get_option", k.encode(), ctypes.byref(v))
        old[k] = v.value
    try:
        for k, v in opts.items():
            call("pamg_set_option", k.encode(), v)
        yield
    finally:
        for k, v in old.items():
            call("pamg_set_option", k.encode(), v)


def upload_pair(ctx, M, **opts):
    """M uploaded with the windowed layout allowed (plus opts) and with ell_xwin 0."""
    h = HCSR.from_arrays(M.rowptr, M.col.astype(np.int32), M.val, M.ncols)
    with options(ell_min_rows=0, sym_dia=0, **opts):
        A = PSparseMatrix(ctx, h)
        with options(ell_xwin=0):
            B = PSparseMatrix(ctx, h)
    lb = layout_of(B)
    assert lb["ell"] and not lb["ell_xwin"] and lb["ell_xwin_groups"] == 0, lb
    return A, B, h


def check_ops(ctx, M, mats, sweeps, seed=3, omega=0.57):
    """SpMV and residual (and `sweeps` Jacobi sweeps) of every matrix in mats: the oracle's bits."""
    rng = np.random.default_rng(seed)
    xh, bh = rng.standard_normal(M.nrows), rng.standard_normal(M.nrows)
    want_y, want_r = bits(O.spmv(M, xh)), bits(O.residual(M, xh, bh))
    want_x = xh
    for _ in range(sweeps):
        want_x = O.jacobi(M, want_x, bh, omega)
    for D in mats:
        x, b, y = PVector(ctx, M.nrows, 0, xh), PVector(ctx, M.nrows, 0, bh), PVector(ctx, M.nrows)
        mul(y, D, x)
        assert np.array_equal(bits(y.own_values()), want_y)
        residual(y, D, x, b)
        assert np.array_equal(bits(y.own_values()), want_r)
        if sweeps:
            t = PVector(ctx, M.nrows)
            jacobi(x, D, b, t, omega, sweeps)
            assert np.array_equal(bits(x.own_values()), bits(want_x))


def palette_grid(nx, ny, nz):
    """A 7-point grid with values redrawn from a 24-entry palette, diagonal 10."""
    M = O.generate("poisson3d", nx, ny, nz)
    pal = np.random.default_rng(9).standard_normal(24)
    val = pal[np.random.default_rng(10).integers(0, 24, M.nnz)]
    rows = np.repeat(np.arange(M.nrows), np.diff(M.rowptr))
    val[M.col == rows] = 10.0
    return O.CSR(M.rowptr.copy(), M.col.copy(), val, M.ncols)


def from_coo(rows, cols, vals, n):
    import scipy.sparse as sp
    T = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    T.sort_indices()
    return O.CSR(T.indptr.astype(np.int64), T.indices.astype(np.int64), T.data.copy(), n)


def ragged():
    """Empty and one-entry rows, columns within 60 of the row, clipped at both ends."""
    n = 3000
    rng = np.random.default_rng(4)
    rows, cols, vals = [], [], []
    for i in range(n):
        if i % 97 == 0:
            continue  # an empty row
        k = 1 if i % 13 == 0 else int(rng.integers(2, 40))
        cs = np.unique(np.clip(i + rng.integers(-60, 60, k), 0, n - 1))
        rows += [i] * len(cs)
        cols += cs.tolist()
        vals += (rng.integers(1, 9, len(cs)) * 0.25).tolist()
    return from_coo(rows, cols, vals, n)


def banded(n):
    """Offsets {-70, -1, 0, 1, 70}: rows 0 and n - 1 touch the first and the last column."""
    pal = np.random.default_rng(21).standard_normal(6)
    rows, cols, vals = [], [], []
    for k, o in enumerate((-70, -1, 0, 1, 70)):
        i = np.arange(max(0, -o), min(n, n - o))
        rows.append(i)
        cols.append(i + o)
        vals.append(np.full(len(i), 7.0) if o == 0 else pal[(i + k) % 6])
    return from_coo(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), n)


def test_regrouping_happens(ctx):
    """128 x 7 x 5 grid, 70 slices: a slice is half an x line, its y neighbours are 2 slices away and
    its z neighbours 14, so the coupled groups are not consecutive slices and the last one is short."""
    M = palette_grid(128, 7, 5)
    assert M.nrows == 70 * 64
    A, B, _h = upload_pair(ctx, M)
    lay = layout_of(A)
    assert lay["ell"] and lay["ell_pair"] and lay["ell_xwin"], lay
    assert lay["ell_gather_groups"] == 0 and lay["ell_xwin_noncontig_groups"] >= 1, lay
    assert lay["tiles"] >= 18, lay  # (70 slices: at least one short group)
    check_ops(ctx, M, (A, B), 2)


def test_partial_last_slice(ctx):
    """100 x 7 x 6: 65 full slices and one of 40 rows."""
    M = palette_grid(100, 7, 6)
    assert M.nrows == 65 * 64 + 40
    A, B, _h = upload_pair(ctx, M)
    lay = layout_of(A)
    assert lay["ell_xwin"] and lay["ell_gather_groups"] == 0, lay
    check_ops(ctx, M, (A, B), 2)


def test_ragged_rows(ctx, capsys):
    """Empty and one-entry rows, windows clipped at both ends. The upload takes the windowed layout
    only where the slices' pair tables fit; where they do not, the bits of the fallback are checked."""
    M = ragged()
    A, B, _h = upload_pair(ctx, M)
    lay = layout_of(A)
    assert lay["ell"], lay
    if lay["ell_xwin"]:
        assert lay["ell_xwin_groups"] > 0 and lay["ell_xwin_max_pairs"] <= 256, lay
    else:
        with capsys.disabled():
            print("\n  ragged: the windowed layout declined (pair tables), checking the fallback", end="")
    check_ops(ctx, M, (A, B), 0)


@pytest.mark.parametrize("n", [1000, 999])
def test_banded_clipped_window(ctx, n):
    """Offsets {-70, -1, 0, 1, 70}: the first group's window is clipped at column 0, the last one's at
    the last column (n odd: its last 16-byte load reaches one double into the vector's pad)."""
    M = banded(n)
    A, B, _h = upload_pair(ctx, M)
    lay = layout_of(A)
    assert lay["ell_xwin"] and lay["ell_gather_groups"] == 0 and lay["ell_xwin_groups"] >= 4, lay
    check_ops(ctx, M, (A, B), 2)


def test_both_paths_in_one_launch(ctx):
    """Two 2048-row diagonal blocks: a tridiagonal one (windows of ~260 columns) and one whose rows
    take the diagonal and 20 of 40 fixed offsets within +-3000 (entries outside the block dropped;
    4 values), whose windows span the block. With ell_xwin_max 1024 the first block's groups are
    windowed and the second block's gather, in one launch."""
    h = 2048
    rng = np.random.default_rng(31)
    offs = np.unique(rng.integers(-3000, 3001, 60))
    offs = offs[offs != 0][:40]
    pal = np.array([0.5, -1.25, 2.0, -0.75])
    rows, cols, vals = [], [], []
    for i in range(h):
        for o in (-1, 0, 1):
            if 0 <= i + o < h:
                rows.append(i)
                cols.append(i + o)
                vals.append(4.0 if o == 0 else -1.0)
    for i in range(h, 2 * h):
        rows.append(i)
        cols.append(i)
        vals.append(9.0)
        for o in rng.choice(offs, 20, replace=False):
            if h <= i + o < 2 * h:
                rows.append(i)
                cols.append(i + int(o))
                vals.append(pal[int(rng.integers(0, 4))])
    M = from_coo(rows, cols, vals, 2 * h)
    A, B, _h = upload_pair(ctx, M, ell_xwin_max=1024)
    lay = layout_of(A)
    assert lay["ell_xwin"] and lay["ell_xwin_groups"] > 0 and lay["ell_gather_groups"] > 0, lay
    assert lay["ell_xwin_max_window"] <= 1024, lay
    check_ops(ctx, M, (A, B), 2)


@pytest.fixture(scope="module")
def level1_128():
    be = pa.SequentialBackend(1)
    A, offs, _xs = pa.generate_problem(be, "poisson3d", 128)
    return be, A, offs


def test_pair_cap_level1_operator_128(ctx, level1_128):
    """The 128^3 hierarchy's A1: the capped greedy keeps every group within 256 pairs (59 of 1032
    plain greedy groups exceed them) and the windows within the census (2105 + run alignment)."""
    be, A, offs = level1_128
    H = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=1000), device=ctx)
    M1 = H.levels[1][0].A
    with options(ell_min_rows=0, sym_dia=0):
        D = PSparseMatrix(ctx, M1)
        with options(ell_xwin=0):
            D0 = PSparseMatrix(ctx, M1)
    lay = layout_of(D)
    assert lay["ell"] and lay["ell_pair"] and lay["ell_xwin"], lay
    assert 0 < lay["ell_xwin_max_pairs"] <= 256 and lay["ell_xwin_max_window"] <= 2500, lay
    # (the few largest windows may gather: the upload lowers the largest window for occupancy)
    assert lay["ell_xwin_groups"] * 100 >= 85 * (lay["ell_xwin_groups"] + lay["ell_gather_groups"]), lay
    assert not layout_of(D0)["ell_xwin"]
    Mo = O.CSR(M1.rowptr.copy(), M1.col.astype(np.int64), M1.val.copy(), M1.ncols)
    rng = np.random.default_rng(8)
    xh, bh = rng.standard_normal(M1.nrows), rng.standard_normal(M1.nrows)
    want_r, want_x = bits(O.residual(Mo, xh, bh)), bits(O.jacobi(Mo, xh, bh, 0.61))
    for E in (D, D0):
        x, b, y = PVector(ctx, M1.nrows, 0, xh), PVector(ctx, M1.nrows, 0, bh), PVector(ctx, M1.nrows)
        residual(y, E, x, b)
        assert np.array_equal(bits(y.own_values()), want_r)
        t = PVector(ctx, M1.nrows)
        jacobi(x, E, b, t, 0.61, 1)
        assert np.array_equal(bits(x.own_values()), want_x)


def test_off_switch_and_decline(ctx):
    """ell_xwin 0: k_rows_ell (checked in every upload_pair). Operators that miss the acceptance
    thresholds — no group's window fits ell_xwin_max 64 — keep k_rows_ell too, bit-exact."""
    for M, sweeps in ((ragged(), 0), (banded(1000), 1)):
        A, B, _h = upload_pair(ctx, M, ell_xwin_max=64)
        lay = layout_of(A)
        assert lay["ell"] and not lay["ell_xwin"] and lay["ell_xwin_groups"] == 0, lay
        check_ops(ctx, M, (A, B), sweeps)
