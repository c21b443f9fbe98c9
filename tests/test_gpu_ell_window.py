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
    """SpMV, residual and prolongate-add (and `sweeps` Jacobi sweeps) of every matrix in mats: the
    oracle's bits."""
    rng = np.random.default_rng(seed)
    xh, bh = rng.standard_normal(M.nrows), rng.standard_normal(M.nrows)
    s = O.spmv(M, xh)
    want_y, want_r = bits(s), bits(O.residual(M, xh, bh))
    want_p = bits((bh + s) + s)  # y <- y + A x from y = b, twice (pamg_bench_rowop: warm-up + 1 timed)
    want_x = xh
    for _ in range(sweeps):
        want_x = O.jacobi(M, want_x, bh, omega)
    for D in mats:
        x, b, y = PVector(ctx, M.nrows, 0, xh), PVector(ctx, M.nrows, 0, bh), PVector(ctx, M.nrows)
        mul(y, D, x)
        assert np.array_equal(bits(y.own_values()), want_y)
        residual(y, D, x, b)
        assert np.array_equal(bits(y.own_values()), want_r)
        ms, yy = ctypes.c_double(), PVector(ctx, M.nrows, 0, bh)
        call("pamg_bench_rowop", ctx.handle, D.handle, 3, x.handle, None, yy.handle, 0.0, 1, ctypes.byref(ms))
        assert np.array_equal(bits(yy.own_values()), want_p)
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


# ---------------------------------------------------------------- the layout's limits, at small sizes
def long_rows(n=1064, no_diag=False):
    """Offsets -127 .. 126 with one value each (the diagonal 300): row i keeps those with
    |offset| <= (0, 6, 24, 48, 96, 127)[(i // 3) % 6] that fall inside the matrix — rows of 1, 13, 49,
    97, 193 and 254 entries. no_diag: every 17th row of >= 49 entries loses its diagonal."""
    offs = np.arange(-127, 127)
    pal = np.random.default_rng(41).standard_normal(254)
    pal[127] = 300.0
    h = np.array([0, 6, 24, 48, 96, 127])[(np.arange(n) // 3) % 6]
    i, k = np.meshgrid(np.arange(n), np.arange(254), indexing="ij")
    c = i + offs[k]
    keep = (np.abs(offs[k]) <= h[i]) & (c >= 0) & (c < n)
    if no_diag:
        keep[np.flatnonzero(keep.sum(axis=1) >= 49)[::17], 127] = False
    return from_coo(i[keep], c[keep], pal[k[keep]], n)


def test_long_rows(ctx):
    """Rows of up to 254 nonzeros (64 index dwords: the 12 preloaded ones and five reloaded batches,
    the last of them past the slice's end), the diagonal of the longest rows at entry 127."""
    M = long_rows()
    assert M.nrows == 16 * 64 + 40
    L = np.diff(M.rowptr)
    assert sorted(set(L[200:800].tolist())) == [1, 13, 49, 97, 193, 254]
    full = np.flatnonzero(L == 254)
    assert len(full) > 100 and np.array_equal(M.col[M.rowptr[full] + 127], full)  # (dpos 127 >= 48)
    A, B, _h = upload_pair(ctx, M)
    lay = layout_of(A)
    assert lay["ell"] and lay["ell_pair"] and lay["ell_xwin"], lay
    assert lay["ell_gather_groups"] == 0 and lay["ell_xwin_max_pairs"] == 254, lay
    check_ops(ctx, M, (A, B), 2)


def test_long_rows_without_diagonal(ctx):
    """The same rows, some of the long ones without a diagonal (dpos 255): no Jacobi (it would divide
    by zero), every other op on every row."""
    M = long_rows(no_diag=True)
    rows = np.repeat(np.arange(M.nrows), np.diff(M.rowptr))
    has = np.zeros(M.nrows, bool)
    has[rows[M.col == rows]] = True
    lost = np.flatnonzero(~has)
    assert len(lost) >= 20 and np.diff(M.rowptr)[lost].min() >= 48 and np.diff(M.rowptr)[lost].max() == 253
    A, B, _h = upload_pair(ctx, M)
    lay = layout_of(A)
    assert lay["ell"] and lay["ell_pair"] and lay["ell_xwin"], lay
    check_ops(ctx, M, (A, B), 0)


def many_chunks(n=40000):
    """The band {-32, -1, 0, 1, 32} and one far entry per row: in the first 60 % of the rows (a
    multiple of 256) lanes 2m and 2m + 1 of a slice take offset 300 (m + 1), in the others lane m does;
    negated where it would leave the matrix. One value per offset, the diagonal 9."""
    i = np.arange(n)
    lane = i % 64
    n1 = n * 6 // 10 // 256 * 256
    far = 300 * (np.where(i < n1, lane // 2, lane) + 1)
    far = np.where(i + far >= n, -far, far)
    assert (i + far).min() >= 0
    pal = np.random.default_rng(43).standard_normal(256)
    rows, cols, vals = [i], [i + far], [pal[far // 300 + 128]]
    for o, v in ((-32, -0.5), (-1, -1.0), (0, 9.0), (1, -1.25), (32, -0.75)):
        r = np.arange(max(0, -o), min(n, n - o))
        rows.append(r)
        cols.append(r + o)
        vals.append(np.full(len(r), v))
    return from_coo(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), n)


def test_many_chunks_and_chunk_limit(ctx):
    """Windows of ~130 runs of two columns (runs merge only within 16 columns; these lie 64 apart): a
    wave takes ~33 chunks, most of them one-lane loads. The groups of the second part hold 4 x 64 far
    runs + the band, over kEllWinChunks = 256, and gather in the same launch."""
    M = many_chunks()
    A, B, _h = upload_pair(ctx, M)
    lay = layout_of(A)
    assert lay["ell_xwin"], lay
    assert 100 <= lay["ell_xwin_max_chunks"] <= 256 and lay["ell_xwin_census"]["runs_max"] >= 100, lay
    assert lay["ell_gather_groups"] > 0 and lay["ell_xwin_groups"] >= lay["ell_gather_groups"], lay
    check_ops(ctx, M, (A, B), 2)


def pair_cap(nvals, nslices=24):
    """Offsets {-2 .. 2}; slice q has nvals (a multiple of 5) values of its own, the entry with offset
    k - 2 of lane l taking the (5 l + k) % nvals-th (+ 50 on the diagonal): nvals pairs per slice."""
    n = 64 * nslices
    base = np.random.default_rng(57).standard_normal((nslices, nvals))
    i, k = np.repeat(np.arange(n), 5), np.tile(np.arange(5), n)
    c = i + k - 2
    v = base[i // 64, (5 * (i % 64) + k) % nvals] + np.where(k == 2, 50.0, 0.0)
    keep = (c >= 0) & (c < n)
    return from_coo(i[keep], c[keep], v[keep], n)


@pytest.mark.parametrize("nvals,per_group", [(90, 2), (70, 3)])
def test_groups_closed_by_pair_cap(ctx, nvals, per_group):
    """Every group closes short of 4 slices at the 256-pair cap (90 pairs a slice: 2 slices, 70: 3):
    waves that own no rows, and the lof words of fewer than 4 waves. The consecutive 4-slice groups of
    ell_xwin 0 hold more than 256 values, so that upload is not ELL at all."""
    M = pair_cap(nvals)
    rows = np.repeat(np.arange(M.nrows), np.diff(M.rowptr))
    for q in (0, 7, 23):  # (offset, value) pairs of a slice
        e = rows // 64 == q
        assert len(set(zip((M.col - rows)[e].tolist(), M.val[e].tolist()))) == nvals
    h = HCSR.from_arrays(M.rowptr, M.col.astype(np.int32), M.val, M.ncols)
    with options(ell_min_rows=0, sym_dia=0):
        A = PSparseMatrix(ctx, h)
        with options(ell_xwin=0):
            B = PSparseMatrix(ctx, h)
    lay = layout_of(A)
    assert lay["ell_xwin"] and not layout_of(B)["ell_xwin"], (lay, layout_of(B))
    assert lay["ell_xwin_census"]["full_groups"] == 0, lay
    assert lay["ell_xwin_census"]["groups"] == 24 // per_group, lay
    assert 128 < lay["ell_xwin_max_pairs"] <= 256, lay
    check_ops(ctx, M, (A, B), 2)


def wide_blocks(n=256 * 40):
    """{-64, -1, 0, 1, 64} everywhere; the rows of the 256-row blocks 15, 25 and 35 also take the
    offsets -400 k, k = 1 .. 10 (where inside the matrix), and the diagonal 20."""
    i = np.arange(n)
    wide = np.isin(i // 256, (15, 25, 35))
    rows, cols, vals = [], [], []
    for o, v in ((-64, -0.5), (-1, -1.0), (0, 4.0), (1, -1.0), (64, -0.5)):
        r = np.arange(max(0, -o), min(n, n - o))
        rows.append(r)
        cols.append(r + o)
        vals.append(np.where(wide[r], 20.0, v) if o == 0 else np.full(len(r), v))
    for k in range(1, 11):
        r = i[wide & (i - 400 * k >= 0)]
        rows.append(r)
        cols.append(r - 400 * k)
        vals.append(np.full(len(r), 0.125 * k))
    return from_coo(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), n)


def test_occupancy_rule_sends_widest_groups_to_gathers(ctx):
    """Three groups whose windows (the band's run and ten 256-column runs 400 apart: more than 2048
    doubles, fewer than the default ell_xwin_max 7168) are the operator's largest: the upload lowers
    the largest window to what 8 workgroups per CU allow and those three gather."""
    M = wide_blocks()
    A, B, _h = upload_pair(ctx, M)
    # pamg_device.h: kEllLdsPerCu = 160 KB; a workgroup's LDS is its window + 2048 B of values + 2048 B
    # of lof words; 8 workgroups per CU: ((160 * 1024 / 8 - 2048) / 8 - 256) & ~1 doubles
    lds_per_cu = 160 * 1024
    fit8 = ((lds_per_cu // 8 - 2048) // 8 - 256) & ~1
    lay = layout_of(A)
    assert lay["ell_xwin"] and lay["ell_gather_groups"] == 3 and lay["ell_xwin_max_window"] <= fit8, lay
    check_ops(ctx, M, (A, B), 2)


def test_window_exactly_at_capacity(ctx):
    """ell_xwin_max equal to the largest window changes nothing; 2 doubles less and the groups of that
    window gather."""
    M = banded(1000)
    A, B, _h = upload_pair(ctx, M)
    la = layout_of(A)
    W = la["ell_xwin_max_window"]
    assert la["ell_xwin"] and W > 0, la
    A1, _B1, _h = upload_pair(ctx, M, ell_xwin_max=W)
    l1 = layout_of(A1)
    assert l1["ell_xwin"] and l1["ell_xwin_max_window"] == W, l1
    assert (l1["ell_xwin_groups"], l1["ell_gather_groups"]) == (la["ell_xwin_groups"], la["ell_gather_groups"]), l1
    A2, _B2, _h = upload_pair(ctx, M, ell_xwin_max=W - 2)
    l2 = layout_of(A2)
    assert l2["ell_xwin"] and l2["ell_xwin_max_window"] < W, l2
    assert l2["ell_gather_groups"] >= la["ell_gather_groups"] + 1, l2
    check_ops(ctx, M, (A, A1, A2, B), 2)


def test_windowed_level1_in_cycle(ctx):
    """poisson3d 32^3 with ell_min_rows 0: the level-1 operator (4192 rows) takes the windowed layout,
    groups closed by the pair cap among them, and runs inside the V-cycle — replayed from the graph
    and launched eagerly — and inside PCG: the oracle's bits and iteration count."""
    from parallel_amg_amd.solver import AMGSolver
    be = pa.SequentialBackend(1)
    Ah, offs, xs = pa.generate_problem(be, "poisson3d", 32)
    H = pa.build_hierarchy(be, Ah, offs, pa.SAParams(max_coarse=100), device=ctx)
    with options(ell_min_rows=0):
        S = AMGSolver(ctx, H)
    lay = layout_of(S.A[1])
    assert lay["ell_xwin"] and lay["ell_xwin_noncontig_groups"] >= 1, lay
    assert lay["ell_xwin_census"]["full_groups"] < lay["ell_xwin_census"]["groups"], lay
    b = PVector(ctx, S.A[0].nrows)
    mul(b, S.A[0], PVector(ctx, S.A[0].nrows, 0, xs[0]))
    Ao = O.generate("poisson3d", 32, 32, 32)
    bo = O.spmv(Ao, O.xstar(Ao.nrows))
    assert np.array_equal(bits(b.own_values()), bits(bo))
    Ho = O.setup(Ao, max_coarse=100)
    assert Ho.nlevels == H.nlevels
    xo, ho = Ho.solve(bo, 5, res_hist=True)
    _xp, ko, _hp = Ho.pcg(bo, 1e-10, 60)
    for graph in (True, False):
        S.set_graph(graph)
        x = S.new_vector()
        hist = S.vcycle(x, b, 5, res_hist=True)
        assert np.array_equal(bits(x.own_values()), bits(xo))
        np.testing.assert_allclose(hist, ho, rtol=1e-12)
        x = S.new_vector()
        k, _h = S.pcg(x, b, 1e-10, 60)
        assert k == ko
