"""Row classes of the windowed sliced ELL (ell_xwin 1; k_rows_ellw<OP, true>): every slice stores its
distinct rows once, class-interleaved, and a class byte per row. Every case uploads the matrix with
ell_xwin 1 (classes allowed) and with ell_xwin 2 (never), asserts through layout_of which form each upload took, and compares
SpMV, residual, prolongate-add, Jacobi sweeps and the Chebyshev smoother of both with the oracle, bit
for bit (so with each other).

Not covered here: an x vector that is not 16-byte aligned (no entry point hands the kernel one: every
vector is its own device allocation); the branch it takes is the gather group's, which is. k_rows_ell
(ell_xwin 0, several parts) keeps the per-row stream, so there is no two-part case."""
import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd._lib import layout_of
from parallel_amg_amd.hcsr import HCSR
from parallel_amg_amd.partitioned import PSparseMatrix, PVector, chebyshev, mul
from test_gpu_chebyshev import cheb_ref, coeffs_ref, diag_of
from test_gpu_ell_window import bits, check_ops, from_coo, options, palette_grid

pytestmark = pytest.mark.gpu

LMAX, RATIO, DEG = 2.3, 4.0, 3


def upload_both(ctx, M, classed, **opts):
    """M in the windowed layout with ell_xwin 1 (the class form taken: `classed`) and with ell_xwin 2."""
    h = HCSR.from_arrays(M.rowptr, M.col.astype(np.int32), M.val, M.ncols)
    with options(ell_min_rows=0, sym_dia=0, **opts):
        A = PSparseMatrix(ctx, h)
        with options(ell_xwin=2):
            B = PSparseMatrix(ctx, h)
    la, lb = layout_of(A), layout_of(B)
    assert la["ell"] and la["ell_pair"] and la["ell_xwin"], la
    assert lb["ell_xwin"] and not lb["ell_class"] and lb["ell_class_census"]["slices"] == 0, lb
    assert la["ell_class"] == classed, la
    c = la["ell_class_census"]
    if classed:  # the half-bytes rule, and the stream bytes count the records in place of the stream
        assert c["slices"] == (M.nrows + 63) // 64 and 1 <= c["classes_mean"] <= c["classes_max"] <= 64, la
        assert 2 * (c["record_bytes"] + c["id_bytes"]) <= c["replaced_bytes"], la
        assert B.stream_bytes - A.stream_bytes == c["replaced_bytes"] - c["record_bytes"] - c["id_bytes"], la
    else:
        assert c["slices"] == 0 and A.stream_bytes == B.stream_bytes, la
    for k in la:  # the windows are the same upload's
        if k.startswith("ell_xwin") or k == "ell_gather_groups":
            assert la[k] == lb[k], (k, la, lb)
    return A, B, la


def check_all(ctx, M, mats, sweeps):
    """check_ops, and where every row has a diagonal the degree-3 Chebyshev smoother."""
    check_ops(ctx, M, mats, sweeps)
    if not sweeps:
        return
    rng = np.random.default_rng(5)
    xh, bh = rng.standard_normal(M.nrows), rng.standard_normal(M.nrows)
    c1, c2 = coeffs_ref(LMAX, RATIO, DEG)
    want = bits(cheb_ref(M, diag_of(M), xh, bh, c1, c2, DEG))
    for D in mats:
        x, b = D.new_input_vector(), PVector(ctx, M.nrows, 0, bh)
        x.set(xh)
        t1, t2 = D.new_input_vector(), D.new_input_vector()
        chebyshev(x, D, b, t1, t2, lmax=LMAX, ratio=RATIO, degree=DEG)
        assert np.array_equal(bits(x.own_values()), want)


def band(n, offsets=(-70, -1, 0, 1, 70), values=(-0.5, -1.25, 7.0, -1.0, -0.75)):
    """One value per offset: the rows away from the ends are identical."""
    rows, cols, vals = [], [], []
    for o, v in zip(offsets, values):
        i = np.arange(max(0, -o), min(n, n - o))
        rows.append(i)
        cols.append(i + o)
        vals.append(np.full(len(i), v))
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)


def test_one_class_per_slice(ctx):
    """n = 512: the slices of rows 128 .. 383 hold one class each, the others the clipped rows' too."""
    M = from_coo(*band(512), 512)
    A, B, lay = upload_both(ctx, M, True)
    c = lay["ell_class_census"]
    assert c["classes_max"] <= 3 and c["record_bytes"] <= 8 * 3 * 8, lay
    check_all(ctx, M, (A, B), 2)


def test_every_row_its_own_class_declines(ctx):
    """Values drawn per entry: (nearly) every row of a slice is a class of its own, the records would
    be as large as the stream, and the upload keeps the per-row stream."""
    M = palette_grid(128, 7, 5)
    A, B, _lay = upload_both(ctx, M, False)
    check_all(ctx, M, (A, B), 1)


def test_mixed_slices(ctx):
    """16 slices of the band; the rows of slice 5 each take their own value at offset 1: 64 classes in
    that slice, one or two in the others, and the operator still passes the half-bytes rule."""
    n = 1024
    r, c, v = band(n)
    e = (r // 64 == 5) & (c - r == 1)
    v[e] = -1.0 - 0.015625 * (r[e] % 64 + 1)
    M = from_coo(r, c, v, n)
    A, B, lay = upload_both(ctx, M, True)
    assert lay["ell_class_census"]["classes_max"] == 64, lay
    check_all(ctx, M, (A, B), 2)


def test_prefix_rows_are_different_classes(ctx):
    """Offsets -2 .. 6, one value each; row i keeps the first 7, 8 or 9 of them (i % 3): rows equal
    over their first entries and of different lengths, two index dwords or three."""
    n = 640
    offs = np.arange(-2, 7)
    val = np.array([-0.5, -0.25, 9.0, -1.0, -0.75, 0.125, 0.375, -0.625, 0.875])
    i, k = np.meshgrid(np.arange(n), np.arange(9), indexing="ij")
    keep = (k < 7 + i % 3) & (i + offs[k] >= 0) & (i + offs[k] < n)
    M = from_coo(i[keep], (i + offs[k])[keep], val[k[keep]], n)
    assert sorted(set(np.diff(M.rowptr)[64:512].tolist())) == [7, 8, 9]
    A, B, lay = upload_both(ctx, M, True)
    assert lay["ell_class_census"]["classes_mean"] >= 3, lay
    check_all(ctx, M, (A, B), 2)


def test_rows_without_diagonal(ctx):
    """The band with every fifth row's diagonal dropped (dpos 255): no Jacobi, every other op."""
    n = 768
    r, c, v = band(n)
    keep = ~((r == c) & (r % 5 == 2))
    M = from_coo(r[keep], c[keep], v[keep], n)
    A, B, lay = upload_both(ctx, M, True)
    assert lay["ell_class_census"]["classes_mean"] >= 2, lay
    check_all(ctx, M, (A, B), 0)


def ragged_runs(n):
    """Runs of 8 equal rows of 1, 5, 13, 40, 49, 60, 3 and 27 entries (48 nonzeros is the kernel's first
    batch of index dwords): row i takes the offsets -(L // 2) .. L - L // 2 - 1 that fall inside, one
    value per offset, the diagonal 40."""
    lens = np.array([1, 5, 13, 40, 49, 60, 3, 27])
    L = lens[(np.arange(n) // 8) % 8]
    offs = np.arange(-30, 30)
    pal = np.random.default_rng(61).standard_normal(60)
    pal[30] = 40.0
    i, k = np.meshgrid(np.arange(n), np.arange(60), indexing="ij")
    o = offs[k]
    keep = (o >= -(L[i] // 2)) & (o < L[i] - L[i] // 2) & (i + o >= 0) & (i + o < n)
    return from_coo(i[keep], (i + o)[keep], pal[k[keep]], n)


def test_ragged_lengths(ctx):
    M = ragged_runs(1024)
    assert sorted(set(np.diff(M.rowptr)[64:960].tolist())) == [1, 3, 5, 13, 27, 40, 49, 60]
    A, B, lay = upload_both(ctx, M, True)
    assert lay["ell_class_census"]["classes_max"] >= 8, lay
    check_all(ctx, M, (A, B), 2)


def test_partial_tails(ctx):
    """64 * 5 + 17 rows: a last slice of 17 rows in a last group of two slices."""
    n = 64 * 5 + 17
    M = from_coo(*band(n), n)
    A, B, lay = upload_both(ctx, M, True)
    assert lay["ell_class_census"]["slices"] == 6 and lay["ell_xwin_census"]["full_groups"] < lay["ell_xwin_census"]["groups"], lay
    check_all(ctx, M, (A, B), 2)


def test_gather_groups(ctx):
    """Two diagonal blocks: 3072 tridiagonal rows (a group's window: <= 4 x 66 columns), then 1024 rows
    of the offsets {0, +-1, +-150 k, k = 1 .. 6} that stay inside the block (six or more of the far ones
    per row: a slice alone reads over 7 x 64 columns). With ell_xwin_max 384 the second block's groups
    gather, from the class records too, beside the windowed groups of the first."""
    n, h = 4096, 3072
    r1, c1, v1 = band(h, (-1, 0, 1), (-1.0, 4.0, -1.25))
    rows, cols, vals = [r1], [c1], [v1]
    for o in [-1, 0, 1] + [s * 150 * k for k in range(1, 7) for s in (-1, 1)]:
        i = np.arange(h, n)
        i = i[(i + o >= h) & (i + o < n)]
        rows.append(i)
        cols.append(i + o)
        vals.append(np.full(len(i), 9.0 if o == 0 else 0.125 + o / 1024.0))
    M = from_coo(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), n)
    A, B, lay = upload_both(ctx, M, True, ell_xwin_max=384)
    assert lay["ell_xwin_groups"] > 0 and lay["ell_gather_groups"] > 0 and lay["ell_xwin_max_window"] <= 384, lay
    check_all(ctx, M, (A, B), 2)


def test_constant_coefficient_grid(ctx):
    """16 x 16 x 12, 7 points: a slice is four x lines; its classes are the boundary kinds of its rows."""
    M = O.generate("poisson3d", 16, 16, 12)
    A, B, lay = upload_both(ctx, M, True)
    assert 2 <= lay["ell_class_census"]["classes_max"] <= 18, lay
    check_all(ctx, M, (A, B), 2)


@pytest.mark.parametrize("n,max_coarse,ell", [(64, 1000, False), (32, 100, True)])
def test_level1_in_cycle(ctx, n, max_coarse, ell):
    """poisson3d hierarchies with ell_min_rows 0: three V-cycles with ell_xwin 1 and with ell_xwin 2
    are the oracle's bit for bit; layout_of says which form the level-1 operator took. At 64^3 that
    operator (33 K rows) stays in tiles (the ELL upload declines it), so neither form runs there;
    at 32^3 (max_coarse 100: 4192 rows, the windowed layout) the class form is taken where allowed."""
    from parallel_amg_amd.solver import AMGSolver
    be = pa.SequentialBackend(1)
    Ah, offs, xs = pa.generate_problem(be, "poisson3d", n)
    H = pa.build_hierarchy(be, Ah, offs, pa.SAParams(max_coarse=max_coarse), device=ctx)
    Ao = O.generate("poisson3d", n, n, n)
    bo = O.spmv(Ao, O.xstar(Ao.nrows))
    Ho = O.setup(Ao, max_coarse=max_coarse)
    assert Ho.nlevels == H.nlevels
    xo = Ho.solve(bo, 3)
    for allowed in (1, 0):
        with options(ell_min_rows=0, ell_xwin=1 if allowed else 2):
            S = AMGSolver(ctx, H)
        lay = layout_of(S.A[1])
        assert lay["ell"] == lay["ell_xwin"] == ell and lay["ell_class"] == bool(ell and allowed), lay
        b = PVector(ctx, S.A[0].nrows)
        mul(b, S.A[0], PVector(ctx, S.A[0].nrows, 0, xs[0]))
        assert np.array_equal(bits(b.own_values()), bits(bo))
        x = S.new_vector()
        S.vcycle(x, b, 3)
        assert np.array_equal(bits(x.own_values()), bits(xo))
