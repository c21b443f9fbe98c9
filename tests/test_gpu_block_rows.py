"""Rectangular block rows on the GPU (pamg_mat_upload_block_rows; SPEC §S14, §S3 "Block rows"): a prolongation- or
restriction-shaped operator between two node-major spaces in the block-row layout gives SpMV and prolongate-add the
bits of the CSR row sums, in both forms of the layout — a lane per node (k_rows_bsr / k_rows_bsr_mc) and, for
operators with fewer rows than columns, a lane per scalar row (k_rows_bsr_r) — for one column and for several.

Shapes (block rows x block columns): 65 x 3 and 3 x 65 (one partly filled slice on either side), 257 x 40 and
40 x 257 (five slices of nodes: two workgroups), 1 x 1; ragged block rows everywhere, an empty block row in two.

Not covered: an x vector that is not 16-byte aligned. No entry point hands the kernels one — a vector starts at
its allocation and a multi-vector's columns start 256-byte aligned (SPEC §S13) — so the 8-byte x loads of block
sizes 2 and 4 are reached by no call."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd._lib import PamgError, call, layout_of
from parallel_amg_amd.partitioned import LocalWorld, MultiVector, PSparseMatrix, PVector, jacobi, mul, spmm
from parallel_amg_amd.solver import AMGSolver
import test_gpu_bsr as B
from test_gpu_block_smoother import bits, differ, to_hcsr
from test_gpu_bsr import from_blocks, raw_layout, same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(65, 3), (3, 65), (257, 40), (40, 257), (1, 1)]
EMPTY_ROW = {(65, 3): 7, (40, 257): 5}
KS = [1, 2, 3, 4, 5, 8]


@contextlib.contextmanager
def row_lanes(value):
    """PAMG_BSR_ROW_LANES for the uploads inside: "0" a lane per node, "1" a lane per row, None the upload's rule."""
    old = os.environ.pop("PAMG_BSR_ROW_LANES", None)
    if value is not None:
        os.environ["PAMG_BSR_ROW_LANES"] = value
    try:
        yield
    finally:
        os.environ.pop("PAMG_BSR_ROW_LANES", None)
        if old is not None:
            os.environ["PAMG_BSR_ROW_LANES"] = old


def rect_blocks(nbr, nbc, bs, seed, deg=9):
    """A random nbr x nbc block matrix: block row m holds 1 .. min(nbc, deg) whole blocks at distinct random block
    columns (ragged), none in EMPTY_ROW's row; values uniform in (-1, 1)."""
    rng = np.random.default_rng(seed)
    br, bc = [], []
    for m in range(nbr):
        cnt = 0 if EMPTY_ROW.get((nbr, nbc)) == m else int(rng.integers(1, min(nbc, deg) + 1))
        br += [m] * cnt
        bc += sorted(rng.choice(nbc, cnt, replace=False).tolist())
    br, bc = np.array(br, np.int64), np.array(bc, np.int64)
    M = from_blocks(nbr, bs, br, bc, rng.uniform(-1.0, 1.0, (len(br), bs, bs)))
    return O.CSR(M.rowptr, M.col, M.val, nbc * bs)


def forms_of(nbr, nbc):
    """The forms of the layout an nbr x nbc operator can take: (environment value, row-per-lane?)."""
    return [("0", False), ("1", True)] if nbr < nbc else [(None, False), ("1", False)]


_cases = {}


def case(ctx, bs, nbr, nbc):
    """The matrix, its uploads (one per form, and a plain PSparseMatrix), a random x and y0, the oracle's SpMV."""
    key = (bs, nbr, nbc)
    if key not in _cases:
        M = rect_blocks(nbr, nbc, bs, 100 * bs + nbr)
        assert M.nrows == nbr * bs and M.ncols == nbc * bs
        per = np.diff(M.rowptr)[::bs] // bs
        assert nbr == 1 or per.min() < per.max()
        ups = []
        for env, want_rows in forms_of(nbr, nbc):
            with row_lanes(env):
                D = PSparseMatrix(ctx, to_hcsr(M), block_rows=bs)
            lay = raw_layout(D)
            assert lay[9] & 32768 and D.blocked and layout_of(D)["bsr"], (key, env, lay)
            assert lay[3] == bs and D.row_lanes == want_rows == layout_of(D)["bsr_row_lanes"], (key, env, lay)
            if want_rows:   # 64 scalar rows per slice: a column and bs values per padded slot
                n = M.nrows
                perrow = np.diff(M.rowptr) // bs
                slots = 64 * sum(int(perrow[s:s + 64].max()) for s in range(0, n, 64))
                assert lay[4] == slots and lay[8] == ((n + 63) // 64 + 3) // 4, lay
                assert D.stream_bytes == 4 + slots * (4 + 8 * bs) + 8 * ((n + 63) // 64 + 1)
            else:
                slots = 64 * sum(int(per[s:s + 64].max()) for s in range(0, nbr, 64))
                assert lay[4] == slots and lay[8] == ((nbr + 63) // 64 + 3) // 4, lay
                assert D.stream_bytes == 4 + slots * (4 + 8 * bs * bs) + 8 * ((nbr + 63) // 64 + 1)
            ups.append(D)
        with row_lanes(None):   # the upload's own rule is one of the forms above
            Dd = PSparseMatrix(ctx, to_hcsr(M), block_rows=bs)
        assert Dd.blocked and (not Dd.row_lanes or nbr < nbc)
        ups.append(Dd)
        P = PSparseMatrix(ctx, to_hcsr(M))
        assert not P.blocked and not layout_of(P)["bsr"]
        rng = np.random.default_rng(31 * bs + nbr)
        xh, y0 = rng.standard_normal((M.ncols, 8)), rng.standard_normal((M.nrows, 8))
        want = np.stack([O.spmv(M, xh[:, c]) for c in range(8)], axis=1)
        want.setflags(write=False)
        _cases[key] = (M, ups, P, xh, y0, want)
    return _cases[key]


def spmv_dev(ctx, D, xh):
    y = PVector(ctx, D.nrows)
    return mul(y, D, PVector(ctx, D.n_own_cols, 0, xh)).own_values()


def prolong_dev(ctx, D, xh, y0):
    """pamg_bench_rowop op 3 with one repetition: a warm-up launch and a timed one, y = (y0 + s) + s."""
    x, y = PVector(ctx, D.n_own_cols, 0, xh), PVector(ctx, D.nrows, 0, y0)
    ms = ctypes.c_double()
    call("pamg_bench_rowop", ctx.handle, D.handle, 3, x.handle, None, y.handle, 0.0, 1, ctypes.byref(ms))
    return y.own_values()


def eq(got, want):
    return np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------------------ one column
@pytest.mark.parametrize("nbr,nbc", SHAPES)
@pytest.mark.parametrize("bs", [2, 3, 4])
def test_spmv_and_prolongate_add_bits(ctx, bs, nbr, nbc):
    M, ups, P, xh, y0, want = case(ctx, bs, nbr, nbc)
    x, y = xh[:, 0], y0[:, 0]
    plain = spmv_dev(ctx, P, x)
    assert eq(plain, want[:, 0])
    if (nbr, nbc) in EMPTY_ROW:
        r = EMPTY_ROW[nbr, nbc] * bs
        assert np.all(bits(want[r:r + bs, 0]) == 0)     # an empty row sums to +0.0
    for D in ups:
        got = spmv_dev(ctx, D, x)
        assert eq(got, want[:, 0]) and eq(got, plain), (D.row_lanes, differ(bits(got), bits(want[:, 0])))
        got = prolong_dev(ctx, D, x, y)
        assert eq(got, (y + want[:, 0]) + want[:, 0]), (D.row_lanes, "prolong")
        assert eq(got, prolong_dev(ctx, P, x, y))


@pytest.mark.parametrize("nbr,nbc", [(65, 3), (3, 65), (257, 40), (40, 257)])
@pytest.mark.parametrize("bs", [2, 3, 4])
def test_x_edge_values_stay_in_the_rows_they_reach(ctx, bs, nbr, nbc):
    M, ups, P, xh, _y0, _want = case(ctx, bs, nbr, nbc)
    neg = np.full(M.ncols, -0.0)
    edge = xh[:, 1].copy()
    cols = np.unique(M.col)                        # columns some row reads
    edge[cols[len(cols) // 3]] = np.nan
    edge[cols[(2 * len(cols)) // 3]] = np.inf
    w_neg, w_edge = O.spmv(M, neg), O.spmv(M, edge)
    assert not np.all(np.isfinite(w_edge)) and np.any(np.isfinite(w_edge))
    for D in ups + [P]:
        assert eq(spmv_dev(ctx, D, neg), w_neg), D.row_lanes
        got = spmv_dev(ctx, D, edge)
        assert np.array_equal(np.isfinite(got), np.isfinite(w_edge)) and same_bits(got, w_edge), D.row_lanes


# ------------------------------------------------------------------------------ several columns
def rowop_multi(ctx, D, op, X, Y):
    ms = ctypes.c_double()
    call("pamg_bench_rowop_multi", ctx.handle, D.handle, op, X.handle, None, Y.handle, 0.0, 1, ctypes.byref(ms))
    return Y.to_numpy()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("nbr,nbc", [(257, 40), (40, 257)])
@pytest.mark.parametrize("bs", [2, 3, 4])
def test_multi_column_bits(ctx, bs, nbr, nbc, k):
    M, ups, _P, xh, y0, want = case(ctx, bs, nbr, nbc)
    for D in ups:
        X, Y = MultiVector.from_numpy(ctx, xh[:, :k]), MultiVector(ctx, M.nrows, k)
        got = spmm(Y, D, X).to_numpy()
        assert eq(got, want[:, :k]), (D.row_lanes, k)
        Y.set(y0[:, :k])
        pro = rowop_multi(ctx, D, 3, X, Y)
        assert eq(pro, (y0[:, :k] + want[:, :k]) + want[:, :k]), (D.row_lanes, k, "prolong")
        # column c is the single-column call on a column view
        W = MultiVector.from_numpy(ctx, y0[:, :k])
        for c in range(k):
            assert eq(mul(W.column(c), D, X.column(c)).own_values(), got[:, c]), (D.row_lanes, k, c)
        assert eq(X.to_numpy(), xh[:, :k])


def test_columns_do_not_mix(ctx):
    bs, nbr, nbc = 3, 40, 257
    M, ups, _P, xh, _y0, want = case(ctx, bs, nbr, nbc)
    xs = xh[:, :4].copy()
    xs[100 * bs + 1, 1] = np.nan
    xs[:, 2] = -0.0
    w1, w2 = O.spmv(M, xs[:, 1]), O.spmv(M, xs[:, 2])
    for D in ups:
        X, Y = MultiVector.from_numpy(ctx, xs), MultiVector(ctx, M.nrows, 4)
        got = spmm(Y, D, X).to_numpy()
        assert eq(got[:, 0], want[:, 0]) and eq(got[:, 3], want[:, 3]) and eq(got[:, 2], w2)
        assert same_bits(got[:, 1], w1) and np.any(np.isnan(got[:, 1])) and np.any(np.isfinite(got[:, 1]))


# ------------------------------------------------------------------------------ declines
def rect_partial_block():
    M = rect_blocks(40, 257, 3, 5)
    keep = np.ones(M.nnz, bool)
    keep[M.rowptr[10] + 1] = False                 # row 10 (node 3, d = 1) loses entry 1 of its first block
    rows = np.repeat(np.arange(M.nrows), np.diff(M.rowptr))
    rp = np.concatenate(([0], np.cumsum(np.bincount(rows[keep], minlength=M.nrows)))).astype(np.int64)
    return O.CSR(rp, M.col[keep].copy(), M.val[keep].copy(), M.ncols)


def rect_different_blocks():
    """B.rows_with_different_blocks with four more columns: 4 x 6 nodes of two unknowns."""
    M = B.rows_with_different_blocks()
    return O.CSR(M.rowptr, M.col, M.val, 12)


@pytest.mark.parametrize("gen,bs", [(rect_partial_block, 3), (rect_different_blocks, 2), (B.unsorted_blocks, 2)],
                         ids=["partial_block", "different_block_columns", "descending_blocks"])
def test_declined_matrices_upload_in_the_existing_layouts(ctx, gen, bs):
    M = gen()
    D, P = PSparseMatrix(ctx, to_hcsr(M), block_rows=bs), PSparseMatrix(ctx, to_hcsr(M))
    lay = raw_layout(D)
    assert not lay[9] & 32768 and not D.blocked and not D.row_lanes
    assert lay == raw_layout(P) and D.stream_bytes == P.stream_bytes
    x = np.random.default_rng(2).standard_normal(M.ncols)
    want = O.spmv(M, x)
    assert eq(spmv_dev(ctx, D, x), want) and eq(spmv_dev(ctx, P, x), want)


def test_parts_with_ghost_columns_decline(built):
    """A nodal hierarchy on two parts, every operator asked into block rows: the operators with ghost columns keep
    today's layouts, and level 0's SpMV has the oracle's bits."""
    n = 4
    Ao = O.generate("elastic3d", n, n, n)
    W = LocalWorld(2)
    try:
        be = pa.SequentialBackend(2)
        A, offs, xs = pa.generate_problem(be, "elastic3d", n)
        assert np.all(offs % 3 == 0)
        H = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=40, block_size=3, agglomerate=0))
        assert H.nlevels >= 2 and H.block_size == 3
        S = [AMGSolver(W.ctxs[p], H, part=p, block_layout="all") for p in range(2)]
        plain = [AMGSolver(W.ctxs[p], H, part=p) for p in range(2)]
        for p in range(2):
            assert S[p].block_layout_P == S[p].block_layout_R == {l: 3 for l in range(H.nlevels - 1)}
            for ops, ref in ((S[p].A_dev[:1], plain[p].A_dev[:1]), (S[p].P[:1], plain[p].P[:1]),
                             (S[p].R[:1], plain[p].R[:1])):
                for Q, Q0 in zip(ops, ref):
                    if Q.n_ghost > 0:
                        assert not Q.blocked
                        for st in (0, 1):
                            assert layout_of(Q, st) == layout_of(Q0, st)
            assert S[p].A_dev[0].n_ghost > 0
        xst = [PVector(W.ctxs[p], S[p].A[0].n_own_cols, S[p].A[0].n_ghost, xs[p]) for p in range(2)]
        y = [PVector(W.ctxs[p], S[p].A[0].nrows) for p in range(2)]
        W.run(lambda p: mul(y[p], S[p].A[0], xst[p]))
        got = np.concatenate([v.own_values() for v in y])
    finally:
        del S, plain
        W.close()
    assert eq(got, O.spmv(Ao, O.xstar(Ao.nrows)))


# ------------------------------------------------------------------------------ argument errors
def upload_raw(ctx, M, bs):
    h = ctypes.c_void_p()
    col = np.ascontiguousarray(M.col, np.int32)
    rp, val = np.ascontiguousarray(M.rowptr, np.int64), np.ascontiguousarray(M.val, np.float64)
    call("pamg_mat_upload_block_rows", ctx.handle, M.nrows, M.ncols, rp.ctypes.data_as(ctypes.c_void_p),
         col.ctypes.data_as(ctypes.c_void_p), 0, val.ctypes.data_as(ctypes.c_void_p), 0, None, bs, ctypes.byref(h))
    return h


def test_argument_errors_leave_the_context_alone(ctx):
    M = rect_blocks(40, 257, 3, 5)                 # 120 x 771
    refs = ctx.refcount()
    for bad_bs in (5, 0, -1):
        with pytest.raises(PamgError) as e:
            upload_raw(ctx, M, bad_bs)
        assert e.value.code == -1 and "outside 1..4" in str(e.value), e.value
    short = O.CSR(M.rowptr[:120].copy(), M.col[:M.rowptr[119]].copy(), M.val[:M.rowptr[119]].copy(), M.ncols)
    with pytest.raises(PamgError) as e:            # 119 rows
        upload_raw(ctx, short, 3)
    assert e.value.code == -1 and "119 rows are not whole blocks" in str(e.value), e.value
    with pytest.raises(PamgError) as e:            # 771 own columns, blocks of 2
        upload_raw(ctx, M, 2)
    assert e.value.code == -1 and "771 own columns are not whole blocks" in str(e.value), e.value
    wide = O.CSR(M.rowptr, M.col, M.val, 772)
    with pytest.raises(PamgError) as e:
        upload_raw(ctx, wide, 3)
    assert e.value.code == -1 and "own columns" in str(e.value), e.value
    bad = O.CSR(M.rowptr, M.col.copy(), M.val, M.ncols)
    bad.col[5] = 771                               # a column out of range, past the argument checks
    with pytest.raises(PamgError):
        upload_raw(ctx, bad, 3)
    assert ctx.refcount() == refs
    h = upload_raw(ctx, short, 1)                  # bs = 1 is pamg_mat_upload
    call("pamg_mat_destroy", h)
    with pytest.raises(ValueError, match="not both"):
        PSparseMatrix(ctx, to_hcsr(M), block_size=3, block_rows=3)
    assert ctx.refcount() == refs


@pytest.mark.parametrize("nbr,nbc", [(257, 40), (40, 257)])
def test_jacobi_on_a_rectangular_block_row_matrix_is_an_argument_error(ctx, nbr, nbc):
    M, ups, _P, xh, y0, want = case(ctx, 3, nbr, nbc)
    for D in ups:
        x, t, b = PVector(ctx, M.ncols, 0, xh[:, 0]), PVector(ctx, M.ncols), PVector(ctx, M.nrows, 0, y0[:, 0])
        with pytest.raises(PamgError) as e:
            jacobi(x, D, b, t, 0.6, 1)
        assert e.value.code == -1 and "must be square" in str(e.value), e.value
        assert eq(x.own_values(), xh[:, 0])
        assert eq(spmv_dev(ctx, D, xh[:, 0]), want[:, 0])   # and the matrix still works
