"""Operators stored in binary32 (SPEC §S15; pamg_mat_upload_f32) on the GPU. An upload with value_bits = 32 IS the
operator A~ = RN32(A): every call on it has the bits of the same call on an fp64 block-row upload of the rounded
array and of the oracle run on the rounded matrix, whichever layout and form the matrix takes, and the block-row
layouts store 4 bytes per value. PCG around a rounded hierarchy solves with the exact operator
(pamg_hier_set_outer).

Shapes: block sizes 2, 3, 4; square random block SPD matrices of 65 and 257 nodes (a partial slice; two
workgroups) and one node; rectangular 65 x 3, 3 x 65, 257 x 40, 40 x 257 and 1 x 1 block rows, ragged, in both
forms of the layout, and 3 x 65 with every slice width 1 .. 9 (every remainder of the row-per-lane form's four-slot
unroll); 1 .. 8 columns. Cycles: the variable-coefficient L_w (x) B of tests/test_gpu_bsr.py at 8^3 nodes on the
scalar hierarchy with level 0 in block rows, and at 7^3 on a nodal hierarchy with every level in block rows."""
import ctypes

import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd import hcsr as HC
from parallel_amg_amd._lib import PamgError, call, layout_of
from parallel_amg_amd.hierarchy import HostPlan, round_values
from parallel_amg_amd.partitioned import (DevicePlan, MultiVector, PSparseMatrix, PVector, block_chebyshev,
                                          block_jacobi, mul, residual)
from parallel_amg_amd.solver import AMGSolver
import test_gpu_block_rows as R
import test_gpu_block_smoother as T
import test_gpu_bsr as B
from test_gpu_block_smoother import bits, differ, to_hcsr

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
OVER = 2.0 ** 128 - 2.0 ** 103          # the smallest magnitude that rounds to an infinite binary32


def rn32(v):
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def rounded(M):
    return O.CSR(M.rowptr, M.col, rn32(M.val), M.ncols)


def eq(got, want):
    return np.array_equal(bits(got), bits(want))


def value_bits(D):
    out = ctypes.c_int()
    call("pamg_mat_value_bits", D.handle, ctypes.byref(out))
    return out.value


def slots_of(M, bs, row_lanes):
    """The padded slots and slices of the block-row layout: per node, or per scalar row in the row-per-lane form."""
    per = np.diff(M.rowptr) // bs
    if not row_lanes:
        per = per[::bs]
    n = len(per)
    return 64 * sum(int(per[s:s + 64].max()) for s in range(0, n, 64)), (n + 63) // 64


def check_report(F, M, bs, row_lanes):
    """Bit 16 with bit 15, 32 value bits and the stream of 4-byte values (all of which fail on the parent)."""
    lay = B.raw_layout(F)
    assert lay[9] & 32768 and lay[9] & 65536 and F.blocked and F.f32_storage, lay
    assert layout_of(F)["bsr"] and layout_of(F)["bsr_f32"]
    assert F.row_lanes == row_lanes == (lay[6] == 1) and lay[3] == bs, lay
    assert value_bits(F) == 32 and F.value_bits == 32
    slots, slices = slots_of(M, bs, row_lanes)
    assert lay[4] == slots
    per_slot = 4 + 4 * (bs if row_lanes else bs * bs)
    assert F.stream_bytes == 4 + slots * per_slot + 8 * (slices + 1), (F.stream_bytes, slots, slices)


def rowop(ctx, D, op, xh, bh, yh, omega=0.375):
    """pamg_bench_rowop with one repetition (a warm-up launch and a timed one)."""
    x, y = PVector(ctx, D.n_own_cols, 0, xh), PVector(ctx, D.nrows, 0, yh)
    b = PVector(ctx, D.nrows, 0, bh) if bh is not None else None
    ms = ctypes.c_double()
    call("pamg_bench_rowop", ctx.handle, D.handle, op, x.handle, b.handle if b is not None else None, y.handle, omega,
         1, ctypes.byref(ms))
    return y.own_values()


def rowop_multi(ctx, D, op, xh, bh, yh, omega=0.375):
    X, Y = MultiVector.from_numpy(ctx, xh), MultiVector.from_numpy(ctx, yh)
    Bm = MultiVector.from_numpy(ctx, bh) if bh is not None else None
    ms = ctypes.c_double()
    call("pamg_bench_rowop_multi", ctx.handle, D.handle, op, X.handle, Bm.handle if Bm is not None else None, Y.handle,
         omega, 1, ctypes.byref(ms))
    return Y.to_numpy()


# ------------------------------------------------------------------------------ square operators
SQUARE = {}
for _bs in (2, 3, 4):
    SQUARE[f"one_node-bs{_bs}"] = (lambda b=_bs: B.one_node(b), _bs)
    for _nb in (65, 257):
        SQUARE[f"random{_nb}-bs{_bs}"] = (lambda n=_nb, b=_bs: B.random_block_spd(n, b, 10 * n + b), _bs)
_square = {}


def square(ctx, name):
    """The matrix, its rounding, the f32 upload F, the fp64 block-row upload D of the rounded array (both with the
    rounded matrix's block data), eight random columns of x and b, and the oracle's results on the rounded matrix."""
    if name not in _square:
        gen, bs = SQUARE[name]
        M = gen()
        Mr = rounded(M)
        F = PSparseMatrix(ctx, to_hcsr(M), block_size=bs, value_bits=32)
        D = PSparseMatrix(ctx, to_hcsr(Mr), block_size=bs)
        check_report(F, M, bs, False)
        assert B.raw_layout(D)[9] & 32768 and not B.raw_layout(D)[9] & 65536 and value_bits(D) == 64
        assert D.stream_bytes - F.stream_bytes == 4 * bs * bs * B.raw_layout(F)[4]
        blocks, inv, _rho = HC.block_diag(to_hcsr(Mr), 0, bs)
        for Q in (F, D):
            Q.set_block_diag(bs, blocks, inv)
        rng = np.random.default_rng(11)
        xh, bh = rng.standard_normal((M.nrows, 8)), rng.standard_normal((M.nrows, 8))
        want = {"spmv": np.stack([O.spmv(Mr, xh[:, c]) for c in range(8)], axis=1),
                "residual": np.stack([O.residual(Mr, xh[:, c], bh[:, c]) for c in range(8)], axis=1),
                "jacobi": np.stack([O.jacobi(Mr, xh[:, c], bh[:, c], B.OMEGA) for c in range(8)], axis=1)}
        for a in (xh, bh, *want.values()):
            a.setflags(write=False)
        _square[name] = (M, Mr, F, D, bs, inv, xh, bh, want)
    return _square[name]


@pytest.mark.parametrize("name", list(SQUARE))
def test_square_row_ops_bits(ctx, name):
    """SpMV, residual, Jacobi, the Chebyshev step and prolongate-add; the fused block Jacobi and block Chebyshev."""
    M, Mr, F, D, bs, inv, xs, bs_, want = square(ctx, name)
    xh, bh = xs[:, 0], bs_[:, 0]
    gotF, gotD = B.run_ops(ctx, F, xh, bh), B.run_ops(ctx, D, xh, bh)
    for op in ("spmv", "residual", "jacobi"):
        assert eq(gotF[op], want[op][:, 0]), (name, op, differ(bits(gotF[op]), bits(want[op][:, 0])))
        assert eq(gotF[op], gotD[op]), (name, op)
    # not vacuous: the unrounded matrix gives other bits (one_node's entries are exact in binary32)
    if name.startswith("one_node"):
        assert np.array_equal(Mr.val, M.val)
    else:
        assert not np.array_equal(Mr.val, M.val) and not eq(O.spmv(M, xh), want["spmv"][:, 0])
    u = want["residual"][:, 0]
    step = xh + ((0.375 * (xh - 0.0)) + ((0.375 * u) / T.diag_of(Mr)))
    y0 = np.zeros(M.nrows)
    assert eq(rowop(ctx, F, 6, xh, bh, y0), step) and eq(rowop(ctx, D, 6, xh, bh, y0), step), name
    s = want["spmv"][:, 0]
    assert eq(rowop(ctx, F, 3, xh, None, bh), (bh + s) + s) and eq(rowop(ctx, D, 3, xh, None, bh), (bh + s) + s), name
    # the fused point-block sweeps (SPEC §S12 on A~: the block data is the rounded matrix's)
    jac = T.block_jacobi_ref(Mr, inv, bs, T.block_jacobi_ref(Mr, inv, bs, xh, bh, T.OMEGA), bh, T.OMEGA)
    c1, c2 = T.coeffs_ref(T.LMAX, T.RATIO, 3)
    cheb = T.block_cheb_ref(Mr, inv, bs, xh, bh, c1, c2, 3)
    for Q in (F, D):
        x, b, t1, t2 = (PVector(ctx, M.nrows, 0, xh), PVector(ctx, M.nrows, 0, bh), Q.new_input_vector(),
                        Q.new_input_vector())
        block_jacobi(x, Q, b, t1, T.OMEGA, 2)
        assert eq(x.own_values(), jac), (name, Q is F, differ(bits(x.own_values()), bits(jac)))
        x.set(xh)
        block_chebyshev(x, Q, b, t1, t2, lmax=T.LMAX, ratio=T.RATIO, degree=3)
        assert eq(x.own_values(), cheb), (name, Q is F, differ(bits(x.own_values()), bits(cheb)))


@pytest.mark.parametrize("k", range(1, 9))
@pytest.mark.parametrize("name", ["random257-bs2", "random257-bs3", "random257-bs4", "random65-bs3"])
def test_square_multi_column_bits(ctx, name, k):
    """k = 1 .. 8 columns (chunks of 4, 2 and 1): each column has the single-column bits."""
    M, Mr, F, D, bs, inv, xs, bs_, want = square(ctx, name)
    xh, bh = np.asfortranarray(xs[:, :k]), np.asfortranarray(bs_[:, :k])
    zero = np.zeros((M.nrows, k))
    assert eq(rowop_multi(ctx, F, 0, xh, None, zero), want["spmv"][:, :k]), (name, k)
    assert eq(rowop_multi(ctx, F, 1, xh, bh, zero), want["residual"][:, :k]), (name, k)
    assert eq(rowop_multi(ctx, F, 2, xh, bh, zero, B.OMEGA), want["jacobi"][:, :k]), (name, k)
    for op in (3, 6, 7, 8):          # prolongate-add, the Chebyshev step, the fused block sweeps
        b = None if op == 3 else bh
        gF, gD = rowop_multi(ctx, F, op, xh, b, bh), rowop_multi(ctx, D, op, xh, b, bh)
        assert eq(gF, gD), (name, k, op)
        if op == 7:
            for c in range(k):
                assert eq(gF[:, c], T.block_jacobi_ref(Mr, inv, bs, xh[:, c], bh[:, c], 0.375)), (name, k, c)


def test_square_columns_do_not_mix(ctx):
    M, Mr, F, _D, bs, _inv, xs, _bs, want = square(ctx, "random257-bs3")
    xh = np.asfortranarray(xs[:, :4]).copy()
    xh[100 * bs + 1, 1] = np.nan
    xh[:, 2] = -0.0
    w1, w2 = O.spmv(Mr, xh[:, 1]), O.spmv(Mr, xh[:, 2])
    got = rowop_multi(ctx, F, 0, xh, None, np.zeros((M.nrows, 4)))
    assert eq(got[:, 0], want["spmv"][:, 0]) and eq(got[:, 3], want["spmv"][:, 3]) and eq(got[:, 2], w2)
    assert B.same_bits(got[:, 1], w1) and np.any(np.isnan(got[:, 1])) and np.any(np.isfinite(got[:, 1]))


# ------------------------------------------------------------------------------ rectangular operators
_rect = {}


def rect(ctx, bs, nbr, nbc):
    """Per form of the layout: the f32 upload and the fp64 block-row upload of the rounded array."""
    key = (bs, nbr, nbc)
    if key not in _rect:
        M = R.rect_blocks(nbr, nbc, bs, 100 * bs + nbr)
        Mr = rounded(M)
        per = np.diff(M.rowptr)[::bs] // bs
        assert nbr == 1 or (per.min() < per.max() and per.max() <= 9)
        assert (nbr, nbc) not in R.EMPTY_ROW or per[R.EMPTY_ROW[nbr, nbc]] == 0
        ups = []
        for env, want_rows in R.forms_of(nbr, nbc):
            with R.row_lanes(env):
                F = PSparseMatrix(ctx, to_hcsr(M), block_rows=bs, value_bits=32)
                D = PSparseMatrix(ctx, to_hcsr(Mr), block_rows=bs)
            check_report(F, M, bs, want_rows)
            assert D.blocked and D.row_lanes == want_rows and not D.f32_storage and value_bits(D) == 64
            ups.append((F, D))
        rng = np.random.default_rng(31 * bs + nbr)
        xh, y0 = rng.standard_normal((M.ncols, 8)), rng.standard_normal((M.nrows, 8))
        want = np.stack([O.spmv(Mr, xh[:, c]) for c in range(8)], axis=1)
        assert nbr == 1 or not eq(O.spmv(M, xh[:, 0]), want[:, 0])      # not vacuous
        for a in (xh, y0, want):
            a.setflags(write=False)
        _rect[key] = (M, Mr, ups, xh, y0, want)
    return _rect[key]


def rect_ops(ctx, Q, x, y):
    out = {"spmv": R.spmv_dev(ctx, Q, x), "prolong": R.prolong_dev(ctx, Q, x, y)}
    r = PVector(ctx, Q.nrows)
    residual(r, Q, PVector(ctx, Q.n_own_cols, 0, x), PVector(ctx, Q.nrows, 0, y))
    out["residual"] = r.own_values()
    return out


@pytest.mark.parametrize("nbr,nbc", R.SHAPES)
@pytest.mark.parametrize("bs", [2, 3, 4])
def test_rectangular_row_ops_bits(ctx, bs, nbr, nbc):
    """SpMV, residual and prolongate-add, a lane per node and a lane per row."""
    M, Mr, ups, xh, y0, want = rect(ctx, bs, nbr, nbc)
    x, y, s = xh[:, 0], y0[:, 0], want[:, 0]
    ref = {"spmv": s, "prolong": (y + s) + s, "residual": y - s}
    for F, D in ups:
        gF, gD = rect_ops(ctx, F, x, y), rect_ops(ctx, D, x, y)
        for op in ref:
            assert eq(gF[op], ref[op]), (F.row_lanes, op, differ(bits(gF[op]), bits(ref[op])))
            assert eq(gF[op], gD[op]), (F.row_lanes, op)
    if (nbr, nbc) in R.EMPTY_ROW:
        r0 = R.EMPTY_ROW[nbr, nbc] * bs
        assert np.all(bits(s[r0:r0 + bs]) == 0)         # an empty block row sums to +0.0


@pytest.mark.parametrize("k", range(1, 9))
@pytest.mark.parametrize("nbr,nbc", [(257, 40), (40, 257)])
@pytest.mark.parametrize("bs", [2, 3, 4])
def test_rectangular_multi_column_bits(ctx, bs, nbr, nbc, k):
    M, Mr, ups, xh, y0, want = rect(ctx, bs, nbr, nbc)
    xk, yk, sk = np.asfortranarray(xh[:, :k]), np.asfortranarray(y0[:, :k]), want[:, :k]
    for F, D in ups:
        assert eq(rowop_multi(ctx, F, 0, xk, None, yk), sk), (F.row_lanes, k)
        assert eq(rowop_multi(ctx, F, 1, xk, yk, np.zeros_like(yk)), yk - sk), (F.row_lanes, k, "residual")
        assert eq(rowop_multi(ctx, F, 3, xk, None, yk), (yk + sk) + sk), (F.row_lanes, k, "prolong")
        assert eq(rowop_multi(ctx, D, 0, xk, None, yk), sk), (D.row_lanes, k)
    if k == 4:          # no column mixes with another
        xs = xk.copy()
        xs[20 * bs + 1, 1] = np.nan
        xs[:, 2] = -0.0
        w1, w2 = O.spmv(Mr, xs[:, 1]), O.spmv(Mr, xs[:, 2])
        for F, _D in ups:
            got = rowop_multi(ctx, F, 0, xs, None, yk)
            assert eq(got[:, 0], sk[:, 0]) and eq(got[:, 3], sk[:, 3]) and eq(got[:, 2], w2), F.row_lanes
            assert B.same_bits(got[:, 1], w1) and np.any(np.isnan(got[:, 1])) and np.any(np.isfinite(got[:, 1]))


@pytest.mark.parametrize("width", range(1, 10))
@pytest.mark.parametrize("bs", [2, 3, 4])
def test_every_slice_width_of_the_row_per_lane_form(ctx, bs, width):
    """3 x 65 block rows, block row 0 exactly `width` blocks wide and the others 1 .. width: the one slice is
    `width` slots wide, so the four-slot groups leave every remainder over widths 1 .. 9."""
    rng = np.random.default_rng(1000 * bs + width)
    br, bc = [], []
    for m in range(3):
        cnt = width if m == 0 else int(rng.integers(1, width + 1))
        br += [m] * cnt
        bc += sorted(rng.choice(65, cnt, replace=False).tolist())
    br, bc = np.array(br, np.int64), np.array(bc, np.int64)
    M = B.from_blocks(3, bs, br, bc, rng.uniform(-1.0, 1.0, (len(br), bs, bs)))
    M = O.CSR(M.rowptr, M.col, M.val, 65 * bs)
    Mr = rounded(M)
    with R.row_lanes("1"):
        F = PSparseMatrix(ctx, to_hcsr(M), block_rows=bs, value_bits=32)
    check_report(F, M, bs, True)
    assert B.raw_layout(F)[4] == 64 * width
    xh = rng.standard_normal((M.ncols, 3))
    want = np.stack([O.spmv(Mr, xh[:, c]) for c in range(3)], axis=1)
    assert eq(R.spmv_dev(ctx, F, xh[:, 0]), want[:, 0]), differ(bits(R.spmv_dev(ctx, F, xh[:, 0])), bits(want[:, 0]))
    assert eq(rowop_multi(ctx, F, 0, np.asfortranarray(xh), None, np.zeros((M.nrows, 3))), want)


# ------------------------------------------------------------------------------ rounding edges
def edge_matrix(bs, top=FLT_MAX):
    """Five nodes; node 0's block row holds the edge values in its blocks (0, 1) .. (0, 4), every block whole:
    a tie that rounds to even, a value that rounds to an f32 subnormal, +-1e-50 (rounds to +-0, stays stored) and
    `top`; the other block rows are a diagonal block and one neighbour."""
    rng = np.random.default_rng(5)
    edges = [1.0 + 2.0 ** -24, 1e-40, 1e-50, top]
    br, bc, bv = [], [], []
    for m in range(5):
        br.append(m)
        bc.append(m)
        bv.append(8.0 * np.eye(bs) + rng.uniform(-1.0, 1.0, (bs, bs)))
    for j, e in enumerate(edges):
        blk = np.full((bs, bs), e)
        blk[1, :] = -e
        br.append(0)
        bc.append(j + 1)
        bv.append(blk)
    for m in range(1, 5):
        br.append(m)
        bc.append(0)
        bv.append(rng.uniform(-1.0, 1.0, (bs, bs)))
    return B.from_blocks(5, bs, np.array(br), np.array(bc), np.array(bv))


@pytest.mark.parametrize("bs", [2, 3, 4])
def test_rounding_edges(ctx, bs):
    M = edge_matrix(bs, top=np.nextafter(OVER, 0.0))     # the double just below the bound: stored as FLT_MAX
    Mr = rounded(M)
    k0 = M.rowptr[0] + bs                                # row 0: the diagonal block, then the four edge blocks
    assert list(Mr.val[k0:k0 + 4 * bs:bs]) == [1.0, 71362 * 2.0 ** -149, 0.0, FLT_MAX]
    k1 = M.rowptr[1] + bs
    assert list(Mr.val[k1:k1 + 4 * bs:bs]) == [-1.0, -71362 * 2.0 ** -149, -0.0, -FLT_MAX]
    assert np.signbit(Mr.val[k1 + 2 * bs]) and not np.signbit(Mr.val[k0 + 2 * bs])
    assert Mr.nnz == M.nnz                               # the entries that round to zero stay stored
    F = PSparseMatrix(ctx, to_hcsr(M), block_size=bs, value_bits=32)
    D = PSparseMatrix(ctx, to_hcsr(Mr), block_size=bs)
    check_report(F, M, bs, False)
    rng = np.random.default_rng(9)
    n = M.nrows
    bh = rng.standard_normal(n)
    xs = {"random": rng.standard_normal(n), "ones": np.ones(n), "negzero": np.full(n, -0.0),
          "huge": np.full(n, 2.0 ** 100), "tiny": np.full(n, 2.0 ** -960)}
    xs["mixed"] = xs["random"].copy()
    xs["mixed"][2 * bs] = -0.0                           # a -0.0 entry of x under the subnormal block
    nan = xs["random"].copy()
    nan[4 * bs] = np.nan                                 # node 4: read by block rows 0 and 4 only
    nan[3 * bs + 1] = np.inf                             # node 3: block rows 0 and 3
    for tag, xh in xs.items():
        got, ref, want = B.run_ops(ctx, F, xh, bh), B.run_ops(ctx, D, xh, bh), B.oracle_ops(Mr, xh, bh)
        for op in want:
            assert B.same_bits(got[op], want[op]), (bs, tag, op, differ(bits(got[op]), bits(want[op])))
            assert B.same_bits(got[op], ref[op]), (bs, tag, op)
    # the widening keeps subnormals: 2^100 times the subnormal entry is far from zero
    sub = np.zeros(n)
    sub[2 * bs:3 * bs] = 2.0 ** 100
    y = R.spmv_dev(ctx, F, sub)
    assert eq(y, O.spmv(Mr, sub)) and y[0] == bs * (71362 * 2.0 ** -149) * 2.0 ** 100 and y[0] > 0.0
    # NaN and +inf in x reach only the rows whose blocks read them
    got, want = B.run_ops(ctx, F, nan, bh), B.oracle_ops(Mr, nan, bh)
    hit = np.zeros(n, bool)
    for m in (0, 3, 4):
        hit[m * bs:(m + 1) * bs] = True
    for op in want:
        assert B.same_bits(got[op], want[op]), (bs, op)
        clean = ~hit
        assert np.all(np.isfinite(got[op][clean])) and not np.any(np.isfinite(got[op][:bs])), (bs, op)


@pytest.mark.parametrize("bs,rect_", [(1, 0), (3, 0), (3, 1)])
def test_overflow_is_refused_and_the_context_still_works(ctx, bs, rect_):
    M = edge_matrix(3, top=OVER)
    rows = np.repeat(np.arange(M.nrows), np.diff(M.rowptr))
    first = int(np.flatnonzero(np.abs(M.val) >= OVER)[0])  # the first of several, in storage order: row 0, column 12
    assert (rows[first], M.col[first]) == (0, 12) and np.count_nonzero(np.abs(M.val) >= OVER) == 9
    refs = ctx.refcount()
    h = ctypes.c_void_p()
    col = np.ascontiguousarray(M.col, np.int32)
    rp, val = np.ascontiguousarray(M.rowptr, np.int64), np.ascontiguousarray(M.val, np.float64)
    for base in (0, 1):
        with pytest.raises(PamgError) as e:
            call("pamg_mat_upload_f32", ctx.handle, M.nrows, M.ncols, (rp + base).ctypes.data_as(ctypes.c_void_p),
                 (col + base).ctypes.data_as(ctypes.c_void_p), 0, val.ctypes.data_as(ctypes.c_void_p), base, None, bs,
                 rect_, ctypes.byref(h))
        assert e.value.code == -1 and not h.value, e.value
        assert f"row {rows[first] + base}, column {M.col[first] + base} " in str(e.value), e.value
        assert "infinite binary32" in str(e.value)
    assert ctx.refcount() == refs                         # nothing was allocated
    with pytest.raises(PamgError) as e:                   # the argument checks of the two block uploads
        PSparseMatrix(ctx, to_hcsr(M), block_size=2, value_bits=32)
    assert e.value.code == -1 and "not whole blocks" in str(e.value)
    with pytest.raises(PamgError) as e:
        call("pamg_mat_upload_f32", ctx.handle, M.nrows, M.ncols, rp.ctypes.data_as(ctypes.c_void_p),
             col.ctypes.data_as(ctypes.c_void_p), 0, val.ctypes.data_as(ctypes.c_void_p), 0, None, 5, 0, ctypes.byref(h))
    assert e.value.code == -1 and "outside 1..4" in str(e.value)
    # the context still works: the same matrix with the value just below the bound uploads and multiplies
    ok = edge_matrix(3, top=np.nextafter(OVER, 0.0))
    F = PSparseMatrix(ctx, to_hcsr(ok), block_size=bs, block_rows=1, value_bits=32) if not rect_ else \
        PSparseMatrix(ctx, to_hcsr(ok), block_rows=bs, value_bits=32)
    x = np.random.default_rng(1).standard_normal(ok.nrows)
    assert eq(R.spmv_dev(ctx, F, x), O.spmv(rounded(ok), x))
    assert np.isinf(rn32(OVER)) and rn32(np.nextafter(OVER, 0.0)) == FLT_MAX
    del F
    assert ctx.refcount() == refs


def test_non_finite_values_are_kept(ctx):
    M = B.random_block_spd(5, 2, 3)
    val = M.val.copy()
    val[M.rowptr[4]] = np.inf
    val[M.rowptr[6] + 1] = np.nan
    Mi = O.CSR(M.rowptr, M.col, val, M.ncols)
    F = PSparseMatrix(ctx, to_hcsr(Mi), block_size=2, value_bits=32)
    x = np.random.default_rng(4).standard_normal(M.nrows)
    assert F.f32_storage and B.same_bits(R.spmv_dev(ctx, F, x), O.spmv(rounded(Mi), x))


# ------------------------------------------------------------------------------ declines
def plain_f32(ctx, M):
    return PSparseMatrix(ctx, to_hcsr(M), value_bits=32)


DECLINES = [(B.partial_block, 3, 0), (B.rows_with_different_blocks, 2, 0), (B.unsorted_blocks, 2, 0),
            (R.rect_partial_block, 3, 1), (R.rect_different_blocks, 2, 1), (lambda: B.random_block_spd(65, 2, 3), 1, 0)]


@pytest.mark.parametrize("gen,bs,rect_", DECLINES, ids=["partial_block", "different_block_columns", "descending_blocks",
                                                        "rect_partial_block", "rect_different_block_columns", "bs1"])
def test_declined_matrices_store_the_rounded_values_in_fp64(ctx, gen, bs, rect_):
    M = gen()
    M = O.CSR(M.rowptr, M.col, M.val / 3.0, M.ncols)      # (a third of every value: few are exact in binary32)
    Mr = rounded(M)
    assert np.count_nonzero(Mr.val != M.val) > M.nnz // 2
    kw = {"block_rows": bs} if rect_ else {"block_size": bs}
    F = PSparseMatrix(ctx, to_hcsr(M), value_bits=32, **kw)
    P = PSparseMatrix(ctx, to_hcsr(Mr))
    lay = B.raw_layout(F)
    assert not lay[9] & 65536 and not lay[9] & 32768 and not F.blocked and not F.f32_storage
    assert lay == B.raw_layout(P) and F.stream_bytes == P.stream_bytes
    assert value_bits(F) == 32 and value_bits(P) == 64
    rng = np.random.default_rng(2)
    x = rng.standard_normal(M.ncols)
    want = O.spmv(Mr, x)
    assert eq(R.spmv_dev(ctx, F, x), want) and eq(R.spmv_dev(ctx, P, x), want)
    assert not eq(want, O.spmv(M, x))
    if M.nrows == M.ncols:
        b = rng.standard_normal(M.nrows)
        got, ref, wanted = B.run_ops(ctx, F, x, b), B.run_ops(ctx, P, x, b), B.oracle_ops(Mr, x, b)
        for op in wanted:
            assert eq(got[op], wanted[op]) and eq(got[op], ref[op]), op


def test_python_argument_errors(ctx):
    M = B.random_block_spd(5, 2, 3)
    with pytest.raises(ValueError, match="32 or 64"):
        PSparseMatrix(ctx, to_hcsr(M), value_bits=16)
    with pytest.raises(ValueError, match="value_bits=32 cannot be combined"):
        PSparseMatrix(ctx, to_hcsr(M), value_bits=32, row_perm=np.arange(10)[::-1].copy())


# ------------------------------------------------------------------------------ cycles
MAX_COARSE = 40
_cycles = {}


def cycle_problem(ctx, kind):
    """F: AMGSolver(values="f32"). G: the fp64 solver of round_values(H) with the exact A_0 set as its outer operator.
    "var": the scalar hierarchy with level 0 in block rows; "nodal": a nodal hierarchy, every level in block rows."""
    if kind not in _cycles:
        nodal = kind == "nodal"
        Ao = B.var_matrix(7 if nodal else 8)
        be = pa.SequentialBackend(1)
        params = pa.SAParams(max_coarse=MAX_COARSE, block_size=3) if nodal else pa.SAParams(max_coarse=MAX_COARSE)
        H = pa.build_hierarchy(be, {0: to_hcsr(Ao)}, np.array([0, Ao.nrows], np.int64), params)
        assert H.nlevels >= 3 if not nodal else H.nlevels >= 2
        lay = "all" if nodal else 3
        F = AMGSolver(ctx, H, reorder="off", block_layout=lay, values="f32")
        Hr = round_values(H)
        G = AMGSolver(ctx, Hr, reorder="off", block_layout=lay)
        E = PSparseMatrix(ctx, H.levels[0][0].A, block_size=3)
        G.set_fine_operator(E)
        assert F.values == "f32" and G.values == "f64"
        # F's level 0 is the rounded operator in 4-byte block rows, its fine operator the exact one in 8-byte ones
        assert F.A_dev[0].f32_storage and value_bits(F.A_dev[0]) == 32 and F.fine_operator() is F.A[0]
        assert F.A[0] is not F.A_dev[0] and F.A[0].blocked and not F.A[0].f32_storage and value_bits(F.A[0]) == 64
        assert G.fine_operator() is E and not G.A_dev[0].f32_storage
        for l in range(H.nlevels - 1):
            ops = (F.A_dev[l], F.P[l], F.R[l])
            assert all(value_bits(Q) == 32 for Q in ops)
            if nodal:
                assert all(Q.f32_storage for Q in ops), l
            assert not np.array_equal(Hr.levels[l][0].P.val, H.levels[l][0].P.val)   # (the rounding changes them)
        for Q in (F, G):
            Q.set_block_size(3, levels="all" if nodal else (0,))
        assert F.rho_b == G.rho_b
        xs = O.xstar(Ao.nrows)
        b = PVector(ctx, Ao.nrows)
        mul(b, F.A[0], PVector(ctx, Ao.nrows, 0, xs))
        assert eq(b.own_values(), O.spmv(Ao, xs))                                    # the exact operator
        _cycles[kind] = (F, G, b, Ao, H, Hr)
    return _cycles[kind]


@pytest.mark.parametrize("smoother,nu", B.SMOOTHERS)
@pytest.mark.parametrize("kind", ["var", "nodal"])
def test_cycle_and_pcg_bits(ctx, kind, smoother, nu):
    F, G, b, Ao, _H, _Hr = cycle_problem(ctx, kind)
    n = Ao.nrows
    Bh = np.asfortranarray(np.stack([b.own_values(), O.xstar(n, 0, 7), np.cos(np.arange(n))], axis=1))
    got = {}
    for tag, Q in (("f32", F), ("ref", G)):
        with T.smoother(Q, smoother, nu, ratio=4.0):
            for graph in (True, False):
                Q.set_graph(graph)
                x = Q.new_vector()
                hist = Q.vcycle(x, b, 3, res_hist=True)
                got[tag, "cycle", graph] = (bits(x.own_values()), bits(hist))
                assert Q.graph_state()["captured"] == graph and not Q.graph_state()["failed"]
            Q.set_graph(True)
            X, Bm = Q.new_multivector(3), MultiVector.from_numpy(ctx, Bh)
            Q.vcycle_multi(X, Bm, 3)
            got[tag, "multi"] = bits(X.to_numpy())
            x = Q.new_vector()
            k, hist = Q.pcg(x, b, 1e-8, 60)
            got[tag, "pcg"] = (bits(x.own_values()), k, bits(hist))
            x = Q.new_vector()
            k, hist = Q.pcg(x, b, 1e-8, 60, lookahead=0)
            got[tag, "pcg0"] = (bits(x.own_values()), k, bits(hist))
            X = Q.new_multivector(3)
            ks, hists = Q.pcg_multi(X, Bm, 1e-8, 60)
            got[tag, "pcgm"] = (bits(X.to_numpy()), list(ks), [bits(h) for h in hists])
    for graph in (True, False):
        for i in (0, 1):
            assert np.array_equal(got["f32", "cycle", graph][i], got["ref", "cycle", graph][i]), (kind, smoother, graph, i)
    assert np.array_equal(got["f32", "cycle", True][0], got["f32", "cycle", False][0])
    assert np.array_equal(got["f32", "multi"], got["ref", "multi"])
    assert np.array_equal(got["f32", "multi"][:, 0], got["f32", "cycle", True][0])    # column 0 is the single cycle
    for key in ("pcg", "pcg0"):
        xf, kf, hf = got["f32", key]
        xr, kr, hr = got["ref", key]
        assert kf == kr and 0 < kf < 60 and np.array_equal(hf, hr) and np.array_equal(xf, xr), (kind, smoother, key)
        h = hf.view(np.float64)
        assert h[-1] <= 1e-8 * h[0]
    assert np.array_equal(got["f32", "pcg"][0], got["f32", "pcg0"][0])
    assert np.array_equal(got["f32", "pcg"][2], got["f32", "pcg0"][2])
    xf, kf, hf = got["f32", "pcgm"]
    xr, kr, hr = got["ref", "pcgm"]
    assert kf == kr and np.array_equal(xf, xr) and all(np.array_equal(a, c) for a, c in zip(hf, hr))
    assert kf[0] == got["f32", "pcg"][1] and np.array_equal(xf[:, 0], got["f32", "pcg"][0])


# ------------------------------------------------------------------------------ the outer operator
def test_pcg_starts_from_the_exact_residual(ctx):
    """res_hist[0] = ||b - A x0|| with the exact A (SPEC §S8: 1e-12 relative), which the rounded operator's residual
    misses by far more. x0 = x* + 1e-6 u, u normal: the residual is small, so the 6e-8 relative rounding of the
    entries moves its norm visibly."""
    F, _G, b, Ao, _H, Hr = cycle_problem(ctx, "var")
    n = Ao.nrows
    x0 = O.xstar(n) + 1e-6 * np.random.default_rng(12).standard_normal(n)
    bh = b.own_values()
    exact = np.linalg.norm(O.residual(Ao, x0, bh))
    Ar = rounded(Ao)
    assert np.array_equal(Ar.val, Hr.levels[0][0].A.val)
    other = np.linalg.norm(O.residual(Ar, x0, bh))
    assert abs(other - exact) > 1e-10 * exact, (other, exact)
    for lookahead in (None, 0):
        x = F.new_vector()
        x.set(x0)
        k, hist = F.pcg(x, b, 1e-8, 0, lookahead=lookahead)
        assert k == 0 and abs(hist[0] - exact) <= 1e-12 * exact, (lookahead, hist[0], exact, other)
    X = F.new_multivector(2)
    X.set(np.asfortranarray(np.stack([x0, x0], axis=1)))
    _ks, hists = F.pcg_multi(X, MultiVector.from_numpy(ctx, np.asfortranarray(np.stack([bh, bh], axis=1))), 1e-8, 0)
    assert all(abs(h[0] - exact) <= 1e-12 * exact for h in hists)
    # a stationary vcycle iterates on the rounded A_0: its history is the rounded operator's
    x = F.new_vector()
    x.set(x0)
    hist = F.vcycle(x, b, 1, res_hist=True)
    after = x.own_values()
    want = np.linalg.norm(O.residual(Ar, after, bh))
    assert abs(hist[0] - want) <= 1e-12 * want


def test_pcg_against_a_plain_python_restatement(ctx):
    """SPEC §S8 in Python: the oracle's V-cycle over the rounded levels as M^-1, the oracle's SpMV with the exact A."""
    F, _G, b, Ao, H, Hr = cycle_problem(ctx, "var")
    lps = [Hr.levels[l][0] for l in range(Hr.nlevels)]
    Ho = O.hierarchy_from_levels([lp.A for lp in lps], [lp.P for lp in lps[:-1]], [lp.R for lp in lps[:-1]],
                                 [lp.omega for lp in lps], H.ainv)
    bh = b.own_values()
    x = np.zeros(Ao.nrows)
    r = O.residual(Ao, x, bh)
    nr0 = np.sqrt(r @ r)
    z = Ho.solve(r, 1)
    p, rz, k = z.copy(), r @ z, 0
    while k < 60:
        k += 1
        q = O.spmv(Ao, p)
        alpha = rz / (p @ q)
        x, r = x + alpha * p, r - alpha * q
        if np.sqrt(r @ r) <= 1e-8 * nr0:
            break
        z = Ho.solve(r, 1)
        rz, beta = r @ z, (r @ z) / rz
        p = z + beta * p
    xd = F.new_vector()
    kd, hist = F.pcg(xd, b, 1e-8, 60)
    assert kd == k and 0 < k < 60, (kd, k)
    assert np.linalg.norm(xd.own_values() - x) <= 1e-8 * np.linalg.norm(x)
    assert np.linalg.norm(O.residual(Ao, xd.own_values(), bh)) <= 2e-8 * nr0     # it solves the exact system


def test_set_outer_refusals(ctx):
    F, G, b, Ao, H, _Hr = cycle_problem(ctx, "var")
    small = PSparseMatrix(ctx, to_hcsr(B.var_matrix(3)), block_size=3)
    with pytest.raises(PamgError) as e:
        G.set_fine_operator(small)
    assert e.value.code == -1 and "81 x 81 operator" in str(e.value), e.value
    hp = HostPlan(n_own=Ao.nrows, col0=0, ghost_ids=np.zeros(0, np.int64))
    dp = DevicePlan(ctx, hp)
    foreign = PSparseMatrix(ctx, H.levels[0][0].A, plan=hp, dplan=dp)
    with pytest.raises(PamgError) as e:
        G.set_fine_operator(foreign)
    assert e.value.code == -1 and "column plan" in str(e.value), e.value
    assert G.fine_operator() is not foreign and G.fine_operator() is not small       # the old one stays
    x = G.new_vector()
    k, _hist = G.pcg(x, b, 1e-8, 60)
    assert 0 < k < 60
    # a permuted level 0: the hierarchy refuses an outer operator, the solver says so before it builds one
    Pm = AMGSolver(ctx, H, reorder="on")
    assert Pm.perm[0] is not None
    with pytest.raises(PamgError) as e:
        Pm.set_fine_operator(PSparseMatrix(ctx, H.levels[0][0].A))
    assert e.value.code == -6 and "permutation" in str(e.value), e.value
    with pytest.raises(ValueError, match="reorder='off'"):
        AMGSolver(ctx, H, reorder="on", values="f32")
    # NULL restores level 0's own operator: PCG then solves the rounded system
    S = AMGSolver(ctx, H, reorder="off", block_layout=3, values="f32")
    S.set_fine_operator(None)
    assert S.fine_operator() is S.A_dev[0]
    x = S.new_vector()
    k, hist = S.pcg(x, b, 1e-8, 60)
    bh = b.own_values()
    assert 0 < k < 60 and np.linalg.norm(O.residual(rounded(Ao), x.own_values(), bh)) <= 2e-8 * np.linalg.norm(bh)
