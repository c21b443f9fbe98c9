"""The block-row layout (pamg_mat_upload_blocked, k_rows_bsr) on the GPU, bit for bit against the oracle
(SPEC §S3: a lane walks its node's blocks in stored order, so every row sum keeps the CSR row sum's bits)
and, for the fused point-block smoothers of §S12, against the restatement of tests/test_gpu_block_smoother.py
and against the same calls on the same matrix uploaded through pamg_mat_upload (the two-pass path).

Shapes: one node; 27 nodes (ragged block rows, the slice's tail idle); 125 nodes (one full slice and a
partial one); 343 nodes (two workgroups, the last slice partial). Matrices: elastic3d, a variable-coefficient
L_w (x) B whose values do not repeat, and random block-sparse SPD matrices for block sizes 2 and 4."""
import ctypes

import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd import hcsr as HC
from parallel_amg_amd._lib import PamgError, call, layout_of
from parallel_amg_amd.partitioned import (LocalWorld, PSparseMatrix, PVector, block_chebyshev, block_jacobi, chebyshev,
                                          estimate_lmax_block, jacobi, mul, residual)
from parallel_amg_amd.solver import AMGSolver
import test_gpu_block_smoother as T
from test_gpu_block_smoother import bits, dense_csr, diag_of, differ, to_hcsr

pytestmark = pytest.mark.gpu

OMEGA = 0.6


# ------------------------------------------------------------------------------ matrices
def mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hash_u(i, seed=20240807):
    """SPEC §S2's u_i = (mix64(seed + (i + 1) 0x9E3779B97F4A7C15) >> 11) 2^-53 for an index array."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (i.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        return (mix64(z) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def from_blocks(nb, bs, brow, bcol, bval):
    """CSR of a block matrix given as block triplets (block row, block column, bs x bs values), every block
    whole and each row's columns ascending."""
    order = np.lexsort((bcol, brow))
    brow, bcol, bval = brow[order], bcol[order], bval[order]
    cnt = np.bincount(brow, minlength=nb)
    start = np.concatenate(([0], np.cumsum(cnt)))[:-1]
    rp = np.zeros(nb * bs + 1, np.int64)
    rp[1:] = np.cumsum(np.repeat(cnt * bs, bs))
    k = np.arange(len(brow)) - start[brow]          # the block's place in its block row
    col = np.empty(rp[-1], np.int64)
    val = np.empty(rp[-1], np.float64)
    for d in range(bs):
        base = rp[brow * bs + d] + k * bs
        for e in range(bs):
            col[base + e] = bcol * bs + e
            val[base + e] = bval[:, d, e]
    return O.CSR(rp, col, val, nb * bs)


def var_matrix(n, bs=3):
    """L_w (x) B on an n^3 grid of nodes with 27-point neighbours: diagonal block 39 B, off-diagonal block
    (m, k) = -w B with w = 0.5 + u, u the §S2 hash of the unordered pair; B = 4 I - J."""
    B = 4.0 * np.eye(bs) - np.ones((bs, bs))
    g = np.arange(n)
    z, y, x = (a.reshape(-1) for a in np.meshgrid(g, g, g, indexing="ij"))
    nb = n ** 3
    m = np.arange(nb)
    br, bc, bv = [m], [m], [np.broadcast_to(39.0 * B, (nb, bs, bs))]
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == dy == dz == 0:
                    continue
                ok = (x + dx >= 0) & (x + dx < n) & (y + dy >= 0) & (y + dy < n) & (z + dz >= 0) & (z + dz < n)
                a = m[ok]
                k = a + dx + n * (dy + n * dz)
                w = 0.5 + hash_u(np.minimum(a, k) * nb + np.maximum(a, k))
                br.append(a)
                bc.append(k)
                bv.append((-w)[:, None, None] * B[None])
    return from_blocks(nb, bs, np.concatenate(br), np.concatenate(bc), np.concatenate(bv))


def random_block_spd(nb, bs, seed, deg=4):
    """A random symmetric block pattern (about 2 deg off-diagonal blocks per block row, ragged), off-diagonal
    blocks uniform in (-1, 1) with A_km = A_mk^T, diagonal blocks (1 + the largest absolute row sum) I."""
    rng = np.random.default_rng(seed)
    a = np.repeat(np.arange(nb), deg)
    k = rng.integers(0, nb, len(a))
    keep = a != k
    lo, hi = np.minimum(a, k)[keep], np.maximum(a, k)[keep]
    pairs = np.unique(lo * nb + hi)
    lo, hi = pairs // nb, pairs % nb
    v = rng.uniform(-1.0, 1.0, (len(lo), bs, bs))
    absrow = np.zeros(nb * bs)
    np.add.at(absrow, (lo[:, None] * bs + np.arange(bs)).reshape(-1), np.abs(v).sum(axis=2).reshape(-1))
    np.add.at(absrow, (hi[:, None] * bs + np.arange(bs)).reshape(-1), np.abs(v).sum(axis=1).reshape(-1))
    dg = (1.0 + absrow.max()) * np.broadcast_to(np.eye(bs), (nb, bs, bs))
    m = np.arange(nb)
    return from_blocks(nb, bs, np.concatenate([m, lo, hi]), np.concatenate([m, hi, lo]),
                       np.concatenate([dg, v, v.transpose(0, 2, 1)]))


def one_node(bs):
    a = np.array([[4.0, -1.0, 0.5, 0.25], [-1.0, 3.0, -0.25, 0.5], [0.5, -0.25, 2.0, -0.125],
                  [0.25, 0.5, -0.125, 5.0]])
    return dense_csr(a[:bs, :bs])


# name -> (matrix, block size, nodes)
CASES = {}
for _bs in (2, 3, 4):
    CASES[f"one_node-bs{_bs}"] = (lambda b=_bs: one_node(b), _bs, 1)
for _n in (3, 5, 7):
    CASES[f"elastic3d{_n}-bs3"] = (lambda n=_n: O.generate("elastic3d", n, n, n), 3, _n ** 3)
    CASES[f"var{_n}-bs3"] = (lambda n=_n: var_matrix(n), 3, _n ** 3)
    for _bs in (2, 4):
        CASES[f"random{_n ** 3}-bs{_bs}"] = (lambda n=_n, b=_bs: random_block_spd(n ** 3, b, 100 * n + b), _bs, _n ** 3)
_cases = {}


def upload_blocked(ctx, M, bs):
    return PSparseMatrix(ctx, to_hcsr(M), block_size=bs)


def raw_layout(D):
    out = (ctypes.c_int * 10)()
    call("pamg_mat_layout", D.handle, 0, out)
    return list(out)


def case(ctx, name):
    """The matrix on the host, in the block-row layout and in the layout pamg_mat_upload picks (both with
    block data), random x and b, and a cache of wanted results; built once per case."""
    if name not in _cases:
        gen, bs, nb = CASES[name]
        M = gen()
        assert M.nrows == nb * bs
        D = upload_blocked(ctx, M, bs)
        lay = raw_layout(D)
        assert lay[9] & 32768 and D.blocked and layout_of(D)["bsr"], lay
        assert lay[3] == bs and lay[8] == ((nb + 63) // 64 + 3) // 4, lay
        # the padded block slots: 64 lanes x the widest block row of each slice
        per = np.diff(M.rowptr)[::bs] // bs
        assert lay[4] == 64 * sum(int(per[s:s + 64].max()) for s in range(0, nb, 64)), lay
        assert D.stream_bytes == 4 + lay[4] * (4 + 8 * bs * bs) + 8 * ((nb + 63) // 64 + 1)
        P = PSparseMatrix(ctx, to_hcsr(M))
        assert not layout_of(P)["bsr"] and not P.blocked
        blocks, inv, _rho = HC.block_diag(to_hcsr(M), 0, bs)
        for Q in (D, P):
            Q.set_block_diag(bs, blocks, inv)
        rng = np.random.default_rng(7)
        _cases[name] = (M, D, P, bs, blocks, inv, rng.standard_normal(M.nrows), rng.standard_normal(M.nrows), {})
    return _cases[name]


def run_ops(ctx, D, xh, bh, omega=OMEGA):
    """SpMV, residual and one Jacobi sweep of device matrix D on host vectors."""
    n = D.nrows
    x, b, y = PVector(ctx, n, 0, xh), PVector(ctx, n, 0, bh), PVector(ctx, n)
    mul(y, D, x)
    out = {"spmv": y.own_values()}
    residual(y, D, x, b)
    out["residual"] = y.own_values()
    t = PVector(ctx, n)
    jacobi(x, D, b, t, omega, 1)
    out["jacobi"] = x.own_values()
    return out


def oracle_ops(M, xh, bh, omega=OMEGA):
    return {"spmv": O.spmv(M, xh), "residual": O.residual(M, xh, bh), "jacobi": O.jacobi(M, xh, bh, omega)}


def same_bits(got, want):
    """SPEC §S3, range of the guarantee: the NaN masks agree and every other entry has the same bits."""
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn])


# ------------------------------------------------------------------------------ row operations
@pytest.mark.parametrize("name", list(CASES))
def test_row_ops_bits(ctx, name):
    """SpMV, residual, Jacobi (omega 0.6), the Chebyshev step (pamg_bench_rowop op 6: c1 = c2 = omega over a
    zero x_{k-1}) and a degree-3 polynomial (its steps k >= 1 read a real x_{k-1})."""
    M, D, _P, _bs, _blocks, _inv, xh, bh, _cache = case(ctx, name)
    got, want = run_ops(ctx, D, xh, bh), oracle_ops(M, xh, bh)
    for op in want:
        assert np.array_equal(bits(got[op]), bits(want[op])), (name, op, differ(bits(got[op]), bits(want[op])))
    n = M.nrows
    x, b, y = PVector(ctx, n, 0, xh), PVector(ctx, n, 0, bh), PVector(ctx, n)
    ms = ctypes.c_double()
    call("pamg_bench_rowop", ctx.handle, D.handle, 6, x.handle, b.handle, y.handle, 0.375, 1, ctypes.byref(ms))
    u = O.residual(M, xh, bh)
    step = xh + ((0.375 * (xh - 0.0)) + ((0.375 * u) / diag_of(M)))
    assert np.array_equal(bits(y.own_values()), bits(step)), (name, differ(bits(y.own_values()), bits(step)))
    c1, c2 = T.coeffs_ref(1.6, 4.0, 3)
    t1, t2 = PVector(ctx, n), PVector(ctx, n)
    chebyshev(x, D, b, t1, t2, lmax=1.6, ratio=4.0, degree=3)
    poly = T.scalar_cheb_ref(M, diag_of(M), xh, bh, c1, c2, 3)
    assert np.array_equal(bits(x.own_values()), bits(poly)), (name, differ(bits(x.own_values()), bits(poly)))
    # prolongate-add (pamg_bench_rowop op 3 runs twice: a warm-up and one timed): y <- y + A x from y = b
    yy = PVector(ctx, n, 0, bh)
    x.set(xh)
    call("pamg_bench_rowop", ctx.handle, D.handle, 3, x.handle, None, yy.handle, 0.0, 1, ctypes.byref(ms))
    s = O.spmv(M, xh)
    assert np.array_equal(bits(yy.own_values()), bits((bh + s) + s))


# ------------------------------------------------------------------------------ floating-point edges
EDGE_CASES = ["var5-bs3", "random125-bs2", "random343-bs4", "elastic3d3-bs3"]


@pytest.mark.parametrize("name", EDGE_CASES)
def test_negative_zero_x(ctx, name):
    M, D, _P, _bs, _blocks, _inv, _xh, bh, _cache = case(ctx, name)
    xh = np.full(M.nrows, -0.0)
    for b in (bh, np.zeros(M.nrows)):
        got, want = run_ops(ctx, D, xh, b), oracle_ops(M, xh, b)
        for op in want:
            assert np.array_equal(bits(got[op]), bits(want[op])), (name, op)


@pytest.mark.parametrize("name", EDGE_CASES)
def test_nan_and_inf_reach_only_their_rows(ctx, name):
    """x with one NaN and one +inf at two nodes: the rows whose blocks include neither node carry the
    oracle's finite bits (a padded slot contributes nothing), the others the oracle's NaN mask and bits."""
    M, D, _P, bs, _blocks, _inv, xh, bh, _cache = case(ctx, name)
    nb = M.nrows // bs
    na, ni = nb // 3, (2 * nb) // 3
    xh = xh.copy()
    xh[na * bs + bs - 1] = np.nan
    xh[ni * bs] = np.inf
    rows = np.repeat(np.arange(M.nrows), np.diff(M.rowptr))
    hit = np.zeros(M.nrows, bool)
    hit[rows[np.isin(M.col // bs, (na, ni))]] = True
    assert hit.any() and not hit.all()
    got, want = run_ops(ctx, D, xh, bh), oracle_ops(M, xh, bh)
    for op in want:
        assert same_bits(got[op], want[op]), (name, op)
        clean = ~hit if op != "jacobi" else ~hit & np.isfinite(xh)
        assert np.all(np.isfinite(got[op][clean])), (name, op)
        assert np.array_equal(bits(got[op][clean]), bits(want[op][clean])), (name, op)


@pytest.mark.parametrize("scale", [2.0 ** -900, 2.0 ** 450])
@pytest.mark.parametrize("name", ["var5-bs3", "random125-bs2", "random125-bs4"])
def test_scaled_operator_through_the_jacobi_quotient(ctx, name, scale):
    M, _D, _P, bs, _blocks, _inv, xh, bh, _cache = case(ctx, name)
    Ms = O.CSR(M.rowptr, M.col, M.val * scale, M.ncols)
    D = upload_blocked(ctx, Ms, bs)
    assert raw_layout(D)[9] & 32768
    for b in (bh, bh * scale):
        got, want = run_ops(ctx, D, xh, b), oracle_ops(Ms, xh, b)
        for op in want:
            assert same_bits(got[op], want[op]), (name, scale, op)


# ------------------------------------------------------------------------------ decline cases
def drop_entries(M, pairs):
    keep = np.ones(M.nnz, bool)
    rows = np.repeat(np.arange(M.nrows), np.diff(M.rowptr))
    for i, j in pairs:
        at = np.flatnonzero((rows == i) & (M.col == j))
        assert len(at) == 1
        keep[at] = False
    rp = np.concatenate(([0], np.cumsum(np.bincount(rows[keep], minlength=M.nrows)))).astype(np.int64)
    return O.CSR(rp, M.col[keep].copy(), M.val[keep].copy(), M.ncols)


def partial_block():
    """elastic3d 3^3 with entry (1, 2) of the off-diagonal block (node 0, node 1) and its mirror removed."""
    return drop_entries(O.generate("elastic3d", 3, 3, 3), [(1, 5), (5, 1)])


def rows_with_different_blocks():
    """Four nodes of two unknowns: every row stores its diagonal block whole, row 2 m also the block of node
    m + 1, row 2 m + 1 the block of node m + 2 — equal lengths, whole blocks, different block columns."""
    rng = np.random.default_rng(3)
    rp, col, val = [0], [], []
    for m in range(4):
        for d in range(2):
            other = (m + 1 + d) % 4
            cs = sorted([2 * m, 2 * m + 1, 2 * other, 2 * other + 1])
            col += cs
            val += [8.0 if c == 2 * m + d else float(rng.uniform(-1, 1)) for c in cs]
            rp.append(len(col))
    return O.CSR(np.array(rp, np.int64), np.array(col, np.int64), np.array(val), 8)


def unsorted_blocks():
    """One node row whose two blocks are stored in descending block order (whole blocks, the same in both
    rows): the kernel's walk would not be the stored order, so the layout declines."""
    rp = np.array([0, 4, 8, 10, 12], np.int64)
    col = np.array([2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 2, 3], np.int64)
    val = np.array([0.5, -0.25, 4.0, 1.0, 0.125, 0.75, 1.0, 3.0, 5.0, 0.5, 0.5, 6.0])
    return O.CSR(rp, col, val, 4)


@pytest.mark.parametrize("gen,bs", [(partial_block, 3), (rows_with_different_blocks, 2), (unsorted_blocks, 2)],
                         ids=["partial_block", "different_block_columns", "descending_blocks"])
def test_declined_matrices_upload_in_the_existing_layouts(ctx, gen, bs):
    M = gen()
    D, P = upload_blocked(ctx, M, bs), PSparseMatrix(ctx, to_hcsr(M))
    lay = raw_layout(D)
    assert not lay[9] & 32768 and not D.blocked
    assert lay == raw_layout(P) and D.stream_bytes == P.stream_bytes
    rng = np.random.default_rng(2)
    xh, bh = rng.standard_normal(M.nrows), rng.standard_normal(M.nrows)
    got, want = run_ops(ctx, D, xh, bh), oracle_ops(M, xh, bh)
    for op in want:
        assert np.array_equal(bits(got[op]), bits(want[op])), op


def test_a_part_with_ghost_columns_declines(built):
    """elastic3d 4 on two parts (offsets multiples of 96, whole nodes), each part's level-0 operator uploaded
    blocked with its plan: rows with ghost columns keep today's layouts, and SpMV gives the oracle's bits."""
    n = 4
    Ao = O.generate("elastic3d", n, n, n)
    W = LocalWorld(2)
    try:
        be = pa.SequentialBackend(2)
        A, offs, xs = pa.generate_problem(be, "elastic3d", n)
        H = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=100), device=W.ctxs[0])
        S = [AMGSolver(W.ctxs[p], H, part=p, block_layout=3) for p in range(2)]
        plain = [AMGSolver(W.ctxs[p], H, part=p) for p in range(2)]
        for p in range(2):
            assert S[p].block_layout == {0: 3} and S[p].A_dev[0].n_ghost > 0
            assert not S[p].A_dev[0].blocked
            for st in (0, 1):
                assert layout_of(S[p].A_dev[0], st) == layout_of(plain[p].A_dev[0], st)
        xst = [PVector(W.ctxs[p], S[p].A[0].n_own_cols, S[p].A[0].n_ghost, xs[p]) for p in range(2)]
        y = [PVector(W.ctxs[p], S[p].A[0].nrows) for p in range(2)]
        W.run(lambda p: mul(y[p], S[p].A[0], xst[p]))
        got = np.concatenate([v.own_values() for v in y])
    finally:
        del S, plain
        W.close()
    assert np.array_equal(bits(got), bits(O.spmv(Ao, O.xstar(Ao.nrows))))


# ------------------------------------------------------------------------------ argument errors
def upload_raw(ctx, M, bs, ncols=None):
    h = ctypes.c_void_p()
    col = np.ascontiguousarray(M.col, np.int32)
    rp, val = np.ascontiguousarray(M.rowptr, np.int64), np.ascontiguousarray(M.val, np.float64)
    call("pamg_mat_upload_blocked", ctx.handle, M.nrows, M.ncols if ncols is None else ncols,
         rp.ctypes.data_as(ctypes.c_void_p), col.ctypes.data_as(ctypes.c_void_p), 0,
         val.ctypes.data_as(ctypes.c_void_p), 0, None, bs, ctypes.byref(h))
    return h


def test_argument_errors_leave_the_context_alone(ctx):
    M = O.generate("elastic3d", 3, 3, 3)          # 81 rows
    R = O.CSR(M.rowptr[:79].copy(), M.col[:M.rowptr[78]].copy(), M.val[:M.rowptr[78]].copy(), 81)  # 78 x 81
    refs = ctx.refcount()
    for bad_bs in (5, 0, -1):
        with pytest.raises(PamgError) as e:
            upload_raw(ctx, M, bad_bs)
        assert e.value.code == -1 and "outside 1..4" in str(e.value), e.value
    for bs in (2, 4):
        with pytest.raises(PamgError) as e:
            upload_raw(ctx, M, bs)
        assert e.value.code == -1 and "not whole blocks" in str(e.value), e.value
    with pytest.raises(PamgError) as e:
        upload_raw(ctx, R, 3)
    assert e.value.code == -1 and "must be square" in str(e.value), e.value
    bad = O.CSR(M.rowptr, M.col.copy(), M.val, M.ncols)
    bad.col[5] = 81                                # a column out of range, past the argument checks
    with pytest.raises(PamgError):
        upload_raw(ctx, bad, 3)
    assert ctx.refcount() == refs
    # bs = 1 is pamg_mat_upload
    D1, P = PSparseMatrix(ctx, to_hcsr(M), block_size=1), PSparseMatrix(ctx, to_hcsr(M))
    assert raw_layout(D1) == raw_layout(P) and not raw_layout(D1)[9] & 32768
    h = upload_raw(ctx, R, 1)
    call("pamg_mat_destroy", h)
    del D1, P
    assert ctx.refcount() == refs


# ------------------------------------------------------------------------------ fused block smoothers
BLOCK_CASES = [n for n in CASES if not n.startswith("elastic3d5") and not n.startswith("var3")]


@pytest.mark.parametrize("nsweeps", [1, 3])
@pytest.mark.parametrize("name", BLOCK_CASES)
def test_fused_block_jacobi_bits(ctx, name, nsweeps):
    M, D, P, bs, _blocks, inv, xh, bh, cache = case(ctx, name)
    if "jac" not in cache:
        xs, cache["jac"] = xh, {}
        for k in (1, 2, 3):
            xs = T.block_jacobi_ref(M, inv, bs, xs, bh, T.OMEGA)
            cache["jac"][k] = bits(xs)
    got = []
    for Q in (D, P):
        x, b, t = Q.new_input_vector(), PVector(ctx, M.nrows, 0, bh), Q.new_input_vector()
        x.set(xh)
        block_jacobi(x, Q, b, t, T.OMEGA, nsweeps)
        got.append(bits(x.own_values()))
        assert np.array_equal(bits(b.own_values()), bits(bh))
    assert np.array_equal(got[0], cache["jac"][nsweeps]), differ(got[0], cache["jac"][nsweeps])
    assert np.array_equal(got[0], got[1]), "the fused pass and the two-pass path differ"


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
@pytest.mark.parametrize("name", BLOCK_CASES)
def test_fused_block_chebyshev_bits(ctx, name, degree):
    M, D, P, bs, _blocks, inv, xh, bh, cache = case(ctx, name)
    key = ("cheb", degree)
    if key not in cache:
        c1, c2 = T.coeffs_ref(T.LMAX, T.RATIO, degree)
        cache[key] = bits(T.block_cheb_ref(M, inv, bs, xh, bh, c1, c2, degree))
    got = []
    for Q in (D, P):
        x, b = Q.new_input_vector(), PVector(ctx, M.nrows, 0, bh)
        x.set(xh)
        t1, t2 = Q.new_input_vector(), Q.new_input_vector()
        block_chebyshev(x, Q, b, t1, t2, lmax=T.LMAX, ratio=T.RATIO, degree=degree)
        got.append(bits(x.own_values()))
    assert np.array_equal(got[0], cache[key]), differ(got[0], cache[key])
    assert np.array_equal(got[0], got[1]), "the fused pass and the two-pass path differ"


@pytest.mark.parametrize("name", BLOCK_CASES)
def test_block_estimate_on_a_block_row_matrix(ctx, name):
    M, D, _P, bs, blocks, inv, _xh, _bh, _cache = case(ctx, name)
    lam_w, v_w, y_w = T.block_estimate_ref(M, blocks, inv, bs, O.xstar(M.nrows, 0, T.SEED), T.STEPS)
    v, y = D.new_input_vector(), D.new_output_vector()
    v.fill_xstar(0, T.SEED)
    lam = estimate_lmax_block(D, v, y, T.STEPS, all_parts=False)
    assert np.array_equal(bits(v.own_values()), bits(v_w))
    assert np.array_equal(bits(y.own_values()), bits(y_w))
    np.testing.assert_allclose(lam, lam_w, rtol=4e-12)


def test_other_block_size_takes_two_passes(ctx):
    """Block data of another size than the layout's (blocks of 2 on a block-row matrix of 4): the sweep is
    the residual pass plus the block pass, with the restatement's bits."""
    M, _D, _P, _bs, _blocks, _inv, xh, bh, _cache = case(ctx, "random125-bs4")
    D = upload_blocked(ctx, M, 4)
    assert raw_layout(D)[9] & 32768
    blocks, inv, _ = HC.block_diag(to_hcsr(M), 0, 2)
    D.set_block_diag(2, blocks, inv)
    x, b, t = D.new_input_vector(), PVector(ctx, M.nrows, 0, bh), D.new_input_vector()
    x.set(xh)
    block_jacobi(x, D, b, t, T.OMEGA, 2)
    want = T.block_jacobi_ref(M, inv, 2, T.block_jacobi_ref(M, inv, 2, xh, bh, T.OMEGA), bh, T.OMEGA)
    assert np.array_equal(bits(x.own_values()), bits(want))


# ------------------------------------------------------------------------------ cycles
MAX_COARSE = 40
_problems = {}


def host_problem(kind):
    be = pa.SequentialBackend(1)
    if kind == "elastic3d":
        Ah, offs, _xs = pa.generate_problem(be, "elastic3d", 8)
        Ao = O.generate("elastic3d", 8, 8, 8)
    else:
        Ao = var_matrix(8)
        Ah, offs = {0: to_hcsr(Ao)}, np.array([0, Ao.nrows], np.int64)
    return be, Ah, offs, Ao


def problem(ctx, kind):
    if kind not in _problems:
        be, Ah, offs, Ao = host_problem(kind)
        H = pa.build_hierarchy(be, Ah, offs, pa.SAParams(max_coarse=MAX_COARSE), device=ctx)
        assert H.nlevels >= 3
        S = AMGSolver(ctx, H, block_layout=3)
        P = AMGSolver(ctx, H)
        assert S.A_dev[0].blocked and raw_layout(S.A_dev[0])[3] == 3 and not P.A_dev[0].blocked
        assert S.L == P.L == H.nlevels
        for Q in (S, P):
            Q.set_block_size(3)
        bo = O.spmv(Ao, O.xstar(Ao.nrows))
        b = PVector(ctx, Ao.nrows)
        mul(b, S.A[0], PVector(ctx, Ao.nrows, 0, O.xstar(Ao.nrows)))
        assert np.array_equal(bits(b.own_values()), bits(bo))
        Ho = O.setup(Ao, max_coarse=MAX_COARSE)
        assert Ho.nlevels == H.nlevels
        rho_b = HC.block_diag(to_hcsr(Ho.A[0]), 0, 3)[2]
        nl = Ho.nlevels - 1
        lmax = [rho_b] + list(Ho.rho[1:nl])
        omega = [4.0 / (3.0 * rho_b)] + list(Ho.omega[1:nl])
        block = {k: T.CycleRef(Ho, k, {0: 3}, omega, lmax) for k in ("jacobi", "chebyshev")}
        scalar = T.CycleRef(Ho, "chebyshev", {}, list(Ho.omega[:nl]), list(Ho.rho[:nl]))
        _problems[kind] = (S, P, b, bo, Ho, block, scalar, {})
    return _problems[kind]


SMOOTHERS = [("jacobi", (1, 1)), ("chebyshev", (2, 2)), ("block_jacobi", (1, 1)), ("block_chebyshev", (2, 2))]


def wanted(kind, nu, bo, Ho, block, scalar, cache):
    """(x, history) of 3 cycles and (x, iterations) of PCG to 1e-8: the oracle's for "jacobi", the restatement's
    for the others."""
    if (kind, nu) not in cache:
        if kind == "jacobi":
            Ho.set_sweeps(*nu)
            xc, hc = Ho.solve(bo, 3, res_hist=True)
            xp, kp, hp = Ho.pcg(bo, 1e-8, 60)
            Ho.set_sweeps(1, 1)
            cache["pcg_hist"] = hp
        else:
            ref = scalar if kind == "chebyshev" else block[kind[len("block_"):]]
            xc, hc = ref.solve(bo, 3, *nu)
            xp, kp = ref.pcg(bo, 1e-8, 60, *nu)
        cache[(kind, nu)] = (xc, hc, xp, kp)
    return cache[(kind, nu)]


@pytest.mark.parametrize("kind,nu", SMOOTHERS)
@pytest.mark.parametrize("prob", ["elastic3d", "var"])
def test_cycle_and_pcg_bits(ctx, prob, kind, nu):
    """Three V-cycles (graph replay on and off) and PCG (host scalars and device-resident, lookahead 0) with
    level 0 in the block-row layout: x, the iteration counts and the histories equal the reference's and
    those of a solver built without block_layout."""
    S, P, b, bo, Ho, block, scalar, cache = problem(ctx, prob)
    xc, hc, xp, kp = wanted(kind, nu, bo, Ho, block, scalar, cache)
    got = {}
    for tag, Q in (("bsr", S), ("plain", P)):
        with T.smoother(Q, kind, nu, ratio=4.0):
            for graph in (True, False):
                Q.set_graph(graph)
                x = Q.new_vector()
                hist = Q.vcycle(x, b, 3, res_hist=True)
                got[tag, "cycle", graph] = (bits(x.own_values()), bits(hist))
                assert Q.graph_state()["captured"] == graph and not Q.graph_state()["failed"]
            Q.set_graph(True)
            x = Q.new_vector()
            k, hist = Q.pcg(x, b, 1e-8, 60)
            got[tag, "pcg"] = (bits(x.own_values()), k, bits(hist))
            x0 = Q.new_vector()
            k0, hist0 = Q.pcg(x0, b, 1e-8, 60, lookahead=0)
            got[tag, "pcg0"] = (bits(x0.own_values()), k0, bits(hist0))
    for graph in (True, False):
        xb, hb = got["bsr", "cycle", graph]
        assert np.array_equal(xb, bits(xc)), (prob, kind, graph, differ(xb, bits(xc)))
        np.testing.assert_allclose(hb.view(np.float64), hc, rtol=1e-12)
        assert np.array_equal(xb, got["plain", "cycle", graph][0])
        assert np.array_equal(hb, got["plain", "cycle", graph][1])
    for key in ("pcg", "pcg0"):
        xb, k, hb = got["bsr", key]
        assert k == kp, (prob, kind, key, k, kp)
        h = hb.view(np.float64)
        assert h[-1] <= 1e-8 * h[0]
        if kind == "jacobi":  # (the oracle's history; the sums of a device dot product take another tree)
            np.testing.assert_allclose(h, cache["pcg_hist"], rtol=1e-6)
        assert np.linalg.norm(xb.view(np.float64) - xp) <= 1e-8 * np.linalg.norm(xp)
        assert np.array_equal(xb, got["plain", key][0]) and k == got["plain", key][1]
        assert np.array_equal(hb, got["plain", key][2])
    assert np.array_equal(got["bsr", "pcg"][0], got["bsr", "pcg0"][0])
    assert np.array_equal(got["bsr", "pcg"][2], got["bsr", "pcg0"][2])


def test_estimated_bounds_and_set_block_size_work_on_top(ctx):
    """set_smoother(lmax="estimate") on a block-row level 0: the bounds of the solver without block_layout."""
    S, P, b, _bo, _Ho, _block, _scalar, _cache = problem(ctx, "var")
    out = {}
    for tag, Q in (("bsr", S), ("plain", P)):
        with T.smoother(Q, "block_chebyshev", (2, 2), ratio=4.0, lmax="estimate"):
            x = Q.new_vector()
            k, hist = Q.pcg(x, b, 1e-8, 60)
            out[tag] = (list(Q.lmax), k, bits(x.own_values()))
    assert out["bsr"][0] == out["plain"][0] and out["bsr"][1] == out["plain"][1]
    assert np.array_equal(out["bsr"][2], out["plain"][2])
