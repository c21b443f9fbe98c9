"""Several right-hand sides (SPEC §S13) on the GPU: a multi-column operation is k independent single-column
operations, so column c of every result must carry the bits of the single-column call on column c — and,
through it, the oracle's (row operations, the Jacobi cycle) or the restatement's of
tests/test_gpu_block_smoother.py (Chebyshev, the point-block smoothers).

Row operations run on block-row matrices of 1, 27, 65 and 257 nodes (a single lane; less than a slice; one
lane in a second slice; past a workgroup of four slices) with ragged block rows, for k = 1, 2, 3, 4, 5, 8
columns — the launch chunks 1, 2, 2+1, 4, 4+1, 4+4 of csrc/multi_cols.h. Cycles and PCG run on the
variable-coefficient operator of tests/test_gpu_bsr.py at 5^3, 6^3 and 7^3 nodes."""
import ctypes

import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd import hcsr as HC
from parallel_amg_amd._lib import PamgError, call, layout_of
from parallel_amg_amd.hierarchy import spmv_host
from parallel_amg_amd.partitioned import (LocalWorld, MultiVector, PVector, block_jacobi, jacobi, mul, residual,
                                          residual_multi, spmm)
from parallel_amg_amd.solver import AMGSolver
import test_gpu_block_smoother as T
import test_gpu_bsr as B
from test_gpu_block_smoother import bits, diag_of, differ, to_hcsr
from test_gpu_bsr import one_node, oracle_ops, random_block_spd, same_bits, upload_blocked, var_matrix, wanted

pytestmark = pytest.mark.gpu

OMEGA = 0.6
CHEB = 0.375   # c1 = c2 of the Chebyshev step and the block Chebyshev step of pamg_bench_rowop_multi
KMAX = 8


def rowop(ctx, D, op, X, Bv, Y, omega=0.0):
    ms = ctypes.c_double()
    call("pamg_bench_rowop_multi", ctx.handle, D.handle, op, X.handle, Bv.handle if Bv is not None else None, Y.handle,
         float(omega), 1, ctypes.byref(ms))
    return Y.to_numpy()


def eq(got, want):
    return np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------------------ 1. row operations
NODES = (1, 27, 65, 257)
_row_cases = {}


def row_case(ctx, bs, nb):
    """A block-row matrix with block data, 8 random columns of x and b, and the wanted result of every
    operation for every column (computed once, never changed)."""
    if (bs, nb) not in _row_cases:
        M = one_node(bs) if nb == 1 else random_block_spd(nb, bs, 1000 * bs + nb)
        n = M.nrows
        assert n == nb * bs
        D = upload_blocked(ctx, M, bs)
        assert layout_of(D)["bsr"] and D.blocked
        if nb > 1:  # ragged block rows inside a slice: padded slots occur
            per = np.diff(M.rowptr)[::bs] // bs
            assert per[:64].min() < per[:64].max()
        blocks, inv, _rho = HC.block_diag(to_hcsr(M), 0, bs)
        D.set_block_diag(bs, blocks, inv)
        rng = np.random.default_rng(11 * bs + nb)
        xh, bh = rng.standard_normal((n, KMAX)), rng.standard_normal((n, KMAX))
        d = diag_of(M)
        want = {k: np.empty((n, KMAX)) for k in ("spmv", "residual", "jacobi", "cheb", "prolong", "bjac", "bcheb")}
        for c in range(KMAX):
            x, b = xh[:, c], bh[:, c]
            ops = oracle_ops(M, x, b, OMEGA)
            for k in ("spmv", "residual", "jacobi"):
                want[k][:, c] = ops[k]
            u = ops["residual"]
            want["cheb"][:, c] = x + ((CHEB * (x - 0.0)) + ((CHEB * u) / d))
            # prolongate-add runs twice (a warm-up and one timed launch) from y = b
            want["prolong"][:, c] = (b + ops["spmv"]) + ops["spmv"]
            want["bjac"][:, c] = T.block_jacobi_ref(M, inv, bs, x, b, OMEGA)
            v = CHEB * T.block_apply(inv, u, bs)
            want["bcheb"][:, c] = x + ((CHEB * (x - 0.0)) + v)
        for w in want.values():
            w.setflags(write=False)
        _row_cases[bs, nb] = (M, D, xh, bh, want)
    return _row_cases[bs, nb]


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("nb", NODES)
@pytest.mark.parametrize("bs", [2, 3, 4])
def test_row_ops_bits(ctx, bs, nb, k):
    M, D, xh, bh, want = row_case(ctx, bs, nb)
    n = M.nrows
    X, Bv = MultiVector.from_numpy(ctx, xh[:, :k]), MultiVector.from_numpy(ctx, bh[:, :k])
    assert X.stride % 32 == 0 and X.stride >= n
    Y = MultiVector(ctx, n, k)
    got = {"spmv": spmm(Y, D, X).to_numpy()}
    assert eq(rowop(ctx, D, 0, X, None, Y), got["spmv"])
    nrm = residual_multi(Y, D, X, Bv, with_norm=True)
    got["residual"] = Y.to_numpy()
    assert eq(rowop(ctx, D, 1, X, Bv, Y), got["residual"])
    got["jacobi"] = rowop(ctx, D, 2, X, Bv, Y, OMEGA)
    got["cheb"] = rowop(ctx, D, 6, X, Bv, Y, CHEB)
    Y.set(bh[:, :k])
    got["prolong"] = rowop(ctx, D, 3, X, None, Y)
    got["bjac"] = rowop(ctx, D, 7, X, Bv, Y, OMEGA)
    got["bcheb"] = rowop(ctx, D, 8, X, Bv, Y, CHEB)
    for op, g in got.items():
        for c in range(k):
            assert eq(g[:, c], want[op][:, c]), (bs, nb, k, op, c, differ(bits(g[:, c]), bits(want[op][:, c])))
    assert eq(X.to_numpy(), xh[:, :k]) and eq(Bv.to_numpy(), bh[:, :k])
    # the single-column calls on column views: the same bits, and the norms of pamg_residual
    W, t = MultiVector(ctx, n, k), PVector(ctx, n)
    for c in range(k):
        xv, bv, wv = X.column(c), Bv.column(c), W.column(c)
        assert eq(mul(wv, D, xv).own_values(), got["spmv"][:, c])
        assert bits(residual(wv, D, xv, bv, with_norm=True)) == bits(nrm[c])
        assert eq(wv.own_values(), got["residual"][:, c])
    Xc = MultiVector.from_numpy(ctx, xh[:, :k])
    for c in range(k):
        assert eq(jacobi(Xc.column(c), D, Bv.column(c), t, OMEGA, 1).own_values(), got["jacobi"][:, c])
    Xc.set(xh[:, :k])
    for c in range(k):
        assert eq(block_jacobi(Xc.column(c), D, Bv.column(c), t, OMEGA, 1).own_values(), got["bjac"][:, c])
    # the other columns of the multi-vector kept their values through the single-column calls
    assert eq(W.to_numpy(), got["residual"])


# ------------------------------------------------------------------------------ 2. columns do not mix
@pytest.mark.parametrize("bs,nb", [(2, 65), (3, 65), (4, 257)])
def test_columns_do_not_mix(ctx, bs, nb):
    """Column 1 carries a NaN and a +inf, column 2 is -0.0 everywhere: columns 0 and 3 keep the oracle's bits,
    column 2 the oracle's for a -0.0 vector, and column 1 is non-finite in the oracle's rows only."""
    M, D, xh, bh, _want = row_case(ctx, bs, nb)
    n, k = M.nrows, 4
    xs = xh[:, :k].copy()
    xs[(nb // 3) * bs + bs - 1, 1] = np.nan
    xs[((2 * nb) // 3) * bs, 1] = np.inf
    xs[:, 2] = -0.0
    X, Bv, Y = MultiVector.from_numpy(ctx, xs), MultiVector.from_numpy(ctx, bh[:, :k]), MultiVector(ctx, n, k)
    got = {"spmv": spmm(Y, D, X).to_numpy(), "residual": residual_multi(Y, D, X, Bv).to_numpy(),
           "jacobi": rowop(ctx, D, 2, X, Bv, Y, OMEGA), "bjac": rowop(ctx, D, 7, X, Bv, Y, OMEGA)}
    inv = HC.block_diag(to_hcsr(M), 0, bs)[1]
    t, W = PVector(ctx, n), MultiVector(ctx, n, k)
    for c in range(k):
        want = oracle_ops(M, xs[:, c], bh[:, c], OMEGA)
        want["bjac"] = T.block_jacobi_ref(M, inv, bs, xs[:, c], bh[:, c], OMEGA)
        for op in got:
            g = got[op][:, c]
            if c == 1:
                assert same_bits(g, want[op]), (op, c)
                assert not np.all(np.isfinite(g)) and np.any(np.isfinite(g))
            else:
                assert np.all(np.isfinite(g)) and eq(g, want[op]), (op, c)
        # ... exactly where the single-column call is
        wv = mul(W.column(c), D, X.column(c)).own_values()
        assert np.array_equal(np.isfinite(wv), np.isfinite(got["spmv"][:, c])) and same_bits(got["spmv"][:, c], wv)
        jv = jacobi(MultiVector.from_numpy(ctx, xs).column(c), D, Bv.column(c), t, OMEGA, 1).own_values()
        assert np.array_equal(np.isfinite(jv), np.isfinite(got["jacobi"][:, c])) and same_bits(got["jacobi"][:, c], jv)


# ------------------------------------------------------------------------------ 3. the column loop
def test_fallback_layouts_loop_over_the_columns(ctx):
    """Operators without the block-row layout (poisson3d 8^3: symmetric, ELL and tile layouts; a matrix
    pamg_mat_upload_blocked declines) with k = 3: every column equals the single-column call."""
    be = pa.SequentialBackend(1)
    A, offs, _xs = pa.generate_problem(be, "poisson3d", 8)
    H = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=40), device=ctx)
    assert H.nlevels >= 2
    S = AMGSolver(ctx, H, reorder="off")
    assert not any(layout_of(a)["bsr"] for a in S.A_dev)
    assert S.graph_state()["enabled"]
    n, k = S.A_dev[0].nrows, 3
    rng = np.random.default_rng(5)
    xh, bh = rng.standard_normal((n, k)), rng.standard_normal((n, k))
    Md = upload_blocked(ctx, B.partial_block(), 3)
    assert not layout_of(Md)["bsr"] and not Md.blocked
    for Q in (S.A[0], Md):
        m = Q.nrows
        X, Y = MultiVector.from_numpy(ctx, xh[:m]), MultiVector(ctx, m, k)
        got = spmm(Y, Q, X).to_numpy()
        for c in range(k):
            assert eq(got[:, c], mul(PVector(ctx, m), Q, PVector(ctx, m, 0, xh[:m, c])).own_values())
    for ncycles in (1, 3):
        X, Bv = S.new_multivector(k), MultiVector.from_numpy(ctx, bh)
        X.set(xh)
        hist = S.vcycle_multi(X, Bv, ncycles, res_hist=True)
        got = X.to_numpy()
        for c in range(k):
            x, b = PVector(ctx, n, 0, xh[:, c]), PVector(ctx, n, 0, bh[:, c])
            h1 = S.vcycle(x, b, ncycles, res_hist=True)
            assert eq(got[:, c], x.own_values()), (ncycles, c)
            assert eq(hist[:, c], h1), (ncycles, c)


# ------------------------------------------------------------------------------ 4. cycles
MAX_COARSE = 40
SMOOTHERS = ["jacobi", "chebyshev", "block_jacobi", "block_chebyshev"]
_problems = {}


def problem(ctx, n):
    """var_matrix(n) with level 0 in the block-row layout, four right-hand sides (A x*, random, A 1, A x* of
    another seed) and the reference objects of tests/test_gpu_bsr.py's problem()."""
    if n not in _problems:
        Ao = var_matrix(n)
        be = pa.SequentialBackend(1)
        Ah, offs = {0: to_hcsr(Ao)}, np.array([0, Ao.nrows], np.int64)
        H = pa.build_hierarchy(be, Ah, offs, pa.SAParams(max_coarse=MAX_COARSE), device=ctx)
        assert H.nlevels >= 2
        S = AMGSolver(ctx, H, reorder="off", block_layout=3)
        assert S.A_dev[0].blocked and layout_of(S.A_dev[0])["bsr"]
        S.set_block_size(3)
        Ho = O.setup(Ao, max_coarse=MAX_COARSE)
        assert Ho.nlevels == H.nlevels
        rho_b = HC.block_diag(to_hcsr(Ho.A[0]), 0, 3)[2]
        nl = Ho.nlevels - 1
        lmax = [rho_b] + list(Ho.rho[1:nl])
        omega = [4.0 / (3.0 * rho_b)] + list(Ho.omega[1:nl])
        block = {k: T.CycleRef(Ho, k, {0: 3}, omega, lmax) for k in ("jacobi", "chebyshev")}
        scalar = T.CycleRef(Ho, "chebyshev", {}, list(Ho.omega[:nl]), list(Ho.rho[:nl]))
        m = Ao.nrows
        bh = np.stack([O.spmv(Ao, O.xstar(m)), np.random.default_rng(n).standard_normal(m), O.spmv(Ao, np.ones(m)),
                       O.spmv(Ao, O.xstar(m, 0, 77))], axis=1)
        bh.setflags(write=False)
        _problems[n] = (S, Ao, bh, Ho, block, scalar, {})
    return _problems[n]


def reference(prob, kind, nu, c):
    """Column c's wanted() of tests/test_gpu_bsr.py — x and history of 3 cycles — and x after one cycle."""
    _S, _Ao, bh, Ho, block, scalar, cache = prob
    if (kind, nu, c) not in cache:
        b = bh[:, c]
        x3, h3, _xp, _kp = wanted(kind, nu, b, Ho, block, scalar, {})
        if kind == "jacobi":
            Ho.set_sweeps(*nu)
            x1 = Ho.solve(b, 1)
            Ho.set_sweeps(1, 1)
        else:
            ref = scalar if kind == "chebyshev" else block[kind[len("block_"):]]
            x1, _h = ref.solve(b, 1, *nu)
        cache[kind, nu, c] = (np.asarray(x1), np.asarray(x3), np.asarray(h3))
    return cache[kind, nu, c]


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("nu", [(1, 1), (2, 3)])
@pytest.mark.parametrize("kind", SMOOTHERS)
@pytest.mark.parametrize("n", [5, 6, 7])
def test_cycle_bits(ctx, n, kind, nu, k):
    prob = problem(ctx, n)
    S, Ao, bh = prob[:3]
    m = Ao.nrows
    Bv = MultiVector.from_numpy(ctx, bh[:, :k])
    with T.smoother(S, kind, nu, ratio=4.0):
        single = {}
        for c in range(k):
            for ncycles in (1, 3):
                x = S.new_vector()
                h = S.vcycle(x, Bv.column(c), ncycles, res_hist=True)
                single[c, ncycles] = (x.own_values(), h)
        for graph in (True, False):
            S.set_graph(graph)
            for ncycles in (1, 3):
                X = S.new_multivector(k)
                hist = S.vcycle_multi(X, Bv, ncycles, res_hist=True)
                got = X.to_numpy()
                assert not S.graph_state()["failed"]
                for c in range(k):
                    x1, x3, h3 = reference(prob, kind, nu, c)
                    want = x1 if ncycles == 1 else x3
                    assert eq(got[:, c], want), (n, kind, nu, k, graph, ncycles, c, differ(bits(got[:, c]), bits(want)))
                    assert eq(got[:, c], single[c, ncycles][0]), (graph, ncycles, c)
                    assert eq(hist[:, c], single[c, ncycles][1]), (graph, ncycles, c)
                    np.testing.assert_allclose(hist[:, c], h3[:ncycles], rtol=1e-12)
        # other multi-vectors of the same k (another graph key), the columns in another order, no history
        S.set_graph(True)
        order = list(range(k))[::-1]
        B2, X2 = MultiVector.from_numpy(ctx, bh[:, order]), S.new_multivector(k)
        S.vcycle_multi(X2, B2, 3)
        got = X2.to_numpy()
        for j, c in enumerate(order):
            assert eq(got[:, j], single[c, 3][0]), (j, c)
    assert eq(Bv.to_numpy(), bh[:, :k]) and m == X2.n_own


# ------------------------------------------------------------------------------ 5. PCG
# Per (n, smoother), all V(1,1): the rtol (of 1e-8, 1e-4, 1e-12, the first that serves) at which the iteration
# counts of columns 0, 2 and 3 (A x*, A 1, A x* of another seed) are not all equal, and the counts pamg_pcg
# gave there on an MI355X — so that a column that has stopped rides along with running ones. (Under block
# Chebyshev V(2,2) the three counts are equal at every one of the three tolerances: 5, 3 and 7 iterations.)
PCG_CASES = {
    (5, "jacobi"): (1e-8, [17, 1, 17]), (6, "jacobi"): (1e-8, [17, 1, 18]), (7, "jacobi"): (1e-8, [18, 16, 18]),
    (5, "chebyshev"): (1e-8, [16, 12, 15]), (6, "chebyshev"): (1e-8, [16, 13, 16]),
    (7, "chebyshev"): (1e-8, [16, 15, 16]),
    (5, "block_jacobi"): (1e-12, [11, 11, 10]), (6, "block_jacobi"): (1e-8, [7, 8, 8]),
    (7, "block_jacobi"): (1e-12, [11, 12, 12]),
    (5, "block_chebyshev"): (1e-4, [3, 4, 3]), (6, "block_chebyshev"): (1e-4, [3, 4, 3]),
    (7, "block_chebyshev"): (1e-4, [3, 4, 3]),
}


@pytest.mark.parametrize("kind", SMOOTHERS)
@pytest.mark.parametrize("n", [5, 6, 7])
def test_pcg_columns_stop_on_their_own(ctx, n, kind):
    prob = problem(ctx, n)
    S, Ao, bh = prob[:3]
    m, k, maxit, nu = Ao.nrows, 4, 60, (1, 1)
    bs = bh.copy()
    bs[:, 1] = 0.0          # column 1 stops at once: ||r_0|| = 0
    Bv = MultiVector.from_numpy(ctx, bs)
    Ah = to_hcsr(Ao)
    rtol, seen = PCG_CASES[n, kind]
    with T.smoother(S, kind, nu, ratio=4.0):
        single = {}
        for c in range(k):
            x = S.new_vector()
            it, h = S.pcg(x, Bv.column(c), rtol, maxit)
            single[rtol, c] = (it, h, x.own_values())
        counts = [single[rtol, c][0] for c in (0, 2, 3)]
        print("pcg iteration counts of columns 0, 2, 3:", n, kind, rtol, counts, "recorded", seen)
        assert len(set(counts)) >= 2, (n, kind, rtol, counts)
        for rtol in (rtol,):
            X = S.new_multivector(k)
            its, hists = S.pcg_multi(X, Bv, rtol, maxit)
            got = X.to_numpy()
            assert its[1] == 0 and eq(got[:, 1], np.zeros(m)) and len(hists[1]) == 1 and hists[1][0] == 0.0
            for c in range(k):
                it, h, x = single[rtol, c]
                assert its[c] == it and eq(hists[c], h) and eq(got[:, c], x), (n, kind, rtol, c, its[c], it)
                if c != 1:
                    assert 0 < it < maxit and h[-1] <= rtol * h[0]
                    # against a host residual, independent of the device path
                    r = bs[:, c] - spmv_host(Ah, got[:, c])
                    assert np.linalg.norm(r) <= 10 * rtol * np.linalg.norm(bs[:, c]), (c, np.linalg.norm(r))
            # a column that stopped early is not written by the later iterations of the others: a run cut
            # at its count leaves the same x
            first = int(min(its[c] for c in (0, 2, 3)))
            Xc = S.new_multivector(k)
            its_c, _h = S.pcg_multi(Xc, Bv, rtol, first)
            early = [c for c in (0, 2, 3) if its[c] == first]
            assert early and all(its_c[c] == first for c in (0, 2, 3))
            for c in early:
                assert eq(Xc.to_numpy()[:, c], got[:, c]), c
        for cut in (1, 0):
            X = S.new_multivector(k)
            its, hists = S.pcg_multi(X, Bv, 1e-8, cut)
            got = X.to_numpy()
            for c in range(k):
                x = S.new_vector()
                it, h = S.pcg(x, Bv.column(c), 1e-8, cut)
                assert its[c] == it and eq(hists[c], h) and eq(got[:, c], x.own_values()), (cut, c)
                assert it == (0 if c == 1 else cut)


# ------------------------------------------------------------------------------ 6. errors and state
def refused(code, fn, *args, **kw):
    with pytest.raises(PamgError) as e:
        fn(*args, **kw)
    assert e.value.code == code and str(e.value).split(": ", 1)[1].strip(), e.value


def test_errors_leave_the_context_alone(ctx):
    prob = problem(ctx, 5)
    S, Ao, bh = prob[:3]
    D, n = S.A_dev[0], Ao.nrows
    X3, B3, B4 = MultiVector(ctx, n, 3), MultiVector.from_numpy(ctx, bh[:, :3]), MultiVector.from_numpy(ctx, bh)
    short = MultiVector(ctx, n - 3, 3)
    refs = ctx.refcount()
    for k in (0, 9, -1):
        refused(-1, MultiVector, ctx, n, k)
    refused(-1, X3.column, 3)
    refused(-1, X3.column, -1)
    for fn in (S.vcycle_multi, S.pcg_multi):
        refused(-1, fn, X3, B4)          # other columns than B
        refused(-1, fn, X3, X3)          # X aliasing B
        refused(-1, fn, short, B3)       # another shape
    refused(-1, spmm, X3, D, B4)
    refused(-1, spmm, X3, D, X3)
    refused(-1, spmm, short, D, B3)
    refused(-1, residual_multi, X3, D, B3, B4)
    refused(-1, residual_multi, X3, D, X3, B3)
    refused(-1, rowop, ctx, D, 5, B3, B3, X3)      # no such op
    refused(-1, rowop, ctx, D, 1, B3, None, X3)    # the residual needs B
    refused(-1, rowop, ctx, D, 0, B3, None, B3)    # X aliasing Y
    assert ctx.refcount() == refs
    # a column view aliases its multi-vector
    v = B3.column(1)
    assert ctx.refcount() == refs + 1
    w = B3.column(1)
    with pytest.raises(PamgError) as e:           # two views of one column: X aliases Y
        call("pamg_spmm", ctx.handle, D.handle, v.handle, w.handle)
    assert e.value.code == -1 and ctx.refcount() == refs + 2
    del v, w
    assert ctx.refcount() == refs
    assert eq(B3.to_numpy(), bh[:, :3])            # destroying the view freed nothing


def test_permuted_hierarchy_and_several_parts_are_state_errors(ctx):
    be = pa.SequentialBackend(1)
    A, offs, _xs = pa.generate_problem(be, "poisson3d", 8)
    H = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=40), device=ctx)
    S = AMGSolver(ctx, H, reorder="on")
    assert 0 in S.reordered
    n = S.A_dev[0].nrows
    X, Bv = MultiVector(ctx, n, 2), MultiVector(ctx, n, 2)
    refs = ctx.refcount()
    refused(-6, S.vcycle_multi, X, Bv)
    refused(-6, S.pcg_multi, X, Bv)
    assert ctx.refcount() == refs
    W = LocalWorld(2)
    try:
        be2 = pa.SequentialBackend(2)
        A2, offs2, _ = pa.generate_problem(be2, "poisson3d", 8)
        H2 = pa.build_hierarchy(be2, A2, offs2, pa.SAParams(max_coarse=40), device=W.ctxs[0])
        S2 = AMGSolver(W.ctxs[0], H2, part=0)
        A0 = S2.A_dev[0]
        X2 = MultiVector(W.ctxs[0], A0.n_own_cols, 2, A0.n_ghost)
        B2, Y2 = MultiVector(W.ctxs[0], A0.nrows, 2), MultiVector(W.ctxs[0], A0.nrows, 2)
        refs2 = W.ctxs[0].refcount()
        # refused before anything is launched: no sibling part is waiting in an exchange
        refused(-6, S2.vcycle_multi, X2, B2)
        refused(-6, S2.pcg_multi, X2, B2)
        refused(-6, spmm, Y2, A0, X2)
        refused(-6, residual_multi, Y2, A0, X2, B2)
        assert W.ctxs[0].refcount() == refs2 and not W.broken
        del S2, X2, B2, Y2, A0
    finally:
        W.close()


@pytest.mark.parametrize("n_own", [1, 81, 4096])
def test_mvec_round_trip(ctx, n_own):
    refs = ctx.refcount()
    rng = np.random.default_rng(n_own)
    for k in (1, 3, 8):
        a = rng.standard_normal((n_own, k))
        X = MultiVector.from_numpy(ctx, a, n_ghost=5)
        assert ctx.refcount() == refs + 1
        assert X.stride % 32 == 0 and n_own + 5 <= X.stride < n_own + 5 + 32
        assert eq(X.to_numpy(), a)
        for c in range(k):
            v = X.column(c)
            assert (v.device_ptr() - X.column(0).device_ptr()) == 8 * c * X.stride and v.device_ptr() % 256 == 0
            assert eq(v.own_values(), a[:, c]) and np.array_equal(v.ghost_values(), np.zeros(5))
            v.set(-a[:, c])
            del v
        assert eq(X.to_numpy(), -a)
        del X
    assert ctx.refcount() == refs
