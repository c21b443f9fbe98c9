"""A nodal hierarchy (SPEC §S14) on the GPU with every level in the block-row layout (``block_layout="all"``):
V-cycles and PCG against the oracle's cycle over the same level operators (``oracle.hierarchy_from_levels``),
bit for bit; Chebyshev and the point-block smoothers on every level (``set_block_size(bs, levels="all")``)
against a solver without ``block_layout`` and against the cycle restatement of tests/test_gpu_block_smoother.py;
the multi-column cycle and PCG against their single-column calls. Problems: elastic3d at 5^3 and 7^3 nodes and the
variable-coefficient L_w (x) B of tests/test_gpu_bsr.py at 6^3, MAX_COARSE = 40.

The last test runs no GPU: PCG iteration counts of the nodal and the scalar hierarchy on elastic3d 7^3."""
import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd import hcsr as HC
from parallel_amg_amd.partitioned import MultiVector, PVector, mul
from parallel_amg_amd.solver import AMGSolver
import test_gpu_block_smoother as T
from test_gpu_block_smoother import bits, differ, to_hcsr
from test_gpu_bsr import raw_layout, var_matrix
from test_nodal_setup import node_blocked

gpu = pytest.mark.gpu
MAX_COARSE = 40
BS = 3
PROBLEMS = {"elastic3d5": lambda: O.generate("elastic3d", 5, 5, 5), "elastic3d7": lambda: O.generate("elastic3d", 7, 7, 7),
            "var6": lambda: var_matrix(6)}


def to_ocsr(M):
    return O.CSR(M.rowptr.copy(), M.col.astype(np.int64), M.val.copy(), M.ncols)


class LevelRef:
    """The host hierarchy's operators as oracle CSRs, in the shape CycleRef reads (A, P, R, ainv, nlevels)."""

    def __init__(self, H):
        lps = [H.levels[l][0] for l in range(H.nlevels)]
        self.A = [to_ocsr(lp.A) for lp in lps]
        self.P = [to_ocsr(lp.P) for lp in lps[:-1]]
        self.R = [to_ocsr(lp.R) for lp in lps[:-1]]
        self.omega = [lp.omega for lp in lps]
        self.rho = [lp.rho for lp in lps]
        self.nlevels = H.nlevels
        n = H.n_coarse
        self.ainv = np.asarray(H.ainv).reshape(n, n).T.copy()


def host(name, block_size=BS):
    Ao = PROBLEMS[name]()
    be = pa.SequentialBackend(1)
    H = pa.build_hierarchy(be, {0: to_hcsr(Ao)}, np.array([0, Ao.nrows], np.int64),
                           pa.SAParams(max_coarse=MAX_COARSE, block_size=block_size))
    lps = [H.levels[l][0] for l in range(H.nlevels)]
    Ho = O.hierarchy_from_levels([lp.A for lp in lps], [lp.P for lp in lps[:-1]], [lp.R for lp in lps[:-1]],
                                 [lp.omega for lp in lps], H.ainv)
    return Ao, H, Ho


_problems = {}


def problem(ctx, name):
    if name not in _problems:
        Ao, H, Ho = host(name)
        assert H.nlevels >= 2 and H.block_size == BS
        # the invariant on the CPU first: every operator qualifies for the block-row layout
        for l in range(H.nlevels):
            lp = H.levels[l][0]
            assert node_blocked(lp.A, BS, True), l
            if l < H.nlevels - 1:
                assert node_blocked(lp.P, BS, False) and node_blocked(lp.R, BS, False), l
        S = AMGSolver(ctx, H, reorder="off", block_layout="all")
        Pl = AMGSolver(ctx, H, reorder="off")
        assert S.block_layout == {l: BS for l in range(H.nlevels)}
        for l in range(H.nlevels - 1):
            for Q in (S.A_dev[l], S.P[l], S.R[l]):
                assert Q.blocked and raw_layout(Q)[9] & 32768 and raw_layout(Q)[3] == BS, l
            assert not S.P[l].row_lanes and not S.A_dev[l].row_lanes
            for Q in (Pl.A_dev[l], Pl.P[l], Pl.R[l]):
                assert not Q.blocked
        for Q in (S, Pl):
            Q.set_block_size(BS, levels="all")
            assert sorted(Q.block_size) == list(range(H.nlevels - 1))
        bo = O.spmv(Ao, O.xstar(Ao.nrows))
        b = PVector(ctx, Ao.nrows)
        mul(b, S.A[0], PVector(ctx, Ao.nrows, 0, O.xstar(Ao.nrows)))
        assert np.array_equal(bits(b.own_values()), bits(bo))
        ref = LevelRef(H)
        nl = H.nlevels - 1
        rho_b = [HC.block_diag(H.levels[l][0].A, 0, BS)[2] for l in range(nl)]
        assert [S.rho_b[l] for l in range(nl)] == rho_b
        every = {l: BS for l in range(nl)}
        block = {k: T.CycleRef(ref, k, every, [4.0 / (3.0 * r) for r in rho_b], rho_b) for k in ("jacobi", "chebyshev")}
        scalar = T.CycleRef(ref, "chebyshev", {}, ref.omega[:nl], ref.rho[:nl])
        _problems[name] = (S, Pl, b, bo, Ho, block, scalar, {})
    return _problems[name]


def wanted(kind, nu, bo, Ho, block, scalar, cache):
    if (kind, nu) not in cache:
        if kind == "jacobi":
            Ho.set_sweeps(*nu)
            xc, hc = Ho.solve(bo, 3, res_hist=True)
            xp, kp, _hp = Ho.pcg(bo, 1e-8, 60)
            Ho.set_sweeps(1, 1)
        else:
            ref = scalar if kind == "chebyshev" else block[kind[len("block_"):]]
            xc, hc = ref.solve(bo, 3, *nu)
            xp, kp = ref.pcg(bo, 1e-8, 60, *nu)
        cache[(kind, nu)] = (xc, hc, xp, kp)
    return cache[(kind, nu)]


SMOOTHERS = [("jacobi", (1, 1)), ("jacobi", (2, 3)), ("chebyshev", (2, 2)), ("block_jacobi", (1, 1)),
             ("block_chebyshev", (2, 2))]


@gpu
@pytest.mark.parametrize("kind,nu", SMOOTHERS)
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_cycle_and_pcg_bits(ctx, name, kind, nu):
    """Three V-cycles (graph and eager) and PCG: the bits of the oracle's cycle over these levels (Jacobi) or of
    the restatement (the others), and of a solver with every operator in the row-wise layouts."""
    S, Pl, b, bo, Ho, block, scalar, cache = problem(ctx, name)
    xc, hc, xp, kp = wanted(kind, nu, bo, Ho, block, scalar, cache)
    got = {}
    for tag, Q in (("bsr", S), ("plain", Pl)):
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
    for graph in (True, False):
        xb, hb = got["bsr", "cycle", graph]
        assert np.array_equal(xb, bits(xc)), (name, kind, graph, differ(xb, bits(xc)))
        np.testing.assert_allclose(hb.view(np.float64), hc, rtol=1e-12)
        assert np.array_equal(xb, got["plain", "cycle", graph][0])
        assert np.array_equal(hb, got["plain", "cycle", graph][1])
    xb, k, hb = got["bsr", "pcg"]
    h = hb.view(np.float64)
    assert k == kp and h[-1] <= 1e-8 * h[0], (name, kind, k, kp)
    assert np.linalg.norm(xb.view(np.float64) - xp) <= 1e-8 * np.linalg.norm(xp)
    assert np.array_equal(xb, got["plain", "pcg"][0]) and k == got["plain", "pcg"][1]
    assert np.array_equal(hb, got["plain", "pcg"][2])


@gpu
@pytest.mark.parametrize("kind,nu", [("jacobi", (1, 1)), ("block_jacobi", (1, 1)), ("block_chebyshev", (2, 3))])
@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("name", ["elastic3d5", "var6"])
def test_multi_column_cycle_and_pcg(ctx, name, k, kind, nu):
    """vcycle_multi and pcg_multi on k columns: every column has the bits of its single-column solve."""
    S, _Pl, _b, _bo, _Ho, _block, _scalar, _cache = problem(ctx, name)
    n = S.A_dev[0].nrows
    rng = np.random.default_rng(17 + k)
    bh = rng.standard_normal((n, k))
    bh[:, 1] *= 1e-3
    with T.smoother(S, kind, nu, ratio=4.0):
        X, Bv = S.new_multivector(k), MultiVector.from_numpy(ctx, bh)
        hist = S.vcycle_multi(X, Bv, 2, res_hist=True)
        got = X.to_numpy()
        Xp = S.new_multivector(k)
        its, hists = S.pcg_multi(Xp, Bv, 1e-8, 60)
        gp = Xp.to_numpy()
        for c in range(k):
            x, b = S.new_vector(), PVector(ctx, n, 0, bh[:, c])
            h1 = S.vcycle(x, b, 2, res_hist=True)
            assert np.array_equal(bits(got[:, c]), bits(x.own_values())), (name, k, kind, c)
            assert np.array_equal(bits(hist[:, c]), bits(h1)), (name, k, kind, c)
            x = S.new_vector()
            kc, hc = S.pcg(x, b, 1e-8, 60)
            assert its[c] == kc and np.array_equal(bits(gp[:, c]), bits(x.own_values())), (name, k, kind, c)
            assert np.array_equal(bits(np.asarray(hists[c])[:kc + 1]), bits(hc)), (name, k, kind, c)


@gpu
def test_block_layout_forms_and_refusals(ctx):
    _Ao, H, _Ho = host("elastic3d5")
    S = AMGSolver(ctx, H, reorder="off", block_layout={"A": {0: BS}, "R": {0: BS}})
    assert S.block_layout == {0: BS} and S.block_layout_P == {} and S.block_layout_R == {0: BS}
    assert S.A_dev[0].blocked and S.R[0].blocked and not S.P[0].blocked
    S3 = AMGSolver(ctx, H, reorder="off", block_layout=BS)          # today's forms keep their meaning
    assert S3.block_layout == {0: BS} and not S3.P[0].blocked and not S3.R[0].blocked
    with pytest.raises(ValueError, match="levels, or 'A', 'P' and 'R'"):
        AMGSolver(ctx, H, reorder="off", block_layout={"A": {0: BS}, "Q": {}})
    with pytest.raises(ValueError, match="a block size, a dict or 'all'"):
        AMGSolver(ctx, H, reorder="off", block_layout="every")
    _Ao, H1, _Ho1 = host("elastic3d5", block_size=1)
    with pytest.raises(ValueError, match="built with block_size=1"):
        AMGSolver(ctx, H1, reorder="off", block_layout="all")
    with pytest.raises(ValueError, match="levels 'some'"):
        S.set_block_size(BS, levels="some")


def test_pcg_iterations_of_the_nodal_and_the_scalar_hierarchy(built, capsys):
    """No GPU: PCG to 1e-8 with the oracle's V(1,1) Jacobi cycle on elastic3d at 7^3 nodes over the nodal and the
    scalar hierarchy (both MAX_COARSE = 40). Both must converge within maxit; the counts are printed (DESIGN.md,
    "Nodal hierarchy": 22 nodal against 24 scalar), no ratio is asserted."""
    maxit = 100
    counts = {}
    for tag, bs in (("nodal", BS), ("scalar", 1)):
        Ao, H, Ho = host("elastic3d7", block_size=bs)
        bo = O.spmv(Ao, O.xstar(Ao.nrows))
        _x, k, hist = Ho.pcg(bo, 1e-8, maxit)
        assert k < maxit and hist[-1] <= 1e-8 * hist[0], (tag, k)
        counts[tag] = (k, [H.levels[l][0].A.nrows for l in range(H.nlevels)])
    with capsys.disabled():
        print(f"\nelastic3d 7^3, PCG to 1e-8, V(1,1) Jacobi: nodal {counts['nodal']}, scalar {counts['scalar']}")
