"""Point-block Jacobi and Chebyshev smoothers and the block estimate (SPEC §S12) on the GPU, bit for bit
against a restatement written here: the oracle's residual and SpMV, and numpy elementwise operations
(numpy fuses nothing) for the block solve w_i = ((0.0 + Dinv_i0 u_0) + Dinv_i1 u_1) + ... and for the
epilogues. The blocks and their inverses come from the host helper, which tests/test_block_diag_host.py
pins against numpy and a pure-Python §S5. The coarsest solve of the cycle restatement is the oracle's
SpMV over the dense inverse, as in tests/test_gpu_chebyshev.py.

Row operations first — the shapes put the block pass at its edges: one block, less than one run of 768
rows, exactly two runs, a partial last run, and the residual pass in the tile, symmetric and ELL layouts —
then cycles, PCG, several parts, the iteration counts the feature is for, and the errors."""
import contextlib
import ctypes

import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd import hcsr as HC
from parallel_amg_amd._lib import PamgError, call, layout_of
from parallel_amg_amd.partitioned import (LocalWorld, PSparseMatrix, PVector, block_chebyshev, block_jacobi,
                                          estimate_lmax_block, mul)
from parallel_amg_amd.solver import AMGSolver
from test_gpu_chebyshev import PAIRS, pcg_bits_ref

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


# ------------------------------------------------------------------------------ the restatement
def coeffs_ref(lmax, ratio, m):
    lmin = lmax / ratio
    theta = (lmax + lmin) / 2.0
    delta = (lmax - lmin) / 2.0
    sigma = theta / delta
    c1, c2, r = [0.0], [1.0 / theta], 1.0 / sigma
    for _ in range(1, m):
        rk = 1.0 / (2.0 * sigma - r)
        c1.append(rk * r)
        c2.append((2.0 * rk) / delta)
        r = rk
    return c1, c2


def diag_of(M):
    rows = np.repeat(np.arange(M.nrows), np.diff(M.rowptr))
    d = np.zeros(M.nrows)
    e = M.col == rows
    d[rows[e]] = M.val[e]
    return d


def to_hcsr(M):
    return HC.HCSR.from_arrays(M.rowptr, M.col.astype(np.int32), M.val, M.ncols)


def block_apply(T, u, bs):
    """w_i = sum_j T_ij u_{bs m + j} over row i's block m, from 0.0 + p_0, j ascending; T is (n, bs)."""
    ub = np.repeat(u.reshape(-1, bs), bs, axis=0)  # row i: the u of its block
    w = np.zeros(len(u))
    for j in range(bs):
        p = T[:, j] * ub[:, j]
        w = w + p
    return w


def block_jacobi_ref(M, inv, bs, x, b, omega):
    """One sweep from x (None: the zero-guess form)."""
    if x is None:
        u = b - 0.0
        v = omega * block_apply(inv, u, bs)
        return 0.0 + v
    u = O.residual(M, x, b)
    v = omega * block_apply(inv, u, bs)
    return x + v


def block_cheb_ref(M, inv, bs, x, b, c1, c2, m):
    xo, x = x, block_jacobi_ref(M, inv, bs, x, b, c2[0])
    for k in range(1, m):
        u = O.residual(M, x, b)
        v = c2[k] * block_apply(inv, u, bs)
        e = x - (xo if xo is not None else 0.0)
        q = c1[k] * e
        t = q + v
        xo, x = x, x + t
    return x


def block_estimate_ref(M, blocks, inv, bs, v, steps):
    lam = []
    for _ in range(steps):
        y = O.spmv(M, v)
        num = float(np.sum(v * y))
        den = float(np.sum(block_apply(blocks, v, bs) * v))
        lam.append(num / den)
        v = block_apply(inv, y, bs)
    return np.array(lam), v, y


def scalar_jacobi_ref(M, d, x, b, omega):
    if x is None:
        return 0.0 + ((omega * (b - 0.0)) / d)
    return O.jacobi(M, x, b, omega)


def scalar_cheb_ref(M, d, x, b, c1, c2, m):
    xo, x = x, scalar_jacobi_ref(M, d, x, b, c2[0])
    for k in range(1, m):
        u = O.residual(M, x, b)
        w = (c2[k] * u) / d
        e = x - (xo if xo is not None else 0.0)
        t = (c1[k] * e) + w
        xo, x = x, x + t
    return x


def dense_csr(a):
    n = a.shape[0]
    return O.CSR(np.arange(0, n * n + 1, n, dtype=np.int64), np.tile(np.arange(n, dtype=np.int64), n),
                 np.ascontiguousarray(a).reshape(-1).copy(), n)


class CycleRef:
    """SPEC §S6 over an oracle hierarchy with the §S12 smoother: ``bsz`` maps a block level to its block
    size, the other levels smooth in the scalar form of the same kind. ``omega`` / ``lmax``: per level."""

    def __init__(self, Ho, kind, bsz, omega, lmax, ratio=4.0):
        self.H, self.kind, self.bsz, self.omega = Ho, kind, dict(bsz), list(omega)
        self.D = [diag_of(M) for M in Ho.A]
        self.inv = {l: HC.block_diag(to_hcsr(Ho.A[l]), 0, bs)[1] for l, bs in self.bsz.items()}
        self.co = [coeffs_ref(lmax[l], ratio, 8) for l in range(Ho.nlevels - 1)]
        self.ainv = dense_csr(Ho.ainv)

    def smooth(self, l, x, b, nu):
        M = self.H.A[l]
        if self.kind == "chebyshev":
            c1, c2 = self.co[l]
            if l in self.bsz:
                return block_cheb_ref(M, self.inv[l], self.bsz[l], x, b, c1, c2, nu)
            return scalar_cheb_ref(M, self.D[l], x, b, c1, c2, nu)
        for _ in range(nu):
            if l in self.bsz:
                x = block_jacobi_ref(M, self.inv[l], self.bsz[l], x, b, self.omega[l])
            else:
                x = scalar_jacobi_ref(M, self.D[l], x, b, self.omega[l])
        return x

    def cycle(self, l, x, b, nu1, nu2):
        H = self.H
        if l == H.nlevels - 1:
            return O.spmv(self.ainv, b)
        x = self.smooth(l, x, b, nu1)
        bc = O.spmv(H.R[l], O.residual(H.A[l], x, b))
        x = x + O.spmv(H.P[l], self.cycle(l + 1, None, bc, nu1, nu2))
        return self.smooth(l, x, b, nu2)

    def solve(self, b, ncycles, nu1, nu2):
        x, hist = np.zeros(len(b)), []
        for _ in range(ncycles):
            x = self.cycle(0, x, b, nu1, nu2)
            hist.append(np.linalg.norm(O.residual(self.H.A[0], x, b)))
        return x, np.array(hist)

    def pcg(self, b, rtol, maxit, nu1, nu2):
        A = self.H.A[0]
        x = np.zeros(len(b))
        r = O.residual(A, x, b)
        nr0 = np.linalg.norm(r)
        z = self.cycle(0, None, r, nu1, nu2)
        p, rz, k = z.copy(), r @ z, 0
        while k < maxit:
            k += 1
            q = O.spmv(A, p)
            alpha = rz / (p @ q)
            x = x + alpha * p
            r = r - alpha * q
            if np.linalg.norm(r) <= rtol * nr0:
                break
            z = self.cycle(0, None, r, nu1, nu2)
            rz, rz_old = r @ z, rz
            p = z + (rz / rz_old) * p
        return x, k


# ------------------------------------------------------------------------------ row operations
LMAX, RATIO, OMEGA, STEPS, SEED = 1.6, 4.0, 0.625, 4, 20240807


def hand_3x3():
    a = np.array([[4.0, -1.0, 0.5], [-1.0, 3.0, -0.25], [0.5, -0.25, 2.0]])
    return dense_csr(a)


# name -> (matrix, block size, upload options, layout flag the residual pass must run in)
TILES = dict(sym_dia=0, ell=0)
ELL = dict(ell_min_rows=0, sym_dia=0)
ROW_CASES = {
    "one_block-3rows-bs3-tiles": (hand_3x3, 3, TILES, "tiles"),
    "elastic3d6-648rows-bs3-tiles": (lambda: O.generate("elastic3d", 6, 6, 6), 3, {}, "tiles"),
    "elastic3d8-1536rows-bs3-tiles": (lambda: O.generate("elastic3d", 8, 8, 8), 3, {}, "tiles"),
    "elastic3d12-5184rows-bs3-tiles": (lambda: O.generate("elastic3d", 12, 12, 12), 3, {}, "tiles"),
    "poisson3d16-bs2-sym": (lambda: O.generate("poisson3d", 16, 16, 16), 2, {}, "sym"),
    "poisson3d16-bs4-ell": (lambda: O.generate("poisson3d", 16, 16, 16), 4, ELL, "ell"),
    "poisson3d32-bs4-sym": (lambda: O.generate("poisson3d", 32, 32, 32), 4, {}, "sym"),
    "poisson3d32-bs2-ell": (lambda: O.generate("poisson3d", 32, 32, 32), 2, ELL, "ell"),
}
_rows = {}


def row_case(ctx, name):
    """The matrix on the host and the device (block data attached), random x and b, and a cache of wanted
    results, built once per case."""
    if name not in _rows:
        gen, bs, opts, flag = ROW_CASES[name]
        M = gen()
        blocks, inv, _rho = HC.block_diag(to_hcsr(M), 0, bs)
        with options(**opts):
            D = PSparseMatrix(ctx, to_hcsr(M))
        lay = layout_of(D)
        if flag == "tiles":
            assert not lay["sym"] and not lay["ell"] and lay["tiles"] > 0, lay
        else:
            assert lay[flag], lay
        D.set_block_diag(bs, blocks, inv)
        assert D.block_size == bs
        rng = np.random.default_rng(7)
        _rows[name] = (M, D, bs, blocks, inv, rng.standard_normal(M.nrows), rng.standard_normal(M.nrows), {})
    return _rows[name]


def differ(got, want):
    return f"{np.count_nonzero(got != want)} of {len(want)} rows differ"


@pytest.mark.parametrize("nsweeps", [1, 3])
@pytest.mark.parametrize("name", list(ROW_CASES))
def test_block_jacobi_bits(ctx, name, nsweeps):
    M, D, bs, _blocks, inv, xh, bh, cache = row_case(ctx, name)
    if "jac" not in cache:
        xs, cache["jac"] = xh, {}
        for k in (1, 2, 3):
            xs = block_jacobi_ref(M, inv, bs, xs, bh, OMEGA)
            cache["jac"][k] = bits(xs)
    x, b, t = D.new_input_vector(), PVector(ctx, M.nrows, 0, bh), D.new_input_vector()
    x.set(xh)
    block_jacobi(x, D, b, t, OMEGA, nsweeps)
    got = bits(x.own_values())
    assert np.array_equal(got, cache["jac"][nsweeps]), differ(got, cache["jac"][nsweeps])
    assert np.array_equal(bits(b.own_values()), bits(bh))


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
@pytest.mark.parametrize("name", list(ROW_CASES))
def test_block_chebyshev_bits(ctx, name, degree):
    M, D, bs, _blocks, inv, xh, bh, cache = row_case(ctx, name)
    key = ("cheb", degree)
    if key not in cache:
        c1, c2 = coeffs_ref(LMAX, RATIO, degree)
        cache[key] = bits(block_cheb_ref(M, inv, bs, xh, bh, c1, c2, degree))
    x, b = D.new_input_vector(), PVector(ctx, M.nrows, 0, bh)
    x.set(xh)
    t1, t2 = D.new_input_vector(), D.new_input_vector()
    block_chebyshev(x, D, b, t1, t2, lmax=LMAX, ratio=RATIO, degree=degree)
    got = bits(x.own_values())
    assert np.array_equal(got, cache[key]), differ(got, cache[key])
    assert np.array_equal(bits(b.own_values()), bits(bh))


@pytest.mark.parametrize("name", list(ROW_CASES))
def test_block_estimate(ctx, name):
    """v and y bit for bit, lambda to 4e-12 (two reductions, SPEC §S10), and every lambda below the bound."""
    M, D, bs, blocks, inv, _xh, _bh, _cache = row_case(ctx, name)
    lam_w, v_w, y_w = block_estimate_ref(M, blocks, inv, bs, O.xstar(M.nrows, 0, SEED), STEPS)
    v, y = D.new_input_vector(), D.new_output_vector()
    v.fill_xstar(0, SEED)
    lam = estimate_lmax_block(D, v, y, STEPS, all_parts=False)
    print(f"\n  {name}: lambda {lam.tolist()}")
    assert np.array_equal(bits(v.own_values()), bits(v_w)), differ(bits(v.own_values()), bits(v_w))
    assert np.array_equal(bits(y.own_values()), bits(y_w))
    np.testing.assert_allclose(lam, lam_w, rtol=4e-12)
    rho_b = HC.block_diag(to_hcsr(M), 0, bs)[2]
    assert np.all(lam <= rho_b * (1 + 1e-12))


def test_scalar_calls_keep_their_bits_with_block_data_attached(ctx):
    """Attaching block data changes nothing for the scalar smoother: the oracle's Jacobi sweep."""
    from parallel_amg_amd.partitioned import jacobi
    M, D, _bs, _blocks, _inv, xh, bh, _cache = row_case(ctx, "elastic3d6-648rows-bs3-tiles")
    x, b, t = D.new_input_vector(), PVector(ctx, M.nrows, 0, bh), D.new_input_vector()
    x.set(xh)
    jacobi(x, D, b, t, OMEGA, 1)
    assert np.array_equal(bits(x.own_values()), bits(O.jacobi(M, xh, bh, OMEGA)))


# ------------------------------------------------------------------------------ cycles
# name -> (grid, max_coarse, {level: block size}); elastic3d 12 coarsens to 5184 / 150 / 8 rows, and with
# blocks of 2 on its level 1 too the zero-guess block form runs inside every cycle
PROBLEMS = {"elastic3d8": (8, 100, {0: 3}), "elastic3d12": (12, 100, {0: 3}),
            "elastic3d12_two_block_levels": (12, 100, {0: 3, 1: 2})}
_problems = {}


def problem(ctx, name):
    if name not in _problems:
        n, mc, bsz = PROBLEMS[name]
        be = pa.SequentialBackend(1)
        Ah, offs, xs = pa.generate_problem(be, "elastic3d", n)
        H = pa.build_hierarchy(be, Ah, offs, pa.SAParams(max_coarse=mc), device=ctx)
        S = AMGSolver(ctx, H)
        for l, bs in bsz.items():
            S.set_block_size(bs, levels=(l,))
        assert S.block_size == bsz
        b = PVector(ctx, S.A[0].nrows)
        mul(b, S.A[0], PVector(ctx, S.A[0].nrows, 0, xs[0]))
        Ao = O.generate("elastic3d", n, n, n)
        bo = O.spmv(Ao, O.xstar(Ao.nrows))
        assert np.array_equal(bits(b.own_values()), bits(bo))
        Ho = O.setup(Ao, max_coarse=mc)
        assert Ho.nlevels == H.nlevels
        rho_b = {l: HC.block_diag(to_hcsr(Ho.A[l]), 0, bs)[2] for l, bs in bsz.items()}
        assert S.rho_b == rho_b
        nl = Ho.nlevels - 1
        lmax = [rho_b.get(l, Ho.rho[l]) for l in range(nl)]
        omega = [4.0 / (3.0 * rho_b[l]) if l in rho_b else Ho.omega[l] for l in range(nl)]
        refs = {k: CycleRef(Ho, k, bsz, omega, lmax) for k in ("jacobi", "chebyshev")}
        _problems[name] = (S, b, bo, refs, {})
    return _problems[name]


@contextlib.contextmanager
def smoother(S, kind, nu, **kw):
    S.set_smoother(kind, **kw)
    S.set_sweeps(*nu)
    try:
        yield
    finally:
        S.set_graph(True)
        S.set_smoother("jacobi")
        S.set_sweeps(1, 1)


@pytest.mark.parametrize("kind,nu", [("jacobi", (1, 1)), ("jacobi", (2, 1)), ("chebyshev", (2, 2)),
                                     ("chebyshev", (3, 3))])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_cycle_bits(ctx, name, kind, nu):
    """3 stationary cycles from x = 0 with the default bounds (rho_b on block levels): the restatement's x
    bits and residual history, from the captured graph and from eager launches."""
    S, b, bo, refs, cache = problem(ctx, name)
    if (kind, nu) not in cache:
        cache[(kind, nu)] = refs[kind].solve(bo, 3, *nu)
    xo, ho = cache[(kind, nu)]
    with smoother(S, "block_" + kind, nu, ratio=4.0):
        for graph in (True, False):
            S.set_graph(graph)
            x = S.new_vector()
            hist = S.vcycle(x, b, 3, res_hist=True)
            got = bits(x.own_values())
            assert np.array_equal(got, bits(xo)), (name, kind, nu, graph, differ(got, bits(xo)))
            np.testing.assert_allclose(hist, ho, rtol=1e-12)
            assert S.graph_state()["captured"] == graph
            assert not S.graph_state()["failed"]


@pytest.mark.parametrize("kind,nu", [("jacobi", (1, 1)), ("chebyshev", (2, 2))])
@pytest.mark.parametrize("name", ["elastic3d8", "elastic3d12"])
def test_pcg(ctx, name, kind, nu):
    """PCG to 1e-8: the restated PCG's iteration count and its x to 1e-8; the device-resident PCG
    (lookahead 0) gives pamg_pcg's bits."""
    S, b, bo, refs, _cache = problem(ctx, name)
    xr, kr = refs[kind].pcg(bo, 1e-8, 60, *nu)
    with smoother(S, "block_" + kind, nu, ratio=4.0):
        x = S.new_vector()
        k, hist = S.pcg(x, b, 1e-8, 60)
        x0 = S.new_vector()
        k0, hist0 = S.pcg(x0, b, 1e-8, 60, lookahead=0)
    print(f"\n  {name} block {kind} V{nu}: pcg iterations device {k}, restatement {kr}")
    assert k == kr
    assert np.linalg.norm(x.own_values() - xr) <= 1e-8 * np.linalg.norm(xr)
    assert hist[-1] <= 1e-8 * hist[0]
    assert k0 == k
    assert np.array_equal(bits(x0.own_values()), bits(x.own_values()))
    assert np.array_equal(bits(hist0), bits(hist))


@pytest.mark.parametrize("nu", PAIRS)
@pytest.mark.parametrize("kind", ["jacobi", "chebyshev"])
def test_cycle_and_pcg_bits_every_pair(ctx, kind, nu):
    """elastic3d 8, every (nu1, nu2) in {1..4}^2 (the sweeps' ping-pong parities, the degrees' remainders
    mod 3): 2 stationary cycles from a given guess, graph and eager, give the restatement's x bits; 2
    PCG iterations (every cycle from a zero guess) the restated iteration's x and history bits."""
    S, b, bo, refs, cache = problem(ctx, "elastic3d8")
    ref = refs[kind]
    if ("two", kind, nu) not in cache:
        cache[("two", kind, nu)] = (ref.solve(bo, 2, *nu),
                                    pcg_bits_ref(lambda r: ref.cycle(0, None, r, *nu), ref.H.A[0], bo, 2))
    (xo, ho), (xp, hp) = cache[("two", kind, nu)]
    with smoother(S, "block_" + kind, nu, ratio=4.0):
        for graph in (True, False):
            S.set_graph(graph)
            x = S.new_vector()
            hist = S.vcycle(x, b, 2, res_hist=True)
            got = bits(x.own_values())
            assert np.array_equal(got, bits(xo)), (kind, nu, graph, differ(got, bits(xo)))
            np.testing.assert_allclose(hist, ho, rtol=1e-12)
            assert S.graph_state()["captured"] == graph
            assert not S.graph_state()["failed"]
        S.set_graph(True)
        for lookahead in (None, 0):
            x = S.new_vector()
            k, hist = S.pcg(x, b, 0.0, 2, lookahead=lookahead)
            got = bits(x.own_values())
            assert k == 2
            assert np.array_equal(got, bits(xp)), (kind, nu, lookahead, differ(got, bits(xp)))
            assert np.array_equal(bits(hist), bits(hp)), (kind, nu, lookahead)


def test_switching_back_leaves_no_state(ctx):
    """Block cycles, then "jacobi" V(1,1): the oracle's own cycles again, bit for bit — the block data
    still attached."""
    S, b, bo, _refs, _cache = problem(ctx, "elastic3d8")
    with smoother(S, "block_chebyshev", (2, 2)):
        S.vcycle(S.new_vector(), b, 2)
    Ao = O.generate("elastic3d", 8, 8, 8)
    xo, ho = O.setup(Ao, max_coarse=100).solve(bo, 3, res_hist=True)
    x = S.new_vector()
    hist = S.vcycle(x, b, 3, res_hist=True)
    assert np.array_equal(bits(x.own_values()), bits(xo))
    np.testing.assert_allclose(hist, ho, rtol=1e-12)


def test_profile_slots_and_bench_chain(ctx):
    """The profiling slots hold the block sweeps, and the pipeline's chain benchmark refuses a block
    hierarchy."""
    S, b, _bo, _refs, _cache = problem(ctx, "elastic3d8")
    with smoother(S, "block_jacobi", (1, 1)):
        assert S.bench_chain(S.new_vector(), b, 1) is None
        ms = S.profile(S.new_vector(), b, 1)
        assert ms[0, 0] > 0 and ms[0, 4] > 0 and ms[0, 1] > 0, ms


# ------------------------------------------------------------------------------ several parts
@pytest.mark.parametrize("nparts", [2, 4])
def test_parts(built, nparts):
    """elastic3d 6 on 2 and 4 parts (offsets multiples of 324 and 162, whole nodes; in-process transport,
    ghost slots poisoned before each exchange). The row operations give the one-part restatement's bits
    on every part; block Jacobi V(1,1) and block Chebyshev V(2,2) cycles give the restatement's on the
    oracle's decoupled hierarchy."""
    n, bs, ncycles = 6, 3, 3
    Ao = O.generate("elastic3d", n, n, n)
    blocks, inv, rho_b = HC.block_diag(to_hcsr(Ao), 0, bs)
    rng = np.random.default_rng(11)
    xh, bh = rng.standard_normal(Ao.nrows), rng.standard_normal(Ao.nrows)
    c1, c2 = coeffs_ref(LMAX, RATIO, 3)
    want_j = block_jacobi_ref(Ao, inv, bs, block_jacobi_ref(Ao, inv, bs, xh, bh, OMEGA), bh, OMEGA)
    want_c = block_cheb_ref(Ao, inv, bs, xh, bh, c1, c2, 3)
    lam_w, v_w, y_w = block_estimate_ref(Ao, blocks, inv, bs, O.xstar(Ao.nrows, 0, SEED), STEPS)
    got = {}
    with options(poison_ghosts=1):
        W = LocalWorld(nparts)
        try:
            be = pa.SequentialBackend(nparts)
            A, offs, xs = pa.generate_problem(be, "elastic3d", n)
            assert all(int(o) % (Ao.nrows // nparts) == 0 for o in offs)
            H = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=100), device=W.ctxs[0])
            S = [AMGSolver(W.ctxs[p], H, part=p) for p in range(nparts)]
            for s in S:
                s.set_block_size(bs)
                assert s.rho_b == {0: rho_b}
            A0 = [s.A[0] for s in S]
            own = [slice(int(offs[p]), int(offs[p + 1])) for p in range(nparts)]

            def vec(p, vals=None):
                v = A0[p].new_input_vector()
                if vals is not None:
                    v.set(vals[own[p]])
                return v

            b = [PVector(W.ctxs[p], A0[p].nrows, 0, bh[own[p]]) for p in range(nparts)]
            x, t1, t2 = ([vec(p, xh) for p in range(nparts)], [vec(p) for p in range(nparts)],
                         [vec(p) for p in range(nparts)])
            W.run(lambda p: block_jacobi(x[p], A0[p], b[p], t1[p], OMEGA, 2))
            got["jac"] = np.concatenate([v.own_values() for v in x])
            x = [vec(p, xh) for p in range(nparts)]
            W.run(lambda p: block_chebyshev(x[p], A0[p], b[p], t1[p], t2[p], LMAX, RATIO, 3))
            got["cheb"] = np.concatenate([v.own_values() for v in x])
            v = [vec(p) for p in range(nparts)]
            for p in range(nparts):
                v[p].fill_xstar(int(offs[p]), SEED)
            y = [PVector(W.ctxs[p], A0[p].nrows) for p in range(nparts)]
            lam = W.run(lambda p: estimate_lmax_block(A0[p], v[p], y[p], STEPS, all_parts=True))
            got["v"] = np.concatenate([q.own_values() for q in v])
            got["y"] = np.concatenate([q.own_values() for q in y])
            # cycles
            xst = [PVector(W.ctxs[p], A0[p].n_own_cols, A0[p].n_ghost, xs[p]) for p in range(nparts)]
            rhs = [PVector(W.ctxs[p], A0[p].nrows) for p in range(nparts)]
            W.run(lambda p: mul(rhs[p], A0[p], xst[p]))
            for kind, nu in (("jacobi", (1, 1)), ("chebyshev", (2, 2))):
                for s in S:
                    s.set_smoother("block_" + kind, ratio=4.0)
                    s.set_sweeps(*nu)
                xc = [s.new_vector() for s in S]
                hist = W.run(lambda p: S[p].vcycle(xc[p], rhs[p], ncycles, res_hist=True))
                got[kind] = (np.concatenate([q.own_values() for q in xc]), hist[0])
        finally:
            del S
            W.close()
    assert np.array_equal(bits(got["jac"]), bits(want_j)), differ(bits(got["jac"]), bits(want_j))
    assert np.array_equal(bits(got["cheb"]), bits(want_c)), differ(bits(got["cheb"]), bits(want_c))
    assert np.array_equal(bits(got["v"]), bits(v_w))
    assert np.array_equal(bits(got["y"]), bits(y_w))
    for p in range(nparts):
        np.testing.assert_allclose(lam[p], lam_w, rtol=4e-12)
        assert np.array_equal(lam[p], lam[0])
    bo = O.spmv(Ao, O.xstar(Ao.nrows))
    Ho = O.setup(Ao, nparts=nparts, max_coarse=100)
    nl = Ho.nlevels - 1
    lmax = [rho_b] + list(Ho.rho[1:nl])
    omega = [4.0 / (3.0 * rho_b)] + list(Ho.omega[1:nl])
    for kind, nu in (("jacobi", (1, 1)), ("chebyshev", (2, 2))):
        xo, ho = CycleRef(Ho, kind, {0: bs}, omega, lmax).solve(bo, ncycles, *nu)
        assert np.array_equal(bits(got[kind][0]), bits(xo)), (kind, differ(bits(got[kind][0]), bits(xo)))
        np.testing.assert_allclose(got[kind][1], ho, rtol=1e-12)


# ------------------------------------------------------------------------------ what the feature is for
def test_block_smoothers_need_fewer_pcg_iterations(ctx):
    """elastic3d 12 (max_coarse 100), PCG to 1e-8, every bound estimated: block Jacobi V(1,1) needs
    strictly fewer iterations than Jacobi V(1,1), and block Chebyshev V(2,2) than Chebyshev V(2,2)."""
    S, b, _bo, _refs, _cache = problem(ctx, "elastic3d12")
    its = {}
    for kind, nu in (("jacobi", (1, 1)), ("block_jacobi", (1, 1)), ("chebyshev", (2, 2)),
                     ("block_chebyshev", (2, 2))):
        with smoother(S, kind, nu, ratio=4.0, lmax="estimate"):
            x = S.new_vector()
            its[kind], hist = S.pcg(x, b, 1e-8, 100)
            assert hist[-1] <= 1e-8 * hist[0]
    print(f"\n  elastic3d 12 pcg iterations: {its}")
    assert its["block_jacobi"] < its["jacobi"], its
    assert its["block_chebyshev"] < its["chebyshev"], its


# ------------------------------------------------------------------------------ errors
@pytest.fixture(scope="module")
def small_hierarchy(ctx):
    be = pa.SequentialBackend(1)
    A, offs, _xs = pa.generate_problem(be, "elastic3d", 6)
    return pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=100), device=ctx)


def raises(code, text, fn, *args, **kw):
    with pytest.raises(PamgError) as e:
        fn(*args, **kw)
    assert e.value.code == code and text in str(e.value), e.value


def test_no_block_data_is_a_state_error(ctx, small_hierarchy):
    M = O.generate("elastic3d", 4, 4, 4)
    D = PSparseMatrix(ctx, to_hcsr(M))
    x, t1, t2, b = (D.new_input_vector() for _ in range(4))
    y = D.new_output_vector()
    raises(-6, "no block data", block_jacobi, x, D, b, t1, OMEGA, 1)
    raises(-6, "no block data", block_chebyshev, x, D, b, t1, t2, LMAX, RATIO, 2)
    raises(-6, "no block data", estimate_lmax_block, D, x, y, 2)
    S = AMGSolver(ctx, small_hierarchy)
    for kind in (2, 3):
        lm = np.full(S.L - 1, 2.0)
        raises(-6, "needs block data", call, "pamg_hier_set_smoother", S.handle, kind,
               lm.ctypes.data_as(ctypes.c_void_p), 4.0)
    raises(-6, "set_block_size", S.set_smoother, "block_jacobi")
    # attached and removed again: the same error
    blocks, inv, _ = HC.block_diag(to_hcsr(M), 0, 3)
    D.set_block_diag(3, blocks, inv)
    block_jacobi(x, D, b, t1, OMEGA, 1)
    D.set_block_diag(1)
    assert D.block_size == 1
    raises(-6, "no block data", block_jacobi, x, D, b, t1, OMEGA, 1)


def test_prolongation_and_restriction_are_refused(ctx, small_hierarchy):
    lp = small_hierarchy.levels[0][0]
    for M in (lp.R, lp.P):
        D = PSparseMatrix(ctx, M)
        raises(-1, "must be square", D.set_block_diag, 3, np.zeros((M.nrows, 3)), np.zeros((M.nrows, 3)))
        x, t1, t2 = (D.new_input_vector() for _ in range(3))
        b = D.new_output_vector()
        raises(-1, "must be square", block_jacobi, x, D, b, t1, OMEGA, 1)
        raises(-1, "must be square", block_chebyshev, x, D, b, t1, t2, LMAX, RATIO, 2)
        raises(-1, "must be square", estimate_lmax_block, D, x, b, 2)


def test_permuted_uploads_are_refused(ctx, small_hierarchy):
    M = O.generate("elastic3d", 4, 4, 4)
    perm = np.random.default_rng(5).permutation(M.nrows)
    D = PSparseMatrix(ctx, to_hcsr(M), row_perm=perm, col_perm=perm)
    blocks, inv, _ = HC.block_diag(to_hcsr(M), 0, 3)
    raises(-6, "permutation", D.set_block_diag, 3, blocks, inv)
    S = AMGSolver(ctx, small_hierarchy, reorder="on")
    with pytest.raises(ValueError, match="permutation"):
        S.set_block_size(3)


def test_rows_not_whole_blocks(ctx):
    M = O.generate("poisson3d", 3, 3, 3)  # 27 rows
    D = PSparseMatrix(ctx, to_hcsr(M))
    for bs in (2, 4):
        raises(-1, "not whole blocks", D.set_block_diag, bs, np.ones((27, bs)), np.ones((27, bs)))
    raises(-1, "outside 1..4", D.set_block_diag, 5, np.ones((27, 5)), np.ones((27, 5)))
    # four parts of elastic3d 6: offsets 0 / 162 / 324 / 486 / 648, whole nodes but no multiples of 4
    W = LocalWorld(4)
    try:
        be = pa.SequentialBackend(4)
        A, offs, _xs = pa.generate_problem(be, "elastic3d", 6)
        H = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=100), device=W.ctxs[0])
        S = AMGSolver(W.ctxs[0], H, part=0)
        with pytest.raises(ValueError, match="not multiples of 4"):
            S.set_block_size(4)
        with pytest.raises(ValueError, match="outside 1..4"):
            S.set_block_size(5)
        S.set_block_size(3)
        assert S.block_size == {0: 3}
    finally:
        del S
        W.close()


def test_aliasing_vectors(ctx):
    M, D, _bs, _blocks, _inv, _xh, _bh, _cache = row_case(ctx, "elastic3d6-648rows-bs3-tiles")
    x, t1, t2, b = (D.new_input_vector() for _ in range(4))
    for args in ((x, D, b, x), (x, D, x, t1), (x, D, t1, t1)):
        raises(-1, "aliasing", block_jacobi, *args, OMEGA, 1)
    for args in ((x, D, b, x, t2), (x, D, b, t1, t1), (x, D, x, t1, t2), (x, D, b, t1, b)):
        raises(-1, "aliasing", block_chebyshev, *args, LMAX, RATIO, 2)
    raises(-1, "must differ", estimate_lmax_block, D, x, x, 2)
    for kw in (dict(lmax=2.0, ratio=1.0, degree=2), dict(lmax=0.0, ratio=4.0, degree=2),
               dict(lmax=2.0, ratio=4.0, degree=0), dict(lmax=2.0, ratio=4.0, degree=65)):
        with pytest.raises(PamgError) as e:
            block_chebyshev(x, D, b, t1, t2, **kw)
        assert e.value.code == -1
    for steps in (0, 65):
        raises(-1, "steps", estimate_lmax_block, D, x, D.new_output_vector(), steps)
