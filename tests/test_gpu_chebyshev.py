"""The Chebyshev polynomial smoother (SPEC §S9) on the GPU, bit for bit against a restatement written
here: the coefficients in Python floats, step 0 as the oracle's Jacobi sweep (or its zero-guess form),
step k >= 1 as numpy elementwise operations on the oracle's residual (numpy fuses nothing), and the
cycle as a recursion over the oracle hierarchy's A / P / R with the oracle's SpMV and residual.

The coarsest solve of the restatement is the oracle's SpMV over the dense inverse (products summed
left to right from +0.0, SPEC §S5): ``H.ainv @ b`` goes through BLAS, whose summation order differs
and costs an ulp (measured: 6.7e-16 on the Jacobi V(1,1) restatement against ``Ho.solve``, which the
SpMV form reproduces bit for bit), and the comparisons below are on bits.

One layout at a time first (``layout_of`` says which kernel ran), then whole cycles, PCG and several
parts."""
import contextlib
import ctypes

import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd._lib import PamgError, call, layout_of
from parallel_amg_amd.hcsr import HCSR
from parallel_amg_amd.partitioned import LocalWorld, PSparseMatrix, PVector, chebyshev, mul
from parallel_amg_amd.solver import AMGSolver

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


def cheb_ref(M, d, x, b, c1, c2, m):
    """One polynomial of degree m from x (None: the zero guess)."""
    if x is None:
        xo, x = None, 0.0 + ((c2[0] * (b - 0.0)) / d)
    else:
        xo, x = x, O.jacobi(M, x, b, c2[0])
    for k in range(1, m):
        u = O.residual(M, x, b)
        v = c2[k] * u
        w = v / d
        e = x - (xo if xo is not None else 0.0)
        q = c1[k] * e
        t = q + w
        xo, x = x, x + t
    return x


def dense_csr(a):
    n = a.shape[0]
    return O.CSR(np.arange(0, n * n + 1, n, dtype=np.int64), np.tile(np.arange(n, dtype=np.int64), n),
                 np.ascontiguousarray(a).reshape(-1).copy(), n)


class CycleRef:
    """The V-cycle of SPEC §S6 with the §S9 smoother over an oracle hierarchy."""

    def __init__(self, Ho, ratio=4.0):
        self.H = Ho
        self.D = [diag_of(M) for M in Ho.A]
        self.co = [coeffs_ref(Ho.rho[l], ratio, 8) for l in range(Ho.nlevels)]
        self.ainv = dense_csr(Ho.ainv)

    def cycle(self, l, x, b, nu1, nu2):
        H = self.H
        if l == H.nlevels - 1:
            return O.spmv(self.ainv, b)
        M, (c1, c2) = H.A[l], self.co[l]
        x = cheb_ref(M, self.D[l], x, b, c1, c2, nu1)
        bc = O.spmv(H.R[l], O.residual(M, x, b))
        x = x + O.spmv(H.P[l], self.cycle(l + 1, None, bc, nu1, nu2))
        return cheb_ref(M, self.D[l], x, b, c1, c2, nu2)

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


# ------------------------------------------------------------------------------ one layout at a time
LMAX, RATIO, DEG = 2.3, 4.0, 3
_want = {}


def smoother_want(name, M):
    """Random x and b and the restated degree-3 smoother on them, once per matrix."""
    if name not in _want:
        rng = np.random.default_rng(3)
        xh, bh = rng.standard_normal(M.nrows), rng.standard_normal(M.nrows)
        c1, c2 = coeffs_ref(LMAX, RATIO, DEG)
        _want[name] = (xh, bh, bits(cheb_ref(M, diag_of(M), xh, bh, c1, c2, DEG)))
    return _want[name]


def run_smoother(ctx, name, M, D):
    xh, bh, want = smoother_want(name, M)
    x, b = D.new_input_vector(), PVector(ctx, M.nrows, 0, bh)
    x.set(xh)
    t1, t2 = D.new_input_vector(), D.new_input_vector()
    chebyshev(x, D, b, t1, t2, lmax=LMAX, ratio=RATIO, degree=DEG)
    got = bits(x.own_values())
    assert np.array_equal(got, want), f"{name}: {np.count_nonzero(got != want)} of {len(want)} rows differ"
    assert np.array_equal(bits(b.own_values()), bits(bh))


def upload(ctx, M):
    return PSparseMatrix(ctx, HCSR.from_arrays(M.rowptr, M.col.astype(np.int32), M.val, M.ncols))


@pytest.mark.parametrize("zm_chunks", [0, 3])
@pytest.mark.parametrize("kind,shape", [("poisson3d", (64, 32, 40)), ("aniso3d", (192, 48, 7))])
def test_layout_sym_zm(ctx, kind, shape, zm_chunks):
    """k_sym_zm: the z-marching sweep; zm_chunks 3 puts chunk boundaries inside the grid (40 planes:
    14 + 14 + 12; 7 planes: 3 + 3 + 1)."""
    M = O.generate(kind, *shape)
    D = upload(ctx, M)
    lay = layout_of(D)
    assert lay["sym"] and lay["sym_vd"] and lay["jr_fused"], lay
    with options(sym_zm=1, zm_chunks=zm_chunks):
        run_smoother(ctx, f"{kind}{shape}", M, D)


@pytest.mark.parametrize("vd,rows", [(1, 2), (0, 1), (0, 2)])
def test_layout_sym_older_kernels(ctx, vd, rows):
    """k_rows_symd (row-class dictionary), k_rows_sym and k_rows_sym2: the residual into the output,
    then k_cheb_update over it."""
    M = O.generate("poisson3d", 24, 24, 24)
    with options(sym_zm=0, sym_vd=vd, sym_rows=rows):
        D = upload(ctx, M)
        lay = layout_of(D)
        assert lay["sym"] and lay["sym_vd"] == bool(vd) and lay["sym_rows"] == rows, lay
        run_smoother(ctx, "poisson3d24", M, D)


def palette_grid(nx, ny, nz):
    """A 7-point grid with values redrawn from a 24-entry palette, diagonal 10."""
    M = O.generate("poisson3d", nx, ny, nz)
    pal = np.random.default_rng(9).standard_normal(24)
    val = pal[np.random.default_rng(10).integers(0, 24, M.nnz)]
    rows = np.repeat(np.arange(M.nrows), np.diff(M.rowptr))
    val[M.col == rows] = 10.0
    return O.CSR(M.rowptr.copy(), M.col.copy(), val, M.ncols)


@pytest.mark.parametrize("pair", [1, 0])
@pytest.mark.parametrize("name", ["grid19", "palette17"])
def test_layout_ell(ctx, name, pair):
    """k_rows_ell, paired and with separate offset / value tables."""
    M = O.generate("poisson3d", 19, 19, 19) if name == "grid19" else palette_grid(17, 17, 17)
    with options(ell_min_rows=0, sym_dia=0, ell_pair=pair, ell_xwin=0):
        D = upload(ctx, M)
    lay = layout_of(D)
    assert lay["ell"] and not lay["ell_xwin"] and lay["ell_pair"] == bool(pair), lay
    run_smoother(ctx, name, M, D)


def from_coo(rows, cols, vals, n):
    import scipy.sparse as sp
    T = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    T.sort_indices()
    return O.CSR(T.indptr.astype(np.int64), T.indices.astype(np.int64), T.data.copy(), n)


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


def two_blocks():
    """Two 2048-row diagonal blocks: a tridiagonal one and one whose rows take the diagonal and 20 of
    40 fixed offsets within +-3000 (entries outside the block dropped; 4 values)."""
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
    return from_coo(rows, cols, vals, 2 * h)


def test_layout_ellw_regrouped(ctx):
    """k_rows_ellw, 128 x 7 x 5: non-consecutive coupled groups and a short last group."""
    M = palette_grid(128, 7, 5)
    with options(ell_min_rows=0, sym_dia=0):
        D = upload(ctx, M)
    lay = layout_of(D)
    assert lay["ell_xwin"] and lay["ell_gather_groups"] == 0 and lay["ell_xwin_noncontig_groups"] >= 1, lay
    run_smoother(ctx, "palette128x7x5", M, D)


def test_layout_ellw_partial_last_slice(ctx):
    """100 x 7 x 6: 65 full slices and one of 40 rows."""
    M = palette_grid(100, 7, 6)
    with options(ell_min_rows=0, sym_dia=0):
        D = upload(ctx, M)
    lay = layout_of(D)
    assert lay["ell_xwin"] and lay["ell_gather_groups"] == 0, lay
    run_smoother(ctx, "palette100x7x6", M, D)


def test_layout_ellw_clipped_windows_unaligned_x(ctx):
    """The banded matrix of 999 rows: windows clipped at column 0 and at the last column (n odd: the
    last 16-byte window load starts at an even column and reaches one double into the vector's pad)."""
    M = banded(999)
    with options(ell_min_rows=0, sym_dia=0):
        D = upload(ctx, M)
    lay = layout_of(D)
    assert lay["ell_xwin"] and lay["ell_gather_groups"] == 0 and lay["ell_xwin_groups"] >= 4, lay
    run_smoother(ctx, "banded999", M, D)


def test_layout_ellw_windowed_and_gathering_groups(ctx):
    """The two-block matrix with ell_xwin_max 1024: windowed and gathering groups in one launch."""
    M = two_blocks()
    with options(ell_min_rows=0, sym_dia=0, ell_xwin_max=1024):
        D = upload(ctx, M)
    lay = layout_of(D)
    assert lay["ell_xwin"] and lay["ell_xwin_groups"] > 0 and lay["ell_gather_groups"] > 0, lay
    run_smoother(ctx, "two_blocks", M, D)


def ragged_with_diagonal():
    """The 3000-row ragged matrix (empty and one-entry rows, columns within 60 of the row), every row
    given the diagonal 12."""
    n = 3000
    rng = np.random.default_rng(4)
    rows, cols, vals = [], [], []
    for i in range(n):
        if i % 97 == 0:
            continue
        k = 1 if i % 13 == 0 else int(rng.integers(2, 40))
        cs = np.unique(np.clip(i + rng.integers(-60, 60, k), 0, n - 1))
        cs = cs[cs != i]
        rows += [i] * len(cs)
        cols += cs.tolist()
        vals += (rng.integers(1, 9, len(cs)) * 0.25).tolist()
    rows += list(range(n))
    cols += list(range(n))
    vals += [12.0] * n
    return from_coo(rows, cols, vals, n)


@pytest.mark.parametrize("name", ["elastic6", "ragged_diag"])
def test_layout_tiles(ctx, name):
    """k_rows_tile2 and k_rows_tm: 1024- and 4096-nonzero tiles, descriptor-driven and tile-major."""
    M = O.generate("elastic3d", 6, 6, 6) if name == "elastic6" else ragged_with_diagonal()
    seen = set()
    for tile_nnz in (1024, 4096):
        for tile_major in (0, 2):
            with options(sym_dia=0, ell=0, tile_nnz=tile_nnz, long_tiles=0, tile_major=tile_major):
                D = upload(ctx, M)
            lay = layout_of(D)
            assert not lay["sym"] and not lay["ell"] and lay["tiles"] > 0 and lay["tile_nnz"] == tile_nnz, lay
            assert not (tile_major == 0 and lay["tm"]), lay
            seen.add((tile_nnz, lay["tm"]))
            run_smoother(ctx, name, M, D)
    assert (1024, True) in seen and (1024, False) in seen, seen


@pytest.mark.parametrize("n", [400, 1100])
def test_layout_long_rows(ctx, n):
    """A dense matrix: rows of 400 nonzeros in 1024-nonzero tiles, and rows of 1100 — longer than the
    tile budget, one workgroup per row in k_rows_long."""
    rng = np.random.default_rng(12)
    a = rng.standard_normal((n, n))
    a[np.arange(n), np.arange(n)] = float(n)
    M = dense_csr(a)
    with options(sym_dia=0, ell=0, tile_nnz=1024, long_tiles=0):
        D = upload(ctx, M)
    lay = layout_of(D)
    assert not lay["sym"] and not lay["ell"], lay
    assert (lay["tiles"] == 0) == (n == 1100), lay  # (1100: no short tile at all)
    run_smoother(ctx, f"dense{n}", M, D)


@pytest.fixture(scope="module")
def small_hierarchy(ctx):
    be = pa.SequentialBackend(1)
    A, offs, _xs = pa.generate_problem(be, "poisson3d", 16)
    return pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=200), device=ctx)


def test_restriction_and_prolongation_are_refused(ctx, small_hierarchy):
    lp = small_hierarchy.levels[0][0]
    for M in (lp.R, lp.P):
        D = PSparseMatrix(ctx, M)
        x, t1, t2 = D.new_input_vector(), D.new_input_vector(), D.new_input_vector()
        b = D.new_output_vector()
        with pytest.raises(PamgError) as e:
            chebyshev(x, D, b, t1, t2, lmax=LMAX, ratio=RATIO, degree=DEG)
        assert e.value.code == -1, e.value  # PAMG_E_ARG


def test_argument_errors(ctx):
    M = O.generate("poisson3d", 8, 8, 8)
    D = upload(ctx, M)
    x, t1, t2, b = (D.new_input_vector() for _ in range(4))
    for kw in (dict(lmax=2.0, ratio=1.0, degree=2), dict(lmax=0.0, ratio=4.0, degree=2),
               dict(lmax=2.0, ratio=4.0, degree=0), dict(lmax=2.0, ratio=4.0, degree=65)):
        with pytest.raises(PamgError) as e:
            chebyshev(x, D, b, t1, t2, **kw)
        assert e.value.code == -1
    for args in ((x, D, b, x, t2), (x, D, b, t1, t1), (x, D, x, t1, t2), (x, D, b, t1, b)):  # aliasing
        with pytest.raises(PamgError) as e:
            chebyshev(*args, lmax=2.0, ratio=4.0, degree=2)
        assert e.value.code == -1


# ------------------------------------------------------------------------------ cycles
PROBLEMS = {"poisson3d24": ("poisson3d", 24, 100), "aniso3d20": ("aniso3d", 20, 300),
            "elastic3d12": ("elastic3d", 12, 1000), "poisson3d64": ("poisson3d", 64, 1000),
            # with ell_min_rows 0: the level-1 operator (4192 rows) in the windowed sliced ELL
            "poisson3d32_ell": ("poisson3d", 32, 100)}
_problems = {}


def problem(ctx, name):
    """Device solver, right-hand side, oracle hierarchy and restatement of a problem, built once."""
    if name not in _problems:
        kind, n, mc = PROBLEMS[name]
        be = pa.SequentialBackend(1)
        Ah, offs, xs = pa.generate_problem(be, kind, n)
        H = pa.build_hierarchy(be, Ah, offs, pa.SAParams(max_coarse=mc), device=ctx)
        with options(ell_min_rows=0) if name.endswith("_ell") else contextlib.nullcontext():
            S = AMGSolver(ctx, H)
        b = PVector(ctx, S.A[0].nrows)
        mul(b, S.A[0], PVector(ctx, S.A[0].nrows, 0, xs[0]))
        Ao = O.generate(kind, *O.grid_shape(kind, n))
        bo = O.spmv(Ao, O.xstar(Ao.nrows))
        assert np.array_equal(bits(b.own_values()), bits(bo))
        Ho = O.setup(Ao, max_coarse=mc)
        assert Ho.nlevels == H.nlevels
        assert [H.levels[l][0].rho for l in range(H.nlevels)] == list(Ho.rho)
        _problems[name] = (S, b, bo, Ho, CycleRef(Ho), {"hierarchy": H})
    return _problems[name]


def ref_solve(ref, cache, bo, nu1, nu2):
    if (nu1, nu2) not in cache:
        cache[(nu1, nu2)] = ref.solve(bo, 3, nu1, nu2)
    return cache[(nu1, nu2)]


@pytest.mark.parametrize("nu", [(2, 2), (3, 1)])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_cycle_bits(ctx, name, nu):
    """3 stationary cycles from x = 0, ratio 4: the restatement's x bits and residual history, from the
    captured graph and from eager launches."""
    S, b, bo, _Ho, ref, cache = problem(ctx, name)
    if name == "poisson3d64":  # the default upload: k_sym_zm beside the neighbour-coded P (at this size level 1,
        l0 = layout_of(S.A_dev[0])  # ~33k rows, is under ell_min_rows and R0 keeps anchored dictionary tiles)
        assert l0["sym"] and l0["sym_vd"] and l0["jr_fused"], l0
        assert layout_of(S.P[0])["pnc"]
    if name == "poisson3d32_ell":
        l1 = layout_of(S.A_dev[1])
        assert l1["ell"] and l1["ell_xwin"], l1
    xo, ho = ref_solve(ref, cache, bo, *nu)
    S.set_smoother("chebyshev", ratio=4.0)
    S.set_sweeps(*nu)
    try:
        for graph in (True, False):
            S.set_graph(graph)
            x = S.new_vector()
            hist = S.vcycle(x, b, 3, res_hist=True)
            assert np.array_equal(bits(x.own_values()), bits(xo)), (name, nu, graph)
            np.testing.assert_allclose(hist, ho, rtol=1e-12)
            assert S.graph_state()["captured"] == graph
            assert not S.graph_state()["failed"]
    finally:
        S.set_graph(True)
        S.set_smoother("jacobi")
        S.set_sweeps(1, 1)


# Every remainder of the two degrees mod 3 (the polynomial's iterates rotate through three vectors), on
# both sides of the spare vector's rule: it is needed where exactly one degree is a multiple of 3.
PAIRS = [(nu1, nu2) for nu1 in (1, 2, 3, 4) for nu2 in (1, 2, 3, 4)]


def pcg_bits_ref(cycle, A, b, maxit):
    """maxit iterations of SPEC §S8 from x = 0 (no convergence test) in the device's arithmetic: the dots
    as test_gpu_reductions restates them, the updates rounded as axpby rounds them, z = cycle(r) from a
    zero guess. Returns x and the history of ||r||."""
    from test_gpu_reductions import restated_dot
    x = np.zeros(len(b))
    r = O.residual(A, x, b)
    hist = [np.sqrt(np.float64(restated_dot(r, r)))]
    z = cycle(r)
    p, rz = z.copy(), restated_dot(r, z)
    for k in range(maxit):
        q = O.spmv(A, p)
        alpha = rz / restated_dot(p, q)
        x = alpha * p + 1.0 * x
        r = (-alpha) * q + 1.0 * r
        hist.append(np.sqrt(np.float64(restated_dot(r, r))))
        if k + 1 < maxit:
            z = cycle(r)
            rz, rz_old = restated_dot(r, z), rz
            p = 1.0 * z + (rz / rz_old) * p
    return x, np.array(hist)


@pytest.mark.parametrize("nu", PAIRS)
def test_cycle_bits_every_degree_pair(ctx, nu):
    """poisson3d 24 (three levels: a three-vector ring on two of them), 2 stationary cycles from a given
    guess: the restatement's x bits, from the captured graph and from eager launches."""
    S, b, bo, _Ho, ref, cache = problem(ctx, "poisson3d24")
    assert S.L >= 3
    if ("two", nu) not in cache:
        cache[("two", nu)] = ref.solve(bo, 2, *nu)
    xo, ho = cache[("two", nu)]
    S.set_smoother("chebyshev", ratio=4.0)
    S.set_sweeps(*nu)
    try:
        for graph in (True, False):
            S.set_graph(graph)
            x = S.new_vector()
            hist = S.vcycle(x, b, 2, res_hist=True)
            assert np.array_equal(bits(x.own_values()), bits(xo)), (nu, graph)
            np.testing.assert_allclose(hist, ho, rtol=1e-12)
            assert S.graph_state()["captured"] == graph
            assert not S.graph_state()["failed"]
    finally:
        S.set_graph(True)
        S.set_smoother("jacobi")
        S.set_sweeps(1, 1)


@pytest.mark.parametrize("nu", PAIRS)
def test_pcg_bits_every_degree_pair(ctx, nu):
    """2 PCG iterations: every cycle starts from a zero guess (the level-0 zero-guess rings). x and the
    residual history are the restated iteration's bits, from pamg_pcg and from the device-resident
    iteration (whose second half enqueues the cycle itself)."""
    S, b, bo, Ho, ref, _cache = problem(ctx, "poisson3d24")
    xo, ho = pcg_bits_ref(lambda r: ref.cycle(0, None, r, *nu), Ho.A[0], bo, 2)
    S.set_smoother("chebyshev", ratio=4.0)
    S.set_sweeps(*nu)
    try:
        for lookahead in (None, 0):
            x = S.new_vector()
            k, hist = S.pcg(x, b, 0.0, 2, lookahead=lookahead)
            assert k == 2
            assert np.array_equal(bits(x.own_values()), bits(xo)), (nu, lookahead)
            assert np.array_equal(bits(hist), bits(ho)), (nu, lookahead)
    finally:
        S.set_smoother("jacobi")
        S.set_sweeps(1, 1)


def test_spare_vector_history(ctx):
    """poisson3d 64 runs the cross-cycle pipeline: after 3 Jacobi V(1,1) cycles the solver owns the spare
    level-0 vector. Chebyshev V(1,3), V(3,1), V(3,3) and V(2,2) on it then give the bits of a solver on
    the same hierarchy that never pipelined: only the degrees decide which cycles use that vector."""
    piped, b, _bo, _Ho, _ref, cache = problem(ctx, "poisson3d64")
    assert piped.bench_chain(piped.new_vector(), b, 1) is not None  # (this hierarchy does pipeline)
    piped.vcycle(piped.new_vector(), b, 3)
    fresh = AMGSolver(ctx, cache["hierarchy"])
    try:
        for nu in ((1, 3), (3, 1), (3, 3), (2, 2)):
            got = []
            for S in (piped, fresh):
                S.set_smoother("chebyshev", ratio=4.0)
                S.set_sweeps(*nu)
                x = S.new_vector()
                S.vcycle(x, b, 2)
                got.append(bits(x.own_values()))
            assert np.array_equal(got[0], got[1]), nu
    finally:
        piped.set_smoother("jacobi")
        piped.set_sweeps(1, 1)


def test_residuals_match_the_recorded_convergence(ctx):
    """The restatement reproduces the convergence the smoother was proposed with: relative residual
    after 5 Chebyshev V(2,2) cycles on poisson3d 24 (max_coarse 100) 1.4e-5, against 1.8e-4 for Jacobi
    V(2,2)."""
    _S, _b, bo, Ho, ref, _c = problem(ctx, "poisson3d24")
    _x, h = ref.solve(bo, 5, 2, 2)
    rel = h[-1] / np.linalg.norm(bo)
    assert 1.35e-5 < rel < 1.45e-5, rel
    Ho.set_sweeps(2, 2)
    try:
        _xj, hj = Ho.solve(bo, 5, res_hist=True)
    finally:
        Ho.set_sweeps(1, 1)
    assert rel < 0.1 * hj[-1] / np.linalg.norm(bo)


def test_switching_back_leaves_no_state(ctx):
    """Chebyshev cycles, then "jacobi" and V(1,1): the next cycles are the oracle's Jacobi cycles (the
    cross-cycle pipeline included: 3 cycles in one run), bit for bit."""
    S, b, bo, Ho, _ref, _c = problem(ctx, "poisson3d24")
    S.set_smoother("chebyshev", ratio=4.0)
    S.set_sweeps(3, 1)
    x = S.new_vector()
    S.vcycle(x, b, 2)
    S.set_smoother("jacobi")
    S.set_sweeps(1, 1)
    xo, ho = Ho.solve(bo, 3, res_hist=True)
    x = S.new_vector()
    hist = S.vcycle(x, b, 3, res_hist=True)
    assert np.array_equal(bits(x.own_values()), bits(xo))
    np.testing.assert_allclose(hist, ho, rtol=1e-12)
    x = S.new_vector()
    S.vcycle(x, b, 3)
    assert np.array_equal(bits(x.own_values()), bits(xo))


def test_degree_one_is_jacobi_with_omega_one_over_theta(ctx):
    """Chebyshev V(1,1) against the oracle's own Jacobi V(1,1) on the same operators with omega_l =
    c2_0 of level l."""
    S, b, bo, Ho, _ref, _c = problem(ctx, "poisson3d24")
    om = [coeffs_ref(Ho.rho[l], 4.0, 1)[1][0] for l in range(Ho.nlevels)]
    Hj = O.hierarchy_from_levels(Ho.A, Ho.P, Ho.R, om, np.ascontiguousarray(Ho.ainv.T).reshape(-1))
    xo = Hj.solve(bo, 3)
    S.set_smoother("chebyshev", ratio=4.0)
    try:
        x = S.new_vector()
        S.vcycle(x, b, 3)
        assert np.array_equal(bits(x.own_values()), bits(xo))
    finally:
        S.set_smoother("jacobi")


def test_reorder_keeps_the_bits(ctx):
    """elastic3d 6 with every level renumbered (reorder "on"): the unpermuted run's x, which is the
    restatement's."""
    be = pa.SequentialBackend(1)
    Ah, offs, xs = pa.generate_problem(be, "elastic3d", 6)
    H = pa.build_hierarchy(be, Ah, offs, pa.SAParams(max_coarse=100), device=ctx)
    Ao = O.generate("elastic3d", 6, 6, 6)
    bo = O.spmv(Ao, O.xstar(Ao.nrows))
    xo, _ho = CycleRef(O.setup(Ao, max_coarse=100)).solve(bo, 3, 2, 2)
    got = {}
    for reorder in ("off", "on"):
        S = AMGSolver(ctx, H, reorder=reorder)
        assert bool(S.reordered) == (reorder == "on")
        A0 = S.A[0]
        b = PVector(ctx, A0.nrows)
        mul(b, A0, PVector(ctx, A0.nrows, 0, xs[0]))
        S.set_smoother("chebyshev", ratio=4.0)
        S.set_sweeps(2, 2)
        x = S.new_vector()
        S.vcycle(x, b, 3)
        got[reorder] = bits(x.own_values())
    assert np.array_equal(got["on"], got["off"])
    assert np.array_equal(got["off"], bits(xo))


def test_pcg(ctx):
    """PCG to 1e-8 preconditioned by one Chebyshev V(2,2) cycle from zero: the restated PCG's iteration
    count (8 on the CPU), its x to 1e-8, and no more iterations than the oracle's Jacobi V(2,2) (10)."""
    S, b, bo, Ho, ref, _c = problem(ctx, "poisson3d24")
    xr, kr = ref.pcg(bo, 1e-8, 60, 2, 2)
    Ho.set_sweeps(2, 2)
    try:
        _xj, kj, _hj = Ho.pcg(bo, 1e-8, 60)
    finally:
        Ho.set_sweeps(1, 1)
    S.set_smoother("chebyshev", ratio=4.0)
    S.set_sweeps(2, 2)
    try:
        x = S.new_vector()
        k, hist = S.pcg(x, b, 1e-8, 60)
    finally:
        S.set_smoother("jacobi")
        S.set_sweeps(1, 1)
    print(f"\n  pcg iterations: device {k}, restatement {kr}, oracle Jacobi V(2,2) {kj}")
    assert k == kr
    assert np.linalg.norm(x.own_values() - xr) <= 1e-8 * np.linalg.norm(xr)
    assert k <= kj
    assert hist[-1] <= 1e-8 * hist[0]


def test_profile_slots_and_bench_chain(ctx):
    """The profiling slots keep their meaning (jacobi_pre / jacobi_post hold the polynomials), and the
    pipeline's chain benchmark refuses a Chebyshev hierarchy."""
    S, b, _bo, _Ho, _ref, _c = problem(ctx, "poisson3d64")
    x = S.new_vector()
    assert S.bench_chain(x, b, 1) is not None
    S.set_smoother("chebyshev", ratio=4.0)
    S.set_sweeps(2, 2)
    try:
        assert S.bench_chain(x, b, 1) is None
        with pytest.raises(PamgError) as e:
            call("pamg_hier_bench_chain", S.handle, x.handle, b.handle, 1, ctypes.byref(ctypes.c_double()))
        assert e.value.code == -6  # PAMG_E_STATE
        ms = S.profile(S.new_vector(), b, 1)
        assert ms[0, 0] > 0 and ms[0, 4] > 0 and ms[0, 1] > 0, ms
    finally:
        S.set_smoother("jacobi")
        S.set_sweeps(1, 1)


def test_bench_rowop_chebyshev_step(ctx):
    """pamg_bench_rowop op 6: one step k >= 1 with c1 = c2 = omega and a zero x_{k-1}."""
    M = palette_grid(17, 17, 17)
    with options(ell_min_rows=0, sym_dia=0):
        D = upload(ctx, M)
    rng = np.random.default_rng(5)
    xh, bh = rng.standard_normal(M.nrows), rng.standard_normal(M.nrows)
    x, b, y = PVector(ctx, M.nrows, 0, xh), PVector(ctx, M.nrows, 0, bh), PVector(ctx, M.nrows)
    ms = ctypes.c_double()
    call("pamg_bench_rowop", ctx.handle, D.handle, 6, x.handle, b.handle, y.handle, 0.375, 2, ctypes.byref(ms))
    u = O.residual(M, xh, bh)
    want = xh + ((0.375 * (xh - 0.0)) + ((0.375 * u) / diag_of(M)))
    assert np.array_equal(bits(y.own_values()), bits(want))
    assert ms.value > 0


# ------------------------------------------------------------------------------ several parts
@pytest.mark.parametrize("nparts,n,max_coarse,agglomerate", [(2, 20, 100, 0), (4, 24, 60, 0), (2, 64, 1000, 32768)])
def test_parts_cycle_bits(built, nparts, n, max_coarse, agglomerate):
    """Chebyshev V(2,2), 3 cycles on several parts (in-process transport, ghost slots poisoned before
    each exchange): the concatenated x is the restatement's on the global operators of the oracle's
    decoupled setup, and pamg_world_vcycle gives the same bits."""
    kind, ncycles = "poisson3d", 3
    with options(poison_ghosts=1):
        W = LocalWorld(nparts)
        try:
            be = pa.SequentialBackend(nparts)
            A, offs, xs = pa.generate_problem(be, kind, n)
            H = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=max_coarse, agglomerate=agglomerate),
                                   device=W.ctxs[0])
            S = [AMGSolver(W.ctxs[p], H, part=p) for p in range(nparts)]
            for s in S:
                s.set_smoother("chebyshev", ratio=4.0)
                s.set_sweeps(2, 2)
            A0 = [s.A[0] for s in S]
            lays = [layout_of(a) for a in A0]
            xst = [PVector(W.ctxs[p], A0[p].n_own_cols, A0[p].n_ghost, xs[p]) for p in range(nparts)]
            b = [PVector(W.ctxs[p], A0[p].nrows) for p in range(nparts)]
            W.run(lambda p: mul(b[p], A0[p], xst[p]))
            x = [s.new_vector() for s in S]
            hist = W.run(lambda p: S[p].vcycle(x[p], b[p], ncycles, res_hist=True))
            xw = [s.new_vector() for s in S]
            arr = lambda objs: (ctypes.c_void_p * nparts)(*[o.handle for o in objs])  # noqa: E731
            hw = np.zeros(ncycles)
            call("pamg_world_vcycle", W._h, arr(S), arr(xw), arr(b), ncycles, hw.ctypes.data_as(ctypes.c_void_p))
            got_x = np.concatenate([v.own_values() for v in x])
            got_w = np.concatenate([v.own_values() for v in xw])
            rho = [H.levels[l][0].rho for l in range(H.nlevels)]
        finally:
            del S
            W.close()
    if n == 64:  # z-slabs in the symmetric layout: k_rows_symd + k_cheb_update inside, tiles on the faces
        assert all(lay["sym"] for lay in lays), lays
    Ao = O.generate(kind, *O.grid_shape(kind, n))
    bo = O.spmv(Ao, O.xstar(Ao.nrows))
    Ho = O.setup(Ao, nparts=nparts, max_coarse=max_coarse, agglomerate=agglomerate)
    assert rho == list(Ho.rho)
    xo, ho = CycleRef(Ho).solve(bo, ncycles, 2, 2)
    assert np.array_equal(bits(got_x), bits(xo))
    assert np.array_equal(bits(got_w), bits(xo))
    np.testing.assert_allclose(hist[0], ho, rtol=1e-12)
    assert np.array_equal(hw, hist[0])
