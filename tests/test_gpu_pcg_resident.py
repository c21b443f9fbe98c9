"""pamg_pcg_resident (SPEC §S11): PCG with alpha, beta, rho and r.r in device memory, the iteration
replayed as two graphs, against pamg_pcg on the same hierarchy — bit for bit in x, the iteration
count and the residual history, for every lookahead, with graphs on and off. pamg_pcg itself is
pinned to the oracle by test_gpu_parity.py::test_pcg_matches_oracle and the 512^3 tests; the
oracle's own PCG is compared here as well (§S8's tolerances).

The problems are the smallest that reach each shape of the reductions (dot_partials: 256-row
blocks, at most 1,024 of them): less than one block, a whole number of blocks, a ragged last block,
and more than 262,144 rows (the grid-stride loop wraps, ragged tail)."""
import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd._lib import PamgError
from parallel_amg_amd.partitioned import LocalWorld, PVector, mul
from parallel_amg_amd.solver import AMGSolver

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -6


def bits(a):
    return np.asarray(a, np.float64).view(np.int64)


# name -> (kind, n, max_coarse or None for the default, permutation seed or None, rows)
PROBLEMS = {
    "poisson2d_12_one_level": ("poisson2d", 12, None, None, 144),
    "poisson2d_12": ("poisson2d", 12, 20, None, 144),
    "elastic3d_8": ("elastic3d", 8, 100, None, 1536),
    "poisson3d_12": ("poisson3d", 12, 100, None, 1728),
    "aniso3d_12": ("aniso3d", 12, 100, None, 1728),
    "poisson2d_520": ("poisson2d", 520, 1000, None, 270400),
    "poisson3d_20_shuffled": ("poisson3d", 20, 100, 5, 8000),
}
# name -> (smoother, nu1, nu2, lmax)
SMOOTHERS = {
    "j11": ("jacobi", 1, 1, "gershgorin"),
    "j22": ("jacobi", 2, 2, "gershgorin"),
    "c22": ("chebyshev", 2, 2, "gershgorin"),
    "c33": ("chebyshev", 3, 3, "gershgorin"),
    "c22e": ("chebyshev", 2, 2, "estimate"),
}
CASES = [(p, s) for p in PROBLEMS for s in SMOOTHERS if p != "poisson2d_520" or s in ("j11", "c22")]

_cache = {}


def problem(ctx, name):
    """(solver, b, x*) of a problem, set up once per session and shared (read-only b)."""
    if name not in _cache:
        kind, n, max_coarse, seed, rows = PROBLEMS[name]
        be = pa.SequentialBackend(1)
        A, offs, xs = pa.generate_problem(be, kind, n)
        if seed is not None:
            A, xs = pa.permute_problem(A, xs, seed)
        params = pa.SAParams() if max_coarse is None else pa.SAParams(max_coarse=max_coarse)
        H = pa.build_hierarchy(be, A, offs, params, device=ctx)
        S = AMGSolver(ctx, H, reorder="auto")
        Af = S.fine_operator()
        assert Af.nrows == rows
        b = PVector(ctx, Af.nrows)
        mul(b, Af, PVector(ctx, Af.n_own_cols, Af.n_ghost, xs[0]))
        _cache[name] = (S, b, xs[0])
    return _cache[name]


def configure(S, smoother):
    kind, nu1, nu2, lmax = SMOOTHERS[smoother]
    S.set_smoother(kind, lmax=lmax)
    S.set_sweeps(nu1, nu2)


def check_stats(S, iters, maxit, lookahead):
    enq, late = S.last_pcg_stats
    assert enq <= maxit
    assert late == enq - iters
    assert 0 <= late <= lookahead
    if lookahead == 0:
        assert late == 0
    return late


def same_as_reference(S, b, rtol, maxit, lookahead, ref, x0=None):
    """One resident solve; x, the count and the history must carry ref's bits. Returns the
    number of iterations run past convergence."""
    k0, h0, x0bits = ref
    x = S.new_vector()
    if x0 is not None:
        x.set(x0)
    k, h = S.pcg(x, b, rtol, maxit, lookahead=lookahead)
    assert k == k0
    assert np.array_equal(bits(h), bits(h0)), (lookahead, h, h0)
    assert np.array_equal(bits(x.own_values()), x0bits), lookahead
    return check_stats(S, k, maxit, lookahead)


def reference(S, b, rtol, maxit, x0=None):
    x = S.new_vector()
    if x0 is not None:
        x.set(x0)
    k, h = S.pcg(x, b, rtol, maxit)
    assert S.last_pcg_stats is None
    return k, h.copy(), bits(x.own_values()).copy()


@pytest.mark.parametrize("name,smoother", CASES)
def test_bits_of_pamg_pcg(ctx, name, smoother):
    S, b, _xs = problem(ctx, name)
    if name == "poisson3d_20_shuffled":
        assert 0 in S.reordered  # the DeviceSpace permutation path
    if name == "poisson2d_12_one_level":
        assert S.L == 1  # the V-cycle is the dense solve
    configure(S, smoother)
    try:
        ref = reference(S, b, 1e-8, 60)
        assert 0 < ref[0] < 60
        for graph in (True, False):
            S.set_graph(graph)
            for lookahead in (0, 1, 3):
                same_as_reference(S, b, 1e-8, 60, lookahead, ref)
    finally:
        S.set_graph(True)


@pytest.fixture
def p12(ctx):
    S, b, xs = problem(ctx, "poisson3d_12")
    configure(S, "j11")
    S.set_graph(True)
    return S, b, xs


def test_late_iterations_leave_x_r_and_history(ctx):
    """lookahead = 3 on runs that converge with k* + 1 <= maxit: iterations are enqueued past
    convergence (each runs its SpMV and V-cycle) and x, the history (whose last entry is the norm
    of the recurrence's r) and b - A x (the ||r_0|| of a second call with maxit = 0) keep
    pamg_pcg's bits. How many run late depends on how far the host is ahead of the stream: on
    the large problem the host enqueues far faster than the device runs, so at least one
    parametrisation must show some."""
    late = []
    for name in ("poisson3d_12", "poisson2d_520"):
        S, b, _xs = problem(ctx, name)
        configure(S, "j11")
        S.set_graph(True)
        k0, h0, xb = reference(S, b, 1e-6, 60)
        assert k0 + 1 <= 60
        x = S.new_vector()
        k, h = S.pcg(x, b, 1e-6, 60, lookahead=3)
        late.append(check_stats(S, k, 60, 3))
        assert k == k0 and np.array_equal(bits(h), bits(h0))
        assert np.array_equal(bits(x.own_values()), xb)
        xr = S.new_vector()
        xr.set(xb.view(np.float64))
        kr, hr = S.pcg(xr, b, 1e-6, 0)
        k2, h2 = S.pcg(x, b, 1e-6, 0, lookahead=3)
        assert kr == k2 == 0 and np.array_equal(bits(hr), bits(h2))
        assert S.last_pcg_stats == (0, 0)
    print(f"\n  iterations run past convergence at lookahead 3: {late}")
    assert max(late) >= 1, late


def test_maxit_zero_and_zero_rhs(ctx, p12):
    S, b, xs = p12
    for lookahead in (0, 1, 3):
        x = S.new_vector()
        x.set(xs * 0.5)
        before = bits(x.own_values()).copy()
        k, h = S.pcg(x, b, 1e-8, 0, lookahead=lookahead)
        assert S.last_pcg_stats == (0, 0)
        xr = S.new_vector()
        xr.set(xs * 0.5)
        kr, hr = S.pcg(xr, b, 1e-8, 0)
        assert k == kr == 0 and np.array_equal(bits(h), bits(hr)) and len(h) == 1
        assert np.array_equal(bits(x.own_values()), before)
        # b = 0 from x = 0: ||r_0|| = 0, no iteration, x untouched
        zero = PVector(ctx, len(xs))
        x = S.new_vector()
        k, h = S.pcg(x, zero, 1e-8, 50, lookahead=lookahead)
        assert k == 0 and h[0] == 0.0 and S.last_pcg_stats == (0, 0)
        assert not x.own_values().any()


@pytest.mark.parametrize("lookahead", [0, 1, 3])
def test_nonzero_guess_and_rtol_zero(p12, lookahead):
    S, b, xs = p12
    x0 = np.cos(np.arange(len(xs), dtype=np.float64))
    ref = reference(S, b, 1e-9, 60, x0=x0)
    same_as_reference(S, b, 1e-9, 60, lookahead, ref, x0=x0)
    ref = reference(S, b, 0.0, 3)
    assert ref[0] == 3
    assert same_as_reference(S, b, 0.0, 3, lookahead, ref) == 0


def test_maxit_at_and_below_the_count(p12):
    S, b, _xs = p12
    kstar = reference(S, b, 1e-10, 60)[0]
    assert 3 <= kstar < 30
    for maxit in (kstar, kstar - 1):
        ref = reference(S, b, 1e-10, maxit)
        assert ref[0] == maxit
        for lookahead in (0, 1, 3, 7):
            assert same_as_reference(S, b, 1e-10, maxit, lookahead, ref) == 0
    # a lookahead beyond the whole solve: k* + lookahead iterations are enqueued before the wait
    # that shows the outcome
    ref = reference(S, b, 1e-10, 60)
    for lookahead in (7, kstar + 2):
        same_as_reference(S, b, 1e-10, 60, lookahead, ref)


def test_recapture_set_sweeps_and_interleaving(p12):
    S, b, _xs = p12
    ref = reference(S, b, 1e-10, 60)
    # two solves in a row into different x vectors (same_as_reference makes a new one each time):
    # the first half's graph holds x, so the second solve recaptures
    same_as_reference(S, b, 1e-10, 60, 1, ref)
    same_as_reference(S, b, 1e-10, 60, 1, ref)
    assert S.graph_state()["enabled"] and not S.graph_state()["failed"]
    # new sweep counts drop the graphs
    S.set_sweeps(2, 2)
    try:
        ref22 = reference(S, b, 1e-10, 60)
        assert ref22[0] < ref[0]
        same_as_reference(S, b, 1e-10, 60, 1, ref22)
        same_as_reference(S, b, 1e-10, 60, 0, ref22)
    finally:
        S.set_sweeps(1, 1)
    # the two entry points share the hierarchy's r, z, p, q
    for lookahead in (0, 3, 1):
        same_as_reference(S, b, 1e-10, 60, lookahead, ref)
        again = reference(S, b, 1e-10, 60)
        assert again[0] == ref[0] and np.array_equal(again[1], ref[1]) and np.array_equal(again[2], ref[2])


def test_bad_arguments(p12):
    S, b, _xs = p12
    x = S.new_vector()
    for rtol, maxit, lookahead in ((1e-8, 10, -1), (1e-8, -1, 0), (float("nan"), 10, 0), (-1.0, 10, 0)):
        with pytest.raises(PamgError) as e:
            S.pcg(x, b, rtol, maxit, lookahead=lookahead)
        assert e.value.code == E_ARG


@pytest.mark.parametrize("name", ["poisson3d_12", "aniso3d_12"])
def test_matches_oracle(ctx, name):
    """§S8's tolerances, as in test_pcg_matches_oracle: equal iteration counts, the history to
    1e-6, x to 1e-8 relative."""
    S, b, xs = problem(ctx, name)
    configure(S, "j11")
    kind, n, max_coarse, _seed, _rows = PROBLEMS[name]
    Ao = O.generate(kind, *O.grid_shape(kind, n))
    bo = O.spmv(Ao, O.xstar(Ao.nrows))
    assert np.array_equal(bits(b.own_values()), bits(bo))
    Ho = O.setup(Ao, max_coarse=max_coarse)
    xo, ko, ho = Ho.pcg(bo, 1e-10, 60)
    for lookahead in (0, 1, 3):
        x = S.new_vector()
        k, h = S.pcg(x, b, 1e-10, 60, lookahead=lookahead)
        assert k == ko
        np.testing.assert_allclose(h, ho, rtol=1e-6)
        assert np.linalg.norm(x.own_values() - xo) <= 1e-8 * np.linalg.norm(xo)


def test_several_parts_are_refused(built):
    """A context of a two-part world gets PAMG_E_STATE, part by part on one thread: nothing is
    exchanged (a rendezvous would wait for the sibling), and the world works afterwards."""
    W = LocalWorld(2)
    try:
        be = pa.SequentialBackend(2)
        A, offs, xs = pa.generate_problem(be, "poisson3d", 12)
        H = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=100), device=W.ctxs[0])
        S = [AMGSolver(W.ctxs[p], H, part=p) for p in range(2)]
        A0 = [s.A[0] for s in S]
        xst = [PVector(W.ctxs[p], A0[p].n_own_cols, A0[p].n_ghost, xs[p]) for p in range(2)]
        b = [PVector(W.ctxs[p], A0[p].nrows) for p in range(2)]
        W.run(lambda p: mul(b[p], A0[p], xst[p]))
        first = W.run(lambda p: S[p].pcg(S[p].new_vector(), b[p], rtol=1e-8, maxit=60))
        for lookahead in (0, 2):
            for p in range(2):
                with pytest.raises(PamgError) as e:
                    S[p].pcg(S[p].new_vector(), b[p], 1e-8, 60, lookahead=lookahead)
                assert e.value.code == E_STATE
        assert not W.broken
        again = W.run(lambda p: S[p].pcg(S[p].new_vector(), b[p], rtol=1e-8, maxit=60))
        for p in range(2):
            assert again[p][0] == first[p][0] and np.array_equal(bits(again[p][1]), bits(first[p][1]))
    finally:
        del S
        W.close()
