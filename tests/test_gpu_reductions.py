"""The device reductions and the element-wise vector calls against references written here.

SPEC §S11 fixes the order of every dot completely, so it is restated in NumPy (``restated_sum``: the
256-row blocks, at most 1,024 of them, the grid-stride order per thread, the wave shuffle tree, the four
wave sums, the same again over the partials, the parts in rank order) and compared bit for bit. The
restatement itself is held to an exact reference: ``math.fsum`` over the error-free two-products of every
pair (Veltkamp / Dekker), with the bound of a summation tree of depth D plus one product rounding,

    |got - exact| <= (D + 1) 2^-53 sum |RN(x_i y_i)|,   D = ceil(n / (256 np)) + 10 + ceil(np / 256) + 10

(D additions on the longest path: a thread's chain, six shuffle steps and four wave sums per tree, twice).
The bound is derived, not measured. On the CPU the restatement stays under 0.05 of it at every size below;
one dropped entry of the normal data exceeds it 1e8 to 1e13 times (on the cancelling data only an entry of
the larger decades does: the bits catch the others).

``axpby`` is SPEC §S8's ``u = a x; v = b y; y = u + v`` — three roundings, no shortcut for a zero
coefficient — which NumPy's ``a * x + b * y`` computes (NumPy does not fuse)."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from parallel_amg_amd._lib import option
from parallel_amg_amd.hcsr import HCSR
from parallel_amg_amd.partitioned import (DevicePlan, LocalWorld, PSparseMatrix, PVector, axpby, consistent, copy, dot,
                                          estimate_lmax, norm)

pytestmark = pytest.mark.gpu

KBLOCK, KCAP = 256, 1024
WRAP = KBLOCK * KCAP  # the first row a thread reaches on its second trip through the grid-stride loop


def bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def same_fp(got, want):
    from test_gpu_fp_edges import same_fp as f
    return f(np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64)))


# ------------------------------------------------------------------------------ the restatement
def nblocks(n):
    return max(1, min(-(-n // KBLOCK), KCAP))


def keep(a):
    return a


def flushed(a):
    """What a unit that flushes subnormals makes of a: signed zero below 2^-1022."""
    a = np.asarray(a, np.float64)
    return np.where(np.abs(a) < 2.0 ** -1022, np.copysign(0.0, a), a)


def block_tree(v, rn=keep):
    """block_sum of every block: v is (blocks, 256) thread values; the wave64 shuffle-down tree (offsets
    32 .. 1, read at lane 0), then the 4 wave sums added in order from +0.0. ``rn`` is applied to every sum
    (``flushed``: the same order on a unit that flushes subnormals, for tests that must tell the two apart)."""
    w = np.array(v, np.float64).reshape(-1, KBLOCK // 64, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w[:, :, :o] = rn(w[:, :, :o] + w[:, :, o:2 * o])
    s = np.zeros(w.shape[0])
    for k in range(KBLOCK // 64):
        s = rn(s + w[:, k, 0])
    return s


def restated_sum(p, rn=keep):
    """The device's sum of the rounded products p (one part)."""
    p = np.asarray(p, np.float64)
    n, nb = len(p), nblocks(len(p))
    stride = KBLOCK * nb
    with np.errstate(all="ignore"):
        acc = np.zeros(stride)  # thread t of block b is acc[256 b + t]
        for lo in range(0, n, stride):
            m = min(stride, n - lo)
            acc[:m] = rn(acc[:m] + p[lo:lo + m])
        partials = block_tree(acc.reshape(nb, KBLOCK), rn)
        acc = np.zeros(KBLOCK)  # the final pass: thread t adds partials t, t + 256, ...
        for lo in range(0, nb, KBLOCK):
            m = min(KBLOCK, nb - lo)
            acc[:m] = rn(acc[:m] + partials[lo:lo + m])
        return float(block_tree(acc.reshape(1, KBLOCK), rn)[0])


def restated_dot(x, y, rn=keep):
    with np.errstate(all="ignore"):
        return restated_sum(rn(rn(np.asarray(x, np.float64)) * rn(np.asarray(y, np.float64))), rn)


def restated_dot_parts(xs, ys):
    """Several parts: the per-part results added in rank order from +0.0."""
    s = 0.0
    with np.errstate(all="ignore"):
        for x, y in zip(xs, ys):
            s = s + np.float64(restated_dot(x, y))
    return float(s)


def exact_dot(x, y):
    """The dot product rounded once (finite data, no over- or underflow in the split)."""
    p = x * y
    c = 134217729.0  # 2^27 + 1
    t = c * x
    xh = t - (t - x)
    xl = x - xh
    t = c * y
    yh = t - (t - y)
    yl = y - yh
    e = xl * yl - (((p - xh * yh) - xl * yh) - xh * yl)
    return math.fsum(np.concatenate([p, e]))


def bound(x, y):
    n, nb = len(x), nblocks(len(x))
    depth = -(-n // (KBLOCK * nb)) + 10 + -(-nb // KBLOCK) + 10
    return (depth + 1) * 2.0 ** -53 * math.fsum(np.abs(x * y))


# ------------------------------------------------------------------------------ the data
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 100_003, 262_143, 262_144, 262_145, 524_545, 856_433]
# every product of two entries is subnormal or rounds to zero, and 2^20 of the largest (2^-1050) still add up
# to a subnormal: no product, partial sum or result of this set is a normal number
SUBNORMAL_PALETTE = np.array([0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1060, -(2.0 ** -1040), 2.0 ** -525, -(2.0 ** -525),
                              2.0 ** -530, -(2.0 ** -533), 2.0 ** -537, 3.0 * 2.0 ** -528, -5.0 * 2.0 ** -531])
# the same with +-1.0 and squares that are normal: subnormal terms absorbed by, or surviving beside, O(1) ones
MIXED_PALETTE = np.array([0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1060, -(2.0 ** -1040), 2.0 ** -520, -(2.0 ** -520),
                          2.0 ** -530, 2.0 ** -511, 1.0, -1.0, 2.0 ** -1000, 3.0 * 2.0 ** -1074])


def make_data(kind, n):
    rng = np.random.default_rng(1000 + n)
    if kind == "normal":
        return rng.standard_normal(n), rng.standard_normal(n)
    if kind == "cancelling":
        # x_i y_i against -(1 + 2^-40) x_i y_i at a shuffled place, the magnitudes over 12 decades
        h = n // 2
        a = rng.standard_normal(h) * 10.0 ** rng.integers(-6, 7, h)
        c = rng.standard_normal(h) * 10.0 ** rng.integers(-6, 7, h)
        x = np.concatenate([a, -a * (1.0 + 2.0 ** -40), rng.standard_normal(n - 2 * h)])
        y = np.concatenate([c, c, rng.standard_normal(n - 2 * h)])
        perm = rng.permutation(n)
        return np.ascontiguousarray(x[perm]), np.ascontiguousarray(y[perm])
    pal = {"subnormal": SUBNORMAL_PALETTE, "mixed": MIXED_PALETTE}[kind]
    x, y = pal[rng.integers(0, len(pal), n)], pal[rng.integers(0, len(pal), n)]
    if kind == "subnormal" and n:  # (one product that is certainly a non-zero subnormal, also at n = 1)
        x[0], y[0] = 2.0 ** -525, 3.0 * 2.0 ** -528
    return x, y


@pytest.mark.parametrize("kind", ["normal", "cancelling", "subnormal", "mixed"])
@pytest.mark.parametrize("n", SIZES)
def test_dot_and_norm_carry_the_restated_bits(ctx, n, kind):
    """dot(x, y), dot(x, x) on one handle and norm(x): the bits of the restated order; for the normal and
    the cancelling data also within the derived bound of the exactly rounded dot. The subnormal set stays
    below 2^-1022 from the products to the result: the restated dots are non-zero subnormals, and the same
    order on a unit that flushes them gives other bits, so nothing may be flushed anywhere."""
    xh, yh = make_data(kind, n)
    x, y = PVector(ctx, n, 0, xh), PVector(ctx, n, 0, yh)
    got_xy, got_xx, got_nrm = dot(x, y), dot(x, x), norm(x)
    want_xy, want_xx = restated_dot(xh, yh), restated_dot(xh, xh)
    print(f"n={n} {kind}: dot {got_xy!r} restated {want_xy!r}; x.x {got_xx!r} restated {want_xx!r}; norm {got_nrm!r}")
    assert np.array_equal(bits(got_xy), bits(want_xy))
    assert np.array_equal(bits(got_xx), bits(want_xx))
    assert np.array_equal(bits(got_nrm), bits(np.sqrt(np.float64(want_xx))))
    if n == 0:
        assert np.array_equal(bits([got_xy, got_nrm]), bits([0.0, 0.0]))  # +0.0, not -0.0
    if kind == "subnormal" and n:
        tiny = 2.0 ** -1022
        assert 0.0 < abs(want_xy) < tiny and 0.0 < want_xx < tiny
        with np.errstate(all="ignore"):
            assert np.all(np.abs(xh * yh) < tiny) and np.all(xh * xh < tiny)
        for a, b, want in ((xh, yh, want_xy), (xh, xh, want_xx)):
            assert not np.array_equal(bits(restated_dot(a, b, flushed)), bits(want))   # (it is +0.0)
            assert not np.array_equal(bits(restated_sum(a * b, flushed)), bits(want))  # flushed in the sums only
    if kind in ("normal", "cancelling"):
        for a, b, got in ((xh, yh, got_xy), (xh, xh, got_xx)):
            err, bnd = abs(got - exact_dot(a, b)), bound(a, b)
            print(f"   |got - exact| = {err:.3e}, bound {bnd:.3e}")
            assert err <= bnd


@pytest.mark.parametrize("n", [1, 65, 257, 262_145])
def test_dot_of_negative_zero_products_is_positive_zero(ctx, n):
    """Every product is -0.0: each thread starts from +0.0, so the sum is +0.0."""
    x, y = PVector(ctx, n, 0, np.ones(n)), PVector(ctx, n, 0, np.full(n, -0.0))
    assert np.all(np.signbit(np.ones(n) * np.full(n, -0.0)))
    assert np.array_equal(bits(dot(x, y)), bits(0.0))
    assert np.array_equal(bits(dot(y, y)), bits(0.0)) and np.array_equal(bits(norm(y)), bits(0.0))


NF = WRAP + 300


@pytest.mark.parametrize("pos", [0, NF - 1, WRAP], ids=["first", "last", "wrapped"])
def test_dot_non_finite_entries(ctx, pos):
    rng = np.random.default_rng(17)
    xh, yh = rng.standard_normal(NF), rng.standard_normal(NF)
    yh[pos] = abs(yh[pos]) + 1.0
    x, y = PVector(ctx, NF, 0, xh), PVector(ctx, NF, 0, yh)

    def check(want_class):
        got, want = dot(x, y), restated_dot(xh, yh)
        assert want_class(want), want
        assert same_fp(got, want), (got, want)
        assert same_fp(norm(x), np.sqrt(np.float64(restated_dot(xh, xh))))

    xh[pos] = np.nan
    x.set(xh)
    check(np.isnan)
    xh[pos] = np.inf
    x.set(xh)
    check(lambda v: v == np.inf)
    other = (pos + 12_345) % NF  # a second product of -inf elsewhere: inf - inf
    xh[other] = -np.inf
    yh[other] = 2.0
    x.set(xh)
    y.set(yh)
    check(np.isnan)


@pytest.mark.parametrize("n", [300, NF])
def test_dot_overflow(ctx, n):
    """Entries of 1e200: every product overflows, the dot and the norm are +inf (not NaN)."""
    xh = np.full(n, 1e200)
    x = PVector(ctx, n, 0, xh)
    assert same_fp(dot(x, x), np.inf) and same_fp(norm(x), np.inf)
    xh[1::2] = -1e200  # the squares are still +inf
    x.set(xh)
    y = PVector(ctx, n, 0, np.abs(xh))
    assert same_fp(dot(x, x), np.inf)
    assert same_fp(dot(x, y), restated_dot(xh, np.abs(xh))) and np.isnan(restated_dot(xh, np.abs(xh)))


# ------------------------------------------------------------------------------ several parts
@pytest.mark.parametrize("own", [(WRAP + 1 + 300, 1_000), (70_001, 0, WRAP + 77)], ids=["2parts", "3parts"])
def test_dot_over_parts_skips_the_ghost_slots(built, own):
    """Uneven parts (one owns no row, one wraps the grid-stride loop), three NaN ghost slots on every
    vector: the dot is the per-part restated sums added in rank order, the norm its square root, and the
    element-wise calls leave the ghost slots alone."""
    import parallel_amg_amd as pa
    from parallel_amg_amd.hierarchy import build_plans
    nparts = len(own)
    offs = np.concatenate([[0], np.cumsum(own)]).astype(np.int64)
    rng = np.random.default_rng(5)
    xh = [rng.standard_normal(m) for m in own]
    yh = [rng.standard_normal(m) for m in own]
    ghosts = {}
    for p in range(nparts):  # three rows of the other parts, ascending
        others = np.concatenate([np.arange(offs[q], offs[q + 1]) for q in range(nparts) if q != p])
        ghosts[p] = np.sort(rng.choice(others, 3, replace=False)).astype(np.int64)
    hp = build_plans(pa.SequentialBackend(nparts), ghosts, offs)
    with option("poison_ghosts", 1):
        W = LocalWorld(nparts)
        try:
            plans = [DevicePlan(W.ctxs[p], hp[p], tag=1) for p in range(nparts)]
            x = [PVector(W.ctxs[p], own[p], 3) for p in range(nparts)]
            y = [PVector(W.ctxs[p], own[p], 3) for p in range(nparts)]
            for v in x + y:  # the owners' values are NaN at the exchange, so every ghost slot is NaN after it
                v.fill(np.nan)
            W.run(lambda p: (consistent(x[p], plans[p]), consistent(y[p], plans[p])))
            for p in range(nparts):
                x[p].set(xh[p])
                y[p].set(yh[p])
                assert np.all(np.isnan(x[p].ghost_values())) and np.all(np.isnan(y[p].ghost_values()))
            got_xy = W.run(lambda p: dot(x[p], y[p]))
            got_xx = W.run(lambda p: dot(x[p], x[p]))
            got_nrm = W.run(lambda p: norm(x[p]))
            # the element-wise calls touch own entries only
            z = [PVector(W.ctxs[p], own[p], 3) for p in range(nparts)]
            for p in range(nparts):
                copy(z[p], y[p])
                axpby(2.5, x[p], -0.5, y[p])
                x[p].fill(3.5)
            own_after = [(x[p].own_values(), y[p].own_values(), z[p].own_values()) for p in range(nparts)]
            ghost_after = [(x[p].ghost_values(), y[p].ghost_values(), z[p].ghost_values()) for p in range(nparts)]
            del plans, x, y, z
        finally:
            W.close()
    want_xy, want_xx = restated_dot_parts(xh, yh), restated_dot_parts(xh, xh)
    for p in range(nparts):
        assert np.array_equal(bits(got_xy[p]), bits(want_xy)), (p, got_xy[p], want_xy)
        assert np.array_equal(bits(got_xx[p]), bits(want_xx))
        assert np.array_equal(bits(got_nrm[p]), bits(np.sqrt(np.float64(want_xx))))
        xo, yo, zo = own_after[p]
        assert np.array_equal(bits(xo), bits(np.full(own[p], 3.5)))
        assert np.array_equal(bits(yo), bits(2.5 * xh[p] + (-0.5) * yh[p]))
        assert np.array_equal(bits(zo), bits(yh[p]))
        xg, yg, zg = ghost_after[p]
        assert np.all(np.isnan(xg)) and np.all(np.isnan(yg))
        assert np.array_equal(bits(zg), bits(np.zeros(3)))  # never exchanged: as created


# ------------------------------------------------------------------------------ k_lmax_step
def test_lmax_sums_carry_the_restated_bits(ctx):
    """Three steps of the SPEC §S10 iteration on a diagonally dominant tridiagonal operator whose rows wrap
    the grid-stride loop with a ragged tail: num_k and den_k are the restated sums of RN(v_i y_i) and of
    RN(RN(a_ii v_i) v_i), so lambda_k = num_k / den_k bit for bit (the binding returns lambda only), and the
    iterate v^3 is the oracle's."""
    n = WRAP + 1 + 300
    rng = np.random.default_rng(23)
    d = rng.uniform(3.0, 5.0, n)
    e = rng.uniform(-1.2, -0.8, n - 1)  # e[i] couples rows i and i + 1
    cnt = np.full(n, 3, np.int64)
    cnt[0] = cnt[-1] = 2
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    col, val = np.empty(rp[-1], np.int64), np.empty(rp[-1])
    i = np.arange(n)
    dpos = rp[:-1] + (i > 0)
    col[dpos], val[dpos] = i, d
    col[dpos[1:] - 1], val[dpos[1:] - 1] = i[1:] - 1, e
    col[dpos[:-1] + 1], val[dpos[:-1] + 1] = i[:-1] + 1, e
    M = O.CSR(rp, col, val, n)
    A = PSparseMatrix(ctx, HCSR.from_arrays(M.rowptr, M.col.astype(np.int32), M.val, M.ncols))
    v0 = rng.uniform(-1.0, 1.0, n)
    v, y = PVector(ctx, n, 0, v0), PVector(ctx, n)
    lam = estimate_lmax(A, v, y, 3)
    vr, want = v0, []
    for _ in range(3):
        yr = O.spmv(M, vr)
        num = restated_sum(vr * yr)
        den = restated_sum((d * vr) * vr)
        want.append(num / den)
        vr = yr / d
    print("lambda", lam.tolist(), "restated", want)
    assert np.array_equal(bits(lam), bits(want))
    assert np.array_equal(bits(v.own_values()), bits(vr))
    assert np.array_equal(bits(y.own_values()), bits(yr))


# ------------------------------------------------------------------------------ axpby, fill, copy, fill_xstar
CAP_ROWS = 8192 * KBLOCK  # the element-wise kernels' grid cap: above it the grid-stride loop wraps
AXPBY_SIZES = [0, 1, 255, 257, CAP_ROWS, CAP_ROWS + 257]
COEFFS = [(2.5, -0.5), (0.0, 1.0), (1.0, 0.0), (0.0, 0.0), (-1.0, 1.0)]
_axpby_host = {}


def axpby_data(n):
    if n not in _axpby_host:
        rng = np.random.default_rng(n + 7)
        _axpby_host[n] = (rng.standard_normal(n), rng.standard_normal(n))
    return _axpby_host[n]


@pytest.mark.parametrize("n", AXPBY_SIZES)
def test_axpby_bits(ctx, n):
    xh, yh = axpby_data(n)
    x, y = PVector(ctx, n, 2, xh), PVector(ctx, n, 2)
    for a, b in COEFFS:
        y.set(yh)
        axpby(a, x, b, y)
        assert np.array_equal(bits(y.own_values()), bits(a * xh + b * yh)), (a, b)
    assert np.array_equal(bits(x.own_values()), bits(xh))
    assert np.array_equal(bits(y.ghost_values()), bits(np.zeros(2)))


@pytest.mark.parametrize("n", [257, CAP_ROWS + 257])
def test_axpby_non_finite_and_aliased(ctx, n):
    """SPEC §S8 has no shortcut: 0 * inf and 0 * NaN are NaN. +inf, -inf and NaN at the first row, the last
    row and, above the grid cap, the first row of the second trip — once in x with y finite there (a = 0 must
    give NaN), once in y with x finite there (b = 0 must give NaN) — and x and y one handle."""
    x0, y0 = axpby_data(n)
    spots = [0, n - 1] + ([CAP_ROWS] if n > CAP_ROWS else [128])
    x, y = PVector(ctx, n), PVector(ctx, n)
    with np.errstate(invalid="ignore"):
        for where in "xy":
            xh, yh = x0.copy(), y0.copy()
            (xh if where == "x" else yh)[spots] = (np.inf, -np.inf, np.nan)
            x.set(xh)
            for a, b in COEFFS:
                y.set(yh)
                axpby(a, x, b, y)
                got = y.own_values()
                assert same_fp(got, a * xh + b * yh), (where, a, b)
                if (a if where == "x" else b) == 0.0:
                    assert np.all(np.isnan(got[spots])), (where, a, b)   # 0 * (+-inf | NaN)
        xh = x0.copy()
        xh[spots] = (np.inf, -np.inf, np.nan)
        for a, b in COEFFS:  # x and y one handle: RN(a x) + RN(b x)
            x.set(xh)
            axpby(a, x, b, x)
            assert same_fp(x.own_values(), a * xh + b * xh), (a, b)


def test_fill_copy_fill_xstar_above_the_grid_cap(ctx):
    """The three calls on CAP_ROWS + 257 rows (a second, ragged trip through the loop), fill_xstar also from
    a global index above 2^33; the ghost slots keep what they held."""
    n, ng = CAP_ROWS + 257, 3
    v, w = PVector(ctx, n, ng), PVector(ctx, n, ng)
    zeros = np.zeros(ng)
    for val in (-0.0, 2.0 ** -1074, 1.0 / 3.0):
        v.fill(val)
        assert np.array_equal(bits(v.own_values()), bits(np.full(n, val)))
    for i0 in (0, 2 ** 33 + 5):
        v.fill_xstar(i0, O.SEED + 1)
        src = v.own_values()
        assert np.array_equal(bits(src), bits(O.xstar(n, seed=O.SEED + 1, i0=i0)))
        w.fill(7.0)
        copy(w, v)
        assert np.array_equal(bits(w.own_values()), bits(src))
    assert np.array_equal(bits(v.ghost_values()), bits(zeros)) and np.array_equal(bits(w.ghost_values()), bits(zeros))
