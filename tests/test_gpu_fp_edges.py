"""Every row kernel at the edges of the floating-point range: signed zeros, subnormals, values near
the top of the range, non-finite x, operators scaled far from 1. The other GPU tests draw every
vector from ``standard_normal``; these give each layout (asserted through ``layout_of``) vectors that
tell a select-away from a multiply-by-zero, a flushed subnormal from a kept one, -0.0 from +0.0 and
div_rn (csrc/div_rn.h) from the IEEE quotient.

The comparison is ``same_fp``: the NaN masks are equal and everything else — +-0.0 and +-inf
included — has the oracle's bits (the host and the GPU may give a NaN another sign or payload).

The contract for non-finite input (SPEC §S3) and what the row-class kernels k_sym_zm / k_sym_zc do
with it: they multiply an ABSENT IN-GRID entry's +0.0 table value by the real x (kernels.hip, above
zc_rows), so a non-finite x there makes a NaN the oracle does not have; a neighbour OUTSIDE the grid
(across a face — the x-wrap neighbour ``i - 1`` of a line's first row among them) is held as +0.0 and
never read. The SPEC grids have no absent in-grid entry, so on them the kernels give the oracle's
bits for any x (``test_nonfinite_x_wrap``); the cut grid has such entries, and there the exception
rows are computed on the host and required to be non-finite (``test_nonfinite_x_absent_in_grid``)."""
import contextlib
import ctypes
from dataclasses import dataclass, field

import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd._lib import PamgError, call, layout_of
from parallel_amg_amd.hcsr import HCSR
from parallel_amg_amd.partitioned import PSparseMatrix, PVector, chebyshev, jacobi, jacobi_residual, mul, residual
from parallel_amg_amd.solver import AMGSolver

from test_gpu_chebyshev import CycleRef, cheb_ref, coeffs_ref, diag_of, options, two_blocks
from test_gpu_ell_window import banded, palette_grid, upload_pair
from test_gpu_parity import LENGTHS, OPT_KEYS, PALETTES, TILE_CONFIGS, _cut_grid, _ell_cases, random_csr

pytestmark = pytest.mark.gpu

OMEGA = 0.57
LMAX, RATIO, DEG = 2.3, 4.0, 3


# ------------------------------------------------------------------------------ the comparison
def same_fp(got, want):
    """Equal NaN masks, equal bits everywhere else."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(got.shape == want.shape and np.array_equal(gn, wn)
                and np.array_equal(got.view(np.int64)[~gn], want.view(np.int64)[~wn]))


def differing(got, want):
    """The rows same_fp objects to."""
    gn, wn = np.isnan(got), np.isnan(want)
    return np.flatnonzero((gn != wn) | (~(gn | wn) & (got.view(np.int64) != want.view(np.int64))))


def assert_same(tag, got, want, rows=None):
    g, w = (got, want) if rows is None else (got[rows], want[rows])
    if not same_fp(g, w):
        d = differing(g, w)
        d = d if rows is None else np.asarray(rows)[d]
        raise AssertionError(f"{tag}: {len(d)} of {len(want)} rows differ; first rows {d[:6].tolist()}, "
                             f"device {[float(v).hex() for v in got[d[:6]]]}, "
                             f"oracle {[float(v).hex() for v in want[d[:6]]]}")


# ------------------------------------------------------------------------------ the layout cases
@dataclass
class Case:
    key: str                 # names the host matrix (cases that share it share the oracle's results)
    M: O.CSR
    D: object                # the device matrix
    run: dict = field(default_factory=dict)  # options in force while the operations run
    fused: bool = False      # jacobi_residual must take the fused pass (k_sym_zc / k_sym_tb)
    rowclass: bool = False   # k_sym_zm / k_sym_zc: maskless sums (the non-finite exception)
    shape: tuple = None      # the grid, where there is one
    prolong: bool = True     # has a prolongate-add kernel (the symmetric layouts are never built for a P)
    keep: tuple = ()         # device objects that must outlive D (the grid a prolongation is coded against)

    @property
    def square(self):        # square with a full diagonal: Jacobi and Chebyshev are defined
        return self.M.nrows == self.M.ncols and bool(np.all(diag_of(self.M) != 0.0))


def shown(lay):
    """The fields of a layout_of result that are set."""
    return str({k: v for k, v in lay.items() if v and k != "ell_xwin_census"})


def upload(ctx, M):
    return PSparseMatrix(ctx, HCSR.from_arrays(M.rowptr, M.col.astype(np.int32), M.val, M.ncols))


_host = {}


def host(key, build):
    if key not in _host:
        _host[key] = build()
    return _host[key]


SYM_GRIDS = {"poisson3d_64x32x40": ("poisson3d", (64, 32, 40)), "aniso3d_192x48x7": ("aniso3d", (192, 48, 7))}


def case_sym(ctx, grid, zch, vd, scale=1.0):
    """k_sym_zm for the one-sweep operations and k_sym_zc through jacobi_residual (sym_vd 1); the
    masked k_rows_sym2 and k_sym_tb on the same operator (sym_vd 0)."""
    kind, shape = SYM_GRIDS[grid]
    M = scaled(host(grid, lambda: O.generate(kind, *shape)), scale)
    with options(sym_vd=vd):
        D = upload(ctx, M)
    lay = layout_of(D)
    assert lay["sym"] and lay["sym_vd"] == bool(vd) and lay["jr_fused"], shown(lay)
    return Case(grid, M, D, dict(sym_zm=1, zm_chunks=zch, jr_fuse=1), fused=True, rowclass=bool(vd), shape=shape,
                prolong=False), lay


def case_sym_older(ctx, vd, rows, scale=1.0):
    """k_rows_symd (1, 2), k_rows_sym (0, 1), k_rows_sym2 (0, 2)."""
    kind, shape = SYM_GRIDS["poisson3d_64x32x40"]
    M = scaled(host("poisson3d_64x32x40", lambda: O.generate(kind, *shape)), scale)
    run = dict(sym_zm=0, sym_vd=vd, sym_rows=rows)
    with options(**run):
        D = upload(ctx, M)
    lay = layout_of(D)
    assert lay["sym"] and lay["sym_vd"] == bool(vd) and lay["sym_rows"] == rows, shown(lay)
    return Case("poisson3d_64x32x40", M, D, run, shape=shape, prolong=False), lay


def case_ell(ctx, kind, pair, scale=1.0):
    """k_rows_ell: paired index bytes or separate offset / value tables."""
    M = scaled(host("ell_" + kind, lambda: _ell_cases(kind)), scale)
    with options(ell_min_rows=0, sym_dia=0, ell_pair=pair, ell_xwin=0):
        D = upload(ctx, M)
    lay = layout_of(D)
    assert lay["ell"] and not lay["ell_xwin"] and lay["ell_xwin_groups"] == 0 and not lay["sym"], shown(lay)
    if kind != "ragged":  # (the ragged rows' groups hold more than 256 pairs: separate tables)
        assert lay["ell_pair"] == bool(pair), shown(lay)
    return Case("ell_" + kind, M, D), lay


# (ragged() is not among them: its groups hold more than 256 (offset, value) pairs, so the upload declines
# the windowed layout for it — test_gpu_ell_window.test_ragged_rows — and it stays with k_rows_ell above)
ELLW = {"palette128x7x5": lambda: palette_grid(128, 7, 5), "banded999": lambda: banded(999), "two_blocks": two_blocks}


def case_ellw(ctx, name, twin, scale=1.0):
    """k_rows_ellw, and the same matrix with ell_xwin 0 (k_rows_ell) beside it."""
    M = scaled(host("ellw_" + name, ELLW[name]), scale)
    A, B, _h = upload_pair(ctx, M, **(dict(ell_xwin_max=1024) if name == "two_blocks" else {}))
    lay = layout_of(A)
    assert lay["ell"] and lay["ell_xwin"] and lay["ell_xwin_groups"] > 0, shown(lay)
    if name == "palette128x7x5":   # regrouped, short last group
        assert lay["ell_gather_groups"] == 0 and lay["ell_xwin_noncontig_groups"] >= 1 and lay["tiles"] >= 18, shown(lay)
    if name == "banded999":        # clipped windows, unaligned x
        assert lay["ell_gather_groups"] == 0 and lay["ell_xwin_groups"] >= 4, shown(lay)
    if name == "two_blocks":       # windowed and gathering groups in one launch
        assert lay["ell_gather_groups"] > 0 and lay["ell_xwin_max_window"] <= 1024, shown(lay)
    if twin:
        lay = layout_of(B)         # (upload_pair asserted: ell, no window)
    return Case("ellw_" + name, M, B if twin else A), lay


def _transfer_operators():
    """Level 0 of the host-built SA hierarchy of the 128 x 32 x 20 Poisson grid: A, P, R."""
    Mg = O.generate("poisson3d", 128, 32, 20)
    n = Mg.nrows
    A = {0: HCSR.from_arrays(Mg.rowptr, Mg.col.astype(np.int32), Mg.val, n)}
    H = pa.build_hierarchy(pa.SequentialBackend(1), A, np.array([0, n], np.int64), pa.SAParams(max_coarse=100))
    lp = H.levels[0][0]
    as_csr = lambda T: O.CSR(T.rowptr.copy(), T.col.astype(np.int64), T.val.copy(), T.ncols)  # noqa: E731
    return lp.A, as_csr(lp.P), as_csr(lp.R)


def case_transfer(ctx, which):
    """k_rows_rpat (the restriction) and k_rows_pnc with compact and 64-bit records (the prolongation,
    uploaded after its grid operator)."""
    A0, P, R = host("transfer", _transfer_operators)
    Ad = PSparseMatrix(ctx, A0)
    assert layout_of(Ad)["jr_fused"], layout_of(Ad)
    if which == "rpat":
        D = upload(ctx, R)
        lay = layout_of(D)
        assert lay["rpat"] and not lay["ell"] and not lay["pnc"], shown(lay)
        return Case("transfer_R", R, D, keep=(Ad,)), lay
    with options(pnc_compact=int(which == "pnc_compact")):
        D = upload(ctx, P)
    lay = layout_of(D)
    assert lay["pnc"] and lay["pnc_compact"] == (which == "pnc_compact") and not lay["rpat"], shown(lay)
    return Case("transfer_P", P, D, keep=(Ad,)), lay


def _tile_matrix(name):
    lengths = LENGTHS[name]
    ncols = max(max(lengths) + 1, len(lengths) + 7)
    return random_csr(np.random.default_rng(11), lengths, ncols, palette=PALETTES["few"])


def case_tiles(ctx, name, cfg):
    """k_rows_tile2 with 32-bit columns (0) and with 24-bit columns (5: the value dictionaries it asks for
    are built for tall operators only, case_tall), the default (9) and tile-major on every eligible set
    (14); rows longer than a tile go to k_rows_long in each."""
    M = host("tiles_" + name, lambda: _tile_matrix(name))
    run = dict(zip(OPT_KEYS, TILE_CONFIGS[cfg]))
    with options(**run):
        D = upload(ctx, M)
    lay = layout_of(D)
    assert not (lay["sym"] or lay["ell"] or lay["rpat"] or lay["pnc"]) and lay["tiles"] > 0, shown(lay)
    assert lay["tile_nnz"] == TILE_CONFIGS[cfg][0], shown(lay)
    if cfg == 0:
        assert not (lay["c24"] or lay["vd"] or lay["rl8"] or lay["cd"] or lay["tm"]), shown(lay)
    if cfg == 5:
        assert lay["c24"] and not (lay["vd"] or lay["rl8"] or lay["cd"] or lay["tm"]), shown(lay)
    if cfg in (9, 14):
        assert lay["c24"] and lay["rl8"] == (name == "len8_edge"), shown(lay)
    if cfg == 14 and name == "len8_edge":  # (ragged: rows of 2049 keep the set out of the tile-major slots)
        assert lay["tm"], shown(lay)
    return Case("tiles_" + name, M, D, run), lay


TALL = {"len255": [255, 2, 1], "short": [3, 4, 1, 5, 0, 9, 2]}


def case_tall(ctx, name):
    """k_rows_tile2 with 4-bit per-tile value dictionaries: built for tall operators (a prolongation's
    shape) only — 6000 rows over 900 columns, the palette's six values (+0.0 and -0.0 among them), a
    255-nonzero row, empty rows; 8-bit row lengths where the rows are short."""
    lengths = (TALL[name] * 6000)[:6000]
    M = host("tall_" + name, lambda: random_csr(np.random.default_rng(13), lengths, 900, palette=PALETTES["few"]))
    with options(row_len8=1, value_dict=1, col24=1):
        D = upload(ctx, M)
    lay = layout_of(D)
    assert lay["vd"] and lay["c24"] and not lay["tm"] and lay["rl8"] == (name == "short"), shown(lay)
    return Case("tall_" + name, M, D), lay


def case_long(ctx):
    """k_rows_long: rows of 5000 and 9000 nonzeros, more than any tile holds (the upload gives such a
    row a workgroup of its own, matrix.hip build_tiles), beside rows of 2047 .. 2049, 1 and 0."""
    lengths = LENGTHS["long"]
    M = host("long", lambda: random_csr(np.random.default_rng(11), lengths, max(lengths) + 1))
    D = upload(ctx, M)
    lay = layout_of(D)
    assert not (lay["sym"] or lay["ell"] or lay["rpat"] or lay["pnc"]), shown(lay)
    assert max(lengths) > 4096 >= lay["tile_nnz"], shown(lay)
    return Case("long", M, D), lay


def scaled(M, c):
    """M with every value times the power of two c (exact: no value of these matrices leaves the
    normal range)."""
    if c == 1.0:
        return M
    v = M.val * c
    assert np.array_equal(v / c, M.val)
    return O.CSR(M.rowptr, M.col, v, M.ncols)


# name -> (builder, Jacobi and Chebyshev defined). The names are the test ids.
CASES = {}
for _g in SYM_GRIDS:
    for _zch in (0, 3):
        for _vd in (1, 0):
            CASES[f"sym_{_g}_zch{_zch}_vd{_vd}"] = (lambda ctx, s=1.0, g=_g, z=_zch, v=_vd: case_sym(ctx, g, z, v, s), True)
for _vd, _rows in ((1, 2), (0, 1), (0, 2)):
    CASES[f"sym_older_vd{_vd}_rows{_rows}"] = (lambda ctx, s=1.0, v=_vd, r=_rows: case_sym_older(ctx, v, r, s), True)
for _kind in ("grid3d", "ragged"):
    for _pair in (1, 0):
        CASES[f"ell_{_kind}_pair{_pair}"] = (lambda ctx, s=1.0, k=_kind, p=_pair: case_ell(ctx, k, p, s), _kind != "ragged")
for _name in ELLW:
    for _twin in (0, 1):
        CASES[f"ellw_{_name}" + ("_xwin0" if _twin else "")] = (
            lambda ctx, s=1.0, n=_name, t=_twin: case_ellw(ctx, n, t, s), True)
for _which in ("rpat", "pnc_compact", "pnc_records"):
    CASES[_which] = (lambda ctx, w=_which: case_transfer(ctx, w), False)
for _name in ("ragged", "len8_edge"):
    for _cfg in (0, 5, 9, 14):
        CASES[f"tiles_{_name}_cfg{_cfg}"] = (lambda ctx, n=_name, c=_cfg: case_tiles(ctx, n, c), False)
for _name in TALL:
    CASES[f"tall_{_name}"] = (lambda ctx, n=_name: case_tall(ctx, n), False)
CASES["long"] = (lambda ctx: case_long(ctx), False)
SQUARE = [n for n, (_b, sq) in CASES.items() if sq]
ROWCLASS = [n for n in CASES if n.startswith("sym_") and n.endswith("_vd1") and "older" not in n]

_built = {}


def get_case(ctx, name, scale=1.0):
    """The case, uploaded once per session; its layout is printed the first time (run with -s to see
    which fields each case had)."""
    if (name, scale) not in _built:
        c, lay = CASES[name][0](ctx) if scale == 1.0 else CASES[name][0](ctx, scale)
        assert c.square == CASES[name][1], name
        print(f"\n  layout {name}" + (f" x {scale.hex()}" if scale != 1.0 else "") + f": {shown(lay)}", end="")
        _built[(name, scale)] = c
    return _built[(name, scale)]


# ------------------------------------------------------------------------------ the operations
def oracle_ops(M, xh, bh, square, single_step=False):
    """What the runner compares with: SPEC §S3 through the oracle, §S9 through its restatement."""
    with np.errstate(all="ignore"):
        s = O.spmv(M, xh)
        w = {"spmv": s, "residual": O.residual(M, xh, bh), "prolongate_add": (bh + s) + s}
        if square:
            w["jacobi1"] = O.jacobi(M, xh, bh, OMEGA)
            if not single_step:
                w["jr_r"] = O.residual(M, w["jacobi1"], bh)
                w["jacobi2"] = O.jacobi(M, w["jacobi1"], bh, OMEGA)
                c1, c2 = coeffs_ref(LMAX, RATIO, DEG)
                w["chebyshev"] = cheb_ref(M, diag_of(M), xh, bh, c1, c2, DEG)
    return w


def device_ops(ctx, c, xh, bh, single_step=False):
    """SpMV, residual, prolongate-add (refused by the symmetric layouts, which have no such kernel); on
    square operators one and two Jacobi sweeps, the fused Jacobi + residual where the layout has it, and
    one Chebyshev polynomial of degree 3."""
    M, D = c.M, c.D
    nr, nc = M.nrows, M.ncols
    got = {}
    with options(**c.run):
        x, b, y = PVector(ctx, nc, 0, xh), PVector(ctx, nr, 0, bh), PVector(ctx, nr)
        mul(y, D, x)
        got["spmv"] = y.own_values()
        residual(y, D, x, b)
        got["residual"] = y.own_values()
        ms, yy = ctypes.c_double(), PVector(ctx, nr, 0, bh)  # y <- y + A x from y = b, twice (warm-up + 1 timed)
        if c.prolong:
            call("pamg_bench_rowop", ctx.handle, D.handle, 3, x.handle, None, yy.handle, 0.0, 1, ctypes.byref(ms))
            got["prolongate_add"] = yy.own_values()
        else:  # refused, not skipped over: y must not come back unchanged as if the operation had run
            with pytest.raises(PamgError) as e:
                call("pamg_bench_rowop", ctx.handle, D.handle, 3, x.handle, None, yy.handle, 0.0, 1, ctypes.byref(ms))
            assert e.value.code == -6, e.value  # PAMG_E_STATE
        if c.square:
            t = PVector(ctx, nr)
            jacobi(x, D, b, t, OMEGA, 1)
            got["jacobi1"] = x.own_values()
            if c.fused:
                x, r = PVector(ctx, nc, 0, xh), PVector(ctx, nr)
                assert jacobi_residual(t, r, D, x, b, OMEGA), "jacobi_residual did not take the fused pass"
                got["jr_t"] = t.own_values()
                if not single_step:
                    got["jr_r"] = r.own_values()
            if not single_step:
                x = PVector(ctx, nc, 0, xh)
                jacobi(x, D, b, t, OMEGA, 2)
                got["jacobi2"] = x.own_values()
                x, t1, t2 = D.new_input_vector(), D.new_input_vector(), D.new_input_vector()
                x.set(xh)
                chebyshev(x, D, b, t1, t2, lmax=LMAX, ratio=RATIO, degree=DEG)
                got["chebyshev"] = x.own_values()
        assert np.array_equal(b.own_values().view(np.int64), bh.view(np.int64))
    return got


_want = {}


def wanted(c, cls, xh, bh, single_step=False):
    k = (c.key, cls, single_step)
    if k not in _want:
        _want[k] = oracle_ops(c.M, xh, bh, c.square, single_step)
    return _want[k]


def run_ops(ctx, name, c, cls, xh, bh, single_step=False):
    want = wanted(c, cls, xh, bh, single_step)
    got = device_ops(ctx, c, xh, bh, single_step)
    for op, g in got.items():
        assert_same(f"{name} {cls} {op}", g, want["jacobi1" if op == "jr_t" else op])
    return got, want


# ------------------------------------------------------------------------------ the vectors
EDGES = np.array([s * v for v in (0.0, 5e-324, 1e-310, 2.0 ** -1022 - 2.0 ** -1074, 2.0 ** -1022, 2.0 ** -1000,
                                  2.0 ** 500) for s in (1.0, -1.0)])


def normals(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def edge_vector(n, seed, is_b):
    """Standard normals; a fixed 30 % of the positions from EDGES; on the fifth [2n/5, 3n/5) x is
    +0.0, -0.0 alternating and b is -0.0."""
    rng = np.random.default_rng(seed + 100)
    v = normals(n, seed)
    at = rng.choice(n, (3 * n) // 10, replace=False)
    v[at] = rng.choice(EDGES, len(at))
    lo, hi = (2 * n) // 5, (3 * n) // 5
    v[lo:hi] = -0.0 if is_b else np.where(np.arange(lo, hi) % 2 == 0, 0.0, -0.0)
    return v


def is_subnormal(v):
    return (v != 0.0) & (np.abs(v) < 2.0 ** -1022)


def is_negzero(v):
    return (v == 0.0) & np.signbit(v)


# the band-structured cases: rows inside the zero fifth read zeros only, so b - s is -0.0 - (+0.0)
BANDED = [n for n in CASES if n.startswith(("sym_", "ell_grid3d", "ellw_palette", "ellw_banded"))]


@pytest.mark.parametrize("name", list(CASES))
def test_finite_edges(ctx, name):
    """Class 1. The three conditions are computed from the oracle alone, before the device runs."""
    c = get_case(ctx, name)
    xh, bh = edge_vector(c.M.ncols, 1, False), edge_vector(c.M.nrows, 2, True)
    want = wanted(c, "finite_edges", xh, bh)
    for op, w in want.items():
        assert np.all(np.isfinite(w)), (name, op)
    # (a subnormal row sum: a row with a single stored entry, or whose other entries meet the zero fifth
    # or a zero value, times a subnormal x. "long" cannot meet it: 7 rows, the short ones of 1 and 0
    # entries, and a row of thousands of entries never sums to a subnormal)
    if name != "long":
        assert np.any(is_subnormal(want["spmv"])), name
    if name in BANDED:
        assert np.any(is_negzero(want["residual"])) and np.any(is_negzero(want["jacobi1"])), name
        # (a second sweep keeps a -0.0 only where the fifth is more than two neighbour distances wide:
        # not on 128 x 7 x 5, whose fifth is one plane, nor on banded(999), 200 rows against offsets +-70)
        if not name.startswith(("ellw_palette", "ellw_banded")):
            assert np.any(is_negzero(want["jacobi2"])), name
    run_ops(ctx, name, c, "finite_edges", xh, bh)


@pytest.mark.parametrize("name", list(CASES))
def test_tiny(ctx, name):
    """Class 2: class 1's normals times 2^-1040 — products and sums live among the subnormals."""
    c = get_case(ctx, name)
    xh, bh = normals(c.M.ncols, 1) * 2.0 ** -1040, normals(c.M.nrows, 2) * 2.0 ** -1040
    _got, want = run_ops(ctx, name, c, "tiny", xh, bh)
    assert np.any(is_subnormal(want["residual"])), name


QUOTIENT_SCALES = [2.0 ** -900, 2.0 ** -450, 2.0 ** 199, 2.0 ** 450]  # (2^199: the Poisson diagonal is 3 2^200)


@pytest.mark.parametrize("scale", QUOTIENT_SCALES, ids=lambda s: s.hex())
@pytest.mark.parametrize("name", SQUARE)
def test_quotient_range(ctx, name, scale):
    """Class 3: x = 0 and omega = 1 make every row of a Jacobi sweep the quotient b_i / d_i alone; b_i =
    m 2^e with e uniform in [-1000, 1000] and the operator scaled by 2^-900 .. 2^450 put the quotients
    on both sides of div_rn's guard, above the largest double and below the smallest normal one. Rows
    5 and 7 hold the two operands the [2^-900, 2^900] guard got wrong (2^900 overflows against d =
    6 2^-900; 9 2^-875 / (3 2^200) is a subnormal tie). On the layouts that divide with `/` this is the
    control. Then one Chebyshev polynomial of degree 2 from x = 0 (step 0 and one three-term step)."""
    c = get_case(ctx, name, scale)
    M, n = c.M, c.M.nrows
    rng = np.random.default_rng(33)
    bh = np.ldexp(1.0 + rng.random(n), rng.integers(-1000, 1001, n)) * rng.choice([1.0, -1.0], n)
    bh[5] = 2.0 ** 900
    bh[7] = 9 * 2.0 ** -875
    xh = np.zeros(n)
    d = diag_of(M)
    with np.errstate(all="ignore"):
        q = bh / d
        want_j = O.jacobi(M, xh, bh, 1.0)
        assert same_fp(want_j, 0.0 + q)  # (the oracle's sweep is this quotient)
        c1, c2 = coeffs_ref(LMAX, RATIO, 2)
        want_c = cheb_ref(M, d, xh, bh, c1, c2, 2)
        want_r = O.residual(M, want_j, bh)
    if scale == 2.0 ** -900:
        assert np.isinf(want_j[5]) and np.count_nonzero(np.isinf(want_j)) > n // 50
    if scale == 2.0 ** 199 and d[7] == 3 * 2.0 ** 200:
        assert want_j[7] == 2.0 ** -1073
    assert np.count_nonzero(is_subnormal(want_j)) + np.count_nonzero(np.isinf(want_j)) > 0
    with options(**c.run):
        x, b, t = PVector(ctx, n, 0, xh), PVector(ctx, n, 0, bh), PVector(ctx, n)
        jacobi(x, c.D, b, t, 1.0, 1)
        assert_same(f"{name} quotient jacobi", x.own_values(), want_j)
        if c.fused:
            x, r = PVector(ctx, n, 0, xh), PVector(ctx, n)
            assert jacobi_residual(t, r, c.D, x, b, 1.0)
            assert_same(f"{name} quotient jacobi_residual t", t.own_values(), want_j)
            assert_same(f"{name} quotient jacobi_residual r", r.own_values(), want_r)
        x, t1, t2 = c.D.new_input_vector(), c.D.new_input_vector(), c.D.new_input_vector()
        x.set(xh)
        chebyshev(x, c.D, b, t1, t2, lmax=LMAX, ratio=RATIO, degree=2)
        assert_same(f"{name} quotient chebyshev", x.own_values(), want_c)
    _built.pop((name, scale))  # (one use: the scaled upload is not kept)


NONFINITE = np.array([np.inf, -np.inf, np.nan] * 4)


def with_nonfinite(xh, at):
    assert len(set(at)) == len(NONFINITE) and min(at) >= 0 and max(at) < len(xh), at
    xh = xh.copy()
    xh[np.asarray(at)] = NONFINITE
    return xh


@pytest.mark.parametrize("name", list(CASES))
def test_nonfinite_x(ctx, name):
    """Class 4 (a), (b): +inf, -inf and NaN in x, four of each. A padded slot's product — with the
    row's own or first x, which may now be NaN — must be selected away, never added as 0 * x.
    (a) Every layout but k_sym_zm / k_sym_zc: positions that include index 0, the last index and
    positions inside the last slice / tile. (b) k_sym_zm / k_sym_zc: positions at least 2 from every
    face of the grid (every row that reads one has it as a stored entry). The oracle's bits, in full."""
    c = get_case(ctx, name)
    n = c.M.ncols
    if name in ROWCLASS:
        nx, ny, nz = c.shape
        at = [((2 + (5 * t) % (nz - 4)) * ny + 2 + (11 * t) % (ny - 4)) * nx + 2 + (37 * t) % (nx - 4) for t in range(12)]
        cls = "nonfinite_inside"
    else:
        at = [0, 1, 2, n - 1, n - 2, n - 3, n - 35, n - 70, n // 2, n // 2 + 1, n // 3, n // 7]
        cls = "nonfinite_ends"
    xh, bh = with_nonfinite(edge_vector(n, 1, False), at), edge_vector(c.M.nrows, 2, True)
    _got, want = run_ops(ctx, name, c, cls, xh, bh)
    assert np.count_nonzero(~np.isfinite(want["spmv"])) >= 1, name


def exception_rows(M, shape, xh, in_grid):
    """Rows i with a non-finite x_j at j in {i +- 1, i +- nx, i +- nx ny} within [0, N) that is not a
    stored column of row i; in_grid: only where j is i's neighbour IN the grid (not across a face)."""
    nx, ny, _nz = shape
    E = set()
    for j in np.flatnonzero(~np.isfinite(xh)):
        for o in (1, -1, nx, -nx, nx * ny, -nx * ny):
            i = int(j) - o
            if not 0 <= i < M.nrows or j in M.col[M.rowptr[i]:M.rowptr[i + 1]]:
                continue
            same_line, same_plane = i // nx == j // nx, i // (nx * ny) == j // (nx * ny)
            if in_grid and not (same_line if abs(o) == 1 else same_plane if abs(o) == nx else True):
                continue
            E.add(i)
    return np.array(sorted(E), np.int64)


def run_with_exceptions(ctx, name, c, cls, xh, bh, E):
    """One-step operations (each output row reads x once, so E is the whole exception): the oracle's
    bits outside E, a non-finite value on E."""
    want = wanted(c, cls, xh, bh, single_step=True)
    got = device_ops(ctx, c, xh, bh, single_step=True)
    rest = np.setdiff1d(np.arange(c.M.nrows), E)
    for op, g in got.items():
        w = want["jacobi1" if op == "jr_t" else op]
        assert_same(f"{name} {cls} {op}", g, w, rest)
        finite_in_E = E[np.isfinite(g[E])]
        assert finite_in_E.size == 0, (name, op, "finite values on exception rows", finite_in_E[:6],
                                       g[finite_in_E[:6]], w[finite_in_E[:6]])


@pytest.mark.parametrize("name", ROWCLASS)
def test_nonfinite_x_wrap(ctx, name):
    """Class 4 (c), at the x wrap: non-finite x at ix = 0, whose index neighbour j - 1 is the last row
    of the line before — not a neighbour in the grid. By index arithmetic alone, E = {rows with such a
    j among i +- 1, i +- nx, i +- nx ny that is not a stored column} has one row per placed value
    (0 < |E| <= 6 x 12). k_sym_zm / k_sym_zc hold every neighbour across a face as +0.0 and never read
    it, so none of those rows is an exception: the rows with an absent IN-GRID neighbour are the
    exception set, it is empty on the SPEC grids, and the oracle's bits are required on every row — the
    rows of E, whose oracle values are finite, among them."""
    c = get_case(ctx, name)
    nx, ny, nz = c.shape
    n = c.M.nrows
    at = [((1 + (5 * t) % (nz - 1)) * ny + (11 * t) % ny) * nx for t in range(12)]
    xh, bh = with_nonfinite(edge_vector(n, 1, False), at), edge_vector(n, 2, True)
    E_index = exception_rows(c.M, c.shape, xh, in_grid=False)
    assert 0 < E_index.size <= 6 * len(at), E_index
    E = exception_rows(c.M, c.shape, xh, in_grid=True)
    assert E.size == 0, E
    got, want = run_ops(ctx, name, c, "nonfinite_wrap", xh, bh)
    assert np.all(np.isfinite(want["spmv"][E_index])) and np.all(np.isfinite(got["spmv"][E_index]))


@pytest.mark.parametrize("zch", [0, 3])
def test_nonfinite_x_absent_in_grid(ctx, zch):
    """Class 4 (c), where the exception is real: the 64^3 grid with the couplings between x = 31 and
    x = 32 removed has absent in-grid entries, held as +0.0 table values and multiplied by the real x
    (k_sym_zm, k_sym_zc). Non-finite x on both sides of the cut: E is computed on the host (one row per
    placed value, the neighbour across the cut); outside E the oracle's bits, on E a non-finite value —
    never a finite one the oracle does not have."""
    M = host("cut_grid", _cut_grid)
    name = f"sym_cut64_zch{zch}"
    if (name, 1.0) not in _built:
        D = upload(ctx, M)
        lay = layout_of(D)
        assert lay["sym"] and lay["sym_vd"] and lay["jr_fused"], shown(lay)
        print(f"\n  layout {name}: {shown(lay)}", end="")
        _built[(name, 1.0)] = Case("cut_grid", M, D, dict(sym_zm=1, zm_chunks=zch, jr_fuse=1), fused=True,
                                   rowclass=True, shape=(64, 64, 64), prolong=False)
    c = _built[(name, 1.0)]
    n = M.nrows
    at = [((2 + 5 * t) * 64 + 3 + 4 * t) * 64 + (31 if t % 2 else 32) for t in range(12)]
    xh, bh = with_nonfinite(edge_vector(n, 1, False), at), edge_vector(n, 2, True)
    E = exception_rows(M, c.shape, xh, in_grid=True)
    assert np.array_equal(E, np.sort([j + 1 if j % 64 == 31 else j - 1 for j in at])), E
    assert 0 < E.size <= 6 * len(at)
    want = wanted(c, "nonfinite_cut", xh, bh, single_step=True)
    assert np.all(np.isfinite(want["spmv"][E]))  # (the oracle sums stored entries only)
    run_with_exceptions(ctx, name, c, "nonfinite_cut", xh, bh, E)


# ------------------------------------------------------------------------------ class 5: scaled cycles
def _scaled_problem(ctx, n, k):
    kind, mc = "poisson3d", (1000 if n == 64 else 100)
    be = pa.SequentialBackend(1)
    Ah, offs, xs = pa.generate_problem(be, kind, n)
    c = 2.0 ** k
    for p in Ah:
        Ah[p].val[:] = Ah[p].val * c
    H = pa.build_hierarchy(be, Ah, offs, pa.SAParams(max_coarse=mc), device=ctx)
    with options(ell_min_rows=0) if n == 32 else contextlib.nullcontext():
        S = AMGSolver(ctx, H)
    if n == 64:
        l0 = layout_of(S.A_dev[0])
        assert l0["sym"] and l0["sym_vd"] and l0["jr_fused"], l0
    else:
        l1 = layout_of(S.A_dev[1])
        assert l1["ell"] and l1["ell_xwin"] and l1["ell_xwin_groups"] > 0, l1
    b = PVector(ctx, S.A[0].nrows)
    mul(b, S.A[0], PVector(ctx, S.A[0].nrows, 0, xs[0]))
    Ao = scaled(O.generate(kind, n, n, n), c)
    bo = O.spmv(Ao, O.xstar(Ao.nrows))
    assert same_fp(b.own_values(), bo)
    Ho = O.setup(Ao, max_coarse=mc)
    assert Ho.nlevels == H.nlevels
    assert [H.levels[l][0].rho for l in range(H.nlevels)] == list(Ho.rho)
    return S, b, bo, Ho


@pytest.mark.parametrize("k", [-300, 0, 300])
@pytest.mark.parametrize("n", [64, 32])
def test_scaled_cycle(ctx, n, k):
    """Class 5: poisson3d with every matrix value times 2^k — setup on the device, b = A x*, 3 V-cycles
    from the graph and eagerly, with Jacobi (against the oracle's setup and solve of the same scaled
    matrix) and with the Chebyshev smoother, V(2,2) (against the §S9 restatement over the oracle's hierarchy):
    x by bits, the residual history to 1e-12. n = 64: level 0 in the fused row-class kernels; n = 32:
    level 1 in the windowed ELL. (Nothing is asserted about x across k.)"""
    S, b, bo, Ho = _scaled_problem(ctx, n, k)
    xo, ho = Ho.solve(bo, 3, res_hist=True)
    xc, hc = CycleRef(Ho).solve(bo, 3, 2, 2)
    assert np.all(np.isfinite(xo)) and np.all(np.isfinite(xc))
    try:
        for smoother, xw, hw in (("jacobi", xo, ho), ("chebyshev", xc, hc)):
            S.set_smoother(smoother, **(dict(ratio=4.0) if smoother == "chebyshev" else {}))
            S.set_sweeps(*((2, 2) if smoother == "chebyshev" else (1, 1)))
            for graph in (True, False):
                S.set_graph(graph)
                x = S.new_vector()
                hist = S.vcycle(x, b, 3, res_hist=True)
                assert_same(f"poisson3d {n} x 2^{k} {smoother} graph={graph}", x.own_values(), xw)
                np.testing.assert_allclose(hist, hw, rtol=1e-12)
                assert S.graph_state()["captured"] == graph and not S.graph_state()["failed"]
    finally:
        S.set_graph(True)
        S.set_smoother("jacobi")
        S.set_sweeps(1, 1)
