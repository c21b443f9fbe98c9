"""Group pairs of the windowed sliced ELL (ell_xwin 1, the default; k_rows_ellw's SPAN 2): two windowed
groups whose windows overlap run in one workgroup of 8 waves on one union window. Every case uploads
the operator with ell_xwin 1, with ell_xwin 3 (the same without pairs) and with ell_xwin 0 (k_rows_ell),
asserts through the census which groups were paired, and compares SpMV, residual, prolongate-add,
Jacobi sweeps and the Chebyshev smoother of all three with the oracle, bit for bit (so with each other).

Not covered here: an x vector that is not 16-byte aligned. No entry point hands the kernel one (every
vector is its own device allocation); the launcher then runs every group alone, in the gather branch
the gather groups of these cases take."""
import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd._lib import layout_of
from parallel_amg_amd.hcsr import HCSR
from parallel_amg_amd.partitioned import PSparseMatrix, PVector, mul
from test_gpu_ell_classes import check_all
from test_gpu_ell_window import bits, from_coo, options

pytestmark = pytest.mark.gpu


def upload_three(ctx, M, **opts):
    """M with group pairs allowed (ell_xwin 1), without (3) and with ell_xwin 0."""
    h = HCSR.from_arrays(M.rowptr, M.col.astype(np.int32), M.val, M.ncols)
    with options(ell_min_rows=0, sym_dia=0, **opts):
        with options(ell_xwin=1):
            A = PSparseMatrix(ctx, h)
        with options(ell_xwin=3):
            B = PSparseMatrix(ctx, h)
        with options(ell_xwin=0):
            C = PSparseMatrix(ctx, h)
    la, lb, lc = layout_of(A), layout_of(B), layout_of(C)
    assert la["ell_xwin"] and lb["ell_xwin"] and lc["ell"] and not lc["ell_xwin"], (la, lb, lc)
    cb = lb["ell_xwin_census"]
    assert cb["span_pairs"] == 0 and cb["span_singles"] == lb["ell_xwin_groups"] and cb["union_max"] == 0, lb
    # the groups and their windows are the same upload's: pairing only renumbers them
    for k in la:
        if k != "ell_xwin_census" and (k.startswith("ell_xwin") or k in ("ell_gather_groups", "tiles")):
            assert la[k] == lb[k], (k, la, lb)
    ca = la["ell_xwin_census"]
    assert 2 * ca["span_pairs"] + ca["span_singles"] == la["ell_xwin_groups"], la
    if ca["span_pairs"]:  # pamg_device.h: kEllSpanWin = (160 KB / 4 - 2 x 4 KB) / 8 doubles, kEllSpanShare = 90
        assert 0 < max(ca["union_mean"], ca["union_p95"]) <= ca["union_max"] <= (160 * 1024 // 4 - 8192) // 8, la
        assert 0.5 <= ca["union_ratio"] <= 0.9, la
    return A, B, C, ca


def bands(n, offsets, vals):
    """One value per offset (the diagonal 9): the offsets inside [0, n)."""
    rows, cols, vv = [], [], []
    for o, v in zip(offsets, vals):
        i = np.arange(max(0, -o), min(n, n - o))
        rows.append(i)
        cols.append(i + o)
        vv.append(np.full(len(i), 9.0 if o == 0 else v))
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vv)


def band_op(n, o):
    """Offsets {-o, -1, 0, 1, o}, o < 64: a slice's columns fall mostly in the slices next to it, so
    the groups are 4 consecutive slices with windows of 256 + 2 o columns; two neighbours' union is
    512 + 2 o, (512 + 2 o) / (512 + 4 o) of the two together — under 90 % from o = 32."""
    r, c, v = bands(n, (-o, -1, 0, 1, o), (-0.5, -1.25, 9.0, -1.0, -0.75))
    return from_coo(r, c, v, n)


def block_diag(blocks):
    """(rows, cols, vals, n) blocks on the diagonal of one operator."""
    rows, cols, vals, at = [], [], [], 0
    for r, c, v, n in blocks:
        rows.append(r + at)
        cols.append(c + at)
        vals.append(v)
        at += n
    return from_coo(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), at)


@pytest.fixture(scope="module")
def hier32(ctx):
    be = pa.SequentialBackend(1)
    Ah, offs, xs = pa.generate_problem(be, "poisson3d", 32)
    return pa.build_hierarchy(be, Ah, offs, pa.SAParams(max_coarse=100), device=ctx), xs


def test_level1_operator_32(ctx, hier32, capsys):
    """A1 of Poisson 32^3 (4192 rows, 66 slices — the last of 32 rows —, groups closed by the pair cap
    among them): several pairs, every op against span 1, k_rows_ell and the oracle."""
    M1 = hier32[0].levels[1][0].A
    M = O.CSR(M1.rowptr.copy(), M1.col.astype(np.int64), M1.val.copy(), M1.ncols)
    A, B, C, census = upload_three(ctx, M)
    with capsys.disabled():
        print(f"\n  A1 32^3: {census}", end="")
    assert census["span_pairs"] >= 1, census
    check_all(ctx, M, (A, B, C), 2)


def test_odd_groups_partial_slice_short_group(ctx, capsys):
    """1448 rows = 22 slices and one of 40 rows: 5 groups of 4 consecutive slices and a last one of 3,
    its last slice partial. Then 1280 rows: 5 groups, an odd number, so one stays single beside the
    pairs and both kernels run in one operator."""
    M = band_op(1448, 60)
    A, B, C, census = upload_three(ctx, M)
    la = layout_of(A)
    with capsys.disabled():
        print(f"\n  1448 rows: {census}", end="")
    assert la["ell_xwin_groups"] == 6 and la["ell_gather_groups"] == 0, la
    assert census["span_pairs"] >= 1, census
    check_all(ctx, M, (A, B, C), 2)
    M = band_op(1280, 60)
    A, B, C, census = upload_three(ctx, M)
    la = layout_of(A)
    assert la["ell_xwin_groups"] == 5 and la["ell_gather_groups"] == 0, la
    assert census["span_pairs"] >= 1 and census["span_singles"] >= 1, census
    check_all(ctx, M, (A, B, C), 2)


def mixed_blocks():
    """Three 2048-row diagonal blocks: bands with o = 40 (windows ~336, unions ~592) and o = 60 (~376 and
    ~632), and the wide rows of test_gpu_ell_window's two-path case (20 of 40 offsets within +-3000:
    windows that span the block)."""
    h = 2048
    rng = np.random.default_rng(31)
    offs = np.unique(rng.integers(-3000, 3001, 60))
    offs = offs[offs != 0][:40]
    pal = np.array([0.5, -1.25, 2.0, -0.75])
    rows, cols, vals = [], [], []
    for i in range(h):
        rows.append(i)
        cols.append(i)
        vals.append(9.0)
        for o in rng.choice(offs, 20, replace=False):
            if 0 <= i + o < h:
                rows.append(i)
                cols.append(i + int(o))
                vals.append(pal[int(rng.integers(0, 4))])
    wide = (np.array(rows), np.array(cols), np.array(vals), h)
    return block_diag([(*bands(h, (-40, -1, 0, 1, 40), (-0.5, -1.25, 9.0, -1.0, -0.75)), h),
                       (*bands(h, (-60, -1, 0, 1, 60), (0.25, -1.5, 9.0, -2.0, 0.125)), h), wide])


def test_capacity_mixes_pairs_singles_and_gathers(ctx, capsys):
    """ell_xwin_max 620: the first block's unions fit and its groups pair, the second block's windows
    fit but their unions do not — singles, but for the block's first and last two groups, whose windows
    are cut at its edges —, the third block's windows do not fit: gather groups. One
    operator, both kernels and both branches. Without the cap the second block pairs too."""
    M = mixed_blocks()
    A0, _B0, _C0, free = upload_three(ctx, M, ell_xwin_max=2048)
    A, B, C, census = upload_three(ctx, M, ell_xwin_max=620)
    la = layout_of(A)
    with capsys.disabled():
        print(f"\n  mixed blocks: cap 2048 {free}, cap 620 {census}", end="")
    assert la["ell_gather_groups"] >= 1 and la["ell_xwin_max_window"] <= 620, la
    assert census["span_pairs"] >= 1 and census["span_singles"] >= 1, census
    assert census["union_max"] <= 620 < free["union_max"] and census["span_pairs"] < free["span_pairs"], (census, free)
    check_all(ctx, M, (A, B, C, A0), 2)


def test_nothing_shared_declines(ctx):
    """Every 256-row block reads only its own columns (offsets {-5, -1, 0, 1, 5} cut at the blocks'
    edges): no group holds another's columns, the pass pairs nothing, and the layout is span 1's."""
    nb, w = 9, 256
    r, c, v = bands(w, (-5, -1, 0, 1, 5), (-0.5, -1.25, 9.0, -1.0, -0.75))
    M = block_diag([(r, c, v, w)] * nb)
    A, B, C, census = upload_three(ctx, M)
    assert census["span_pairs"] == 0 and census["span_singles"] == nb, census
    assert layout_of(A) == layout_of(B) and A.stream_bytes == B.stream_bytes
    check_all(ctx, M, (A, B, C), 2)


def test_pairs_share_little_declines(ctx):
    """Tridiagonal rows: neighbouring groups share two columns of ~260, far above kEllSpanShare."""
    r, c, v = bands(2048, (-1, 0, 1), (-1.0, 9.0, -1.25))
    M = from_coo(r, c, v, 2048)
    A, B, C, census = upload_three(ctx, M)
    assert census["span_pairs"] == 0 and census["span_singles"] == 8, census
    check_all(ctx, M, (A, B, C), 1)


def test_cycle_and_pcg_span2_equals_span1(ctx, hier32):
    """poisson3d 32^3 with ell_min_rows 0 through the solver: five V-cycles (graph replay and eager)
    and a PCG solve with the level-1 operator in pairs and in single groups, identical bits."""
    from parallel_amg_amd.solver import AMGSolver
    H, xs = hier32
    got = {}
    for span in (2, 1):
        with options(ell_min_rows=0, ell_xwin=1 if span == 2 else 3):
            S = AMGSolver(ctx, H)
        census = layout_of(S.A[1])["ell_xwin_census"]
        assert layout_of(S.A[1])["ell_xwin"] and (census["span_pairs"] >= 1) == (span == 2), census
        b = PVector(ctx, S.A[0].nrows)
        mul(b, S.A[0], PVector(ctx, S.A[0].nrows, 0, xs[0]))
        out = []
        for graph in (True, False):
            S.set_graph(graph)
            x = S.new_vector()
            hist = S.vcycle(x, b, 5, res_hist=True)
            out += [bits(x.own_values()), bits(hist)]
        x = S.new_vector()
        k, _h = S.pcg(x, b, 1e-10, 60)
        got[span] = out + [bits(x.own_values()), np.array([k])]
    for a, b in zip(got[2], got[1]):
        assert np.array_equal(a, b)
