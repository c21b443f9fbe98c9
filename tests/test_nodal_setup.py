"""Nodal aggregation on the host (SPEC §S14; no GPU): ``build_hierarchy(..., SAParams(block_size=bs))`` against
a restatement written here from the SPEC text — the node matrix as plain Python loops in the stated order, §S4.2-3
on it through ``oracle.aggregate_sets`` (the independent set-based form), the tentative expansion — fed to the
already pinned ``H.gershgorin``, ``H.spgemm``, ``H.smooth``, ``H.transpose`` and ``H.cholinv``. Every level's A, P,
R, omega, agg and the coarsest inverse are compared array for array, bit for bit.

MAX_COARSE = 40 gives elastic3d at 7^3 nodes (1029 rows) three levels; the test asserts it."""
import math
import os
import re

import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd import _lib
from parallel_amg_amd import hcsr as H
from parallel_amg_amd._lib import PamgError
from test_gpu_block_smoother import to_hcsr
from test_gpu_bsr import from_blocks, random_block_spd, var_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_COARSE = 40
THETA = 0.02


# ------------------------------------------------------------------------------ the restatement
def node_matrix_py(A, bs, need_diag=True):
    """§S14's node matrix of a global, node-blocked CSR: per stored block the sum of squares from +0.0 with d
    outer and e inner (Python floats: each square and each add rounded once), then one square root."""
    rp, col, val = A.rowptr, A.col, A.val
    nb = (len(rp) - 1) // bs
    nrp, ncol, nval = [0], [], []
    for m in range(nb):
        k0 = int(rp[bs * m])
        nblk = (int(rp[bs * m + 1]) - k0) // bs
        for k in range(nblk):
            s = 0.0
            for d in range(bs):
                for e in range(bs):
                    a = float(val[int(rp[bs * m + d]) + k * bs + e])
                    s = s + a * a
            ncol.append(int(col[k0 + k * bs]) // bs)
            nval.append(math.sqrt(s))
        nrp.append(len(ncol))
    return O.CSR(np.array(nrp, np.int64), np.array(ncol, np.int64), np.array(nval, np.float64), nb)


def tentative_py(agg, bs, nc):
    """Row bs m + d: the single entry (bs agg(m) + d, 1 / sqrt|agg(m)|); agg holds global coarse node ids."""
    cnt = np.bincount(agg[agg >= 0])
    rp, col, val = [0], [], []
    for m in range(len(agg)):
        for d in range(bs):
            if agg[m] >= 0:
                col.append(bs * int(agg[m]) + d)
                val.append(1.0 / math.sqrt(float(cnt[agg[m]])))
            rp.append(len(col))
    return H.HCSR.from_arrays(np.array(rp, np.int64), np.array(col, np.int32), np.array(val), nc)


def node_blocked(M, bs, need_diag):
    """The §S3 block-row property in numpy (what the device's build_bsr checks), plus the diagonal block."""
    rp, col = np.asarray(M.rowptr, np.int64), np.asarray(M.col, np.int64)
    if (len(rp) - 1) % bs or M.ncols % bs:
        return False
    lens = np.diff(rp).reshape(-1, bs)
    if np.any(lens != lens[:, :1]) or np.any(lens % bs):
        return False
    for m in range(lens.shape[0]):
        rows = [col[rp[bs * m + d]:rp[bs * m + d + 1]] for d in range(bs)]
        if any(not np.array_equal(r, rows[0]) for r in rows):
            return False
        c = rows[0].reshape(-1, bs)
        if np.any(c[:, 0] % bs) or np.any(c != c[:, :1] + np.arange(bs)) or np.any(np.diff(c[:, 0]) <= 0):
            return False
        if need_diag and bs * m not in c[:, 0]:
            return False
    return True


def restate(A, bs, node_offsets=None, max_coarse=MAX_COARSE, theta=THETA, agglomerate=0):
    """§S14 in the global view: a list of levels (A, P, R, omega, agg as global coarse node ids, coarse node
    offsets) and the coarsest inverse. ``node_offsets``: the parts' node offsets on level 0."""
    nparts = 1 if node_offsets is None else len(node_offsets) - 1
    noffs = None if node_offsets is None else np.asarray(node_offsets, np.int64)
    levels = []
    while True:
        n = A.nrows
        if nparts > 1 and levels and 0 < agglomerate and n <= agglomerate:
            noffs = None
        omega = 4.0 / (3.0 * H.gershgorin(A, 0))
        lev = {"A": A, "omega": omega, "noffs": noffs}
        levels.append(lev)
        if n <= max_coarse:
            break
        N = node_matrix_py(A, bs)
        agg, coffs = O.aggregate_sets(N, theta, noffs)
        nc = bs * int(coffs[-1])
        if nc == 0 or nc >= n:
            break
        T = tentative_py(agg, bs, nc)
        P = H.smooth(A, 0, T, H.spgemm(A, 0, T), omega)
        R = H.transpose(P, 0, 0, nc)
        Ac = H.spgemm(R, 0, H.spgemm(A, 0, P))
        lev.update(P=P, R=R, agg=agg, coffs=coffs)
        A, noffs = Ac, (coffs if noffs is not None else None)
    return levels, H.cholinv(A)


# ------------------------------------------------------------------------------ comparing
def stacked(hier, l, which):
    """(rowptr, col, val) of level l's operator with the parts' row blocks under one another."""
    rps, cols, vals, base = [np.zeros(1, np.int64)], [], [], 0
    for M in hier.part_rows(l, which):
        rps.append(M.rowptr[1:] + base)
        base += int(M.rowptr[-1])
        cols.append(M.col)
        vals.append(M.val)
    return np.concatenate(rps), np.concatenate(cols), np.concatenate(vals)


def same_csr(got, want, what):
    rp, col, val = got
    assert np.array_equal(rp, want.rowptr), what
    assert np.array_equal(col, want.col), what
    assert np.array_equal(val.view(np.uint64), want.val.view(np.uint64)), what


def compare(hier, levels, ainv, bs):
    assert hier.nlevels == len(levels)
    for l, lev in enumerate(levels):
        lps = [hier.levels[l][p] for p in sorted(hier.levels[l])]
        same_csr(stacked(hier, l, "A"), lev["A"], f"A_{l}")
        assert all(lp.omega == lev["omega"] for lp in lps), l
        assert node_blocked(lev["A"], bs, True), l
        if "P" not in lev:
            assert lps[0].P is None
            continue
        same_csr(stacked(hier, l, "P"), lev["P"], f"P_{l}")
        same_csr(stacked(hier, l, "R"), lev["R"], f"R_{l}")
        assert node_blocked(lev["P"], bs, False) and node_blocked(lev["R"], bs, False), l
        # LevelPart.agg: local node aggregates (creation order per part), -1 isolated
        if lps[0].whole or lev["noffs"] is None:
            got = lps[0].agg.astype(np.int64)
        else:
            got = np.concatenate([np.where(lp.agg >= 0, lp.agg.astype(np.int64) + lev["coffs"][i], -1)
                                  for i, lp in enumerate(lps)])
        assert np.array_equal(got, lev["agg"]), l
    assert np.array_equal(np.asarray(hier.ainv).view(np.uint64), ainv.view(np.uint64))


def build(M, bs, max_coarse=MAX_COARSE, **kw):
    be = pa.SequentialBackend(1)
    return pa.build_hierarchy(be, {0: to_hcsr(M)}, np.array([0, M.nrows], np.int64),
                              pa.SAParams(theta=THETA, max_coarse=max_coarse, block_size=bs, **kw))


def weak_node(bs=3, nb=10):
    """A chain of nodes, every link -B but the last, which is 1e-6 of it: the last node is isolated."""
    B = 4.0 * np.eye(bs) - np.ones((bs, bs))
    m = np.arange(nb)
    w = np.ones(nb - 1)
    w[-1] = 1e-6
    br = np.concatenate([m, m[:-1], m[1:]])
    bc = np.concatenate([m, m[1:], m[:-1]])
    bv = np.concatenate([np.broadcast_to(3.0 * B, (nb, bs, bs)), -w[:, None, None] * B, -w[:, None, None] * B])
    return from_blocks(nb, bs, br, bc, bv)


PROBLEMS = {
    "elastic3d4": (lambda: O.generate("elastic3d", 4, 4, 4), 3),
    "elastic3d5": (lambda: O.generate("elastic3d", 5, 5, 5), 3),
    "elastic3d7": (lambda: O.generate("elastic3d", 7, 7, 7), 3),
    "var5": (lambda: var_matrix(5), 3),
    "random64-bs2": (lambda: random_block_spd(64, 2, 11), 2),
    "random125-bs4": (lambda: random_block_spd(125, 4, 12), 4),
    "weak-node": (lambda: weak_node(), 3),
}


# ------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_hierarchy_has_the_bits_of_the_restatement(built, name):
    gen, bs = PROBLEMS[name]
    M = gen()
    mc = 6 if name == "weak-node" else MAX_COARSE
    hier = build(M, bs, mc)
    levels, ainv = restate(to_hcsr(M), bs, max_coarse=mc)
    assert len(levels) >= 2
    if name == "elastic3d7":
        assert len(levels) >= 3
    if name == "weak-node":
        assert levels[0]["agg"][-1] == -1 and np.all(levels[0]["agg"][:-1] >= 0)
        P = levels[0]["P"]
        assert P.rowptr[-1] > P.rowptr[-1 - bs]  # the isolated node's rows of P keep A T's pattern
    compare(hier, levels, ainv, bs)
    # the invariant: the product's own check accepts every level
    for l in range(hier.nlevels):
        A = hier.levels[l][0].A
        N = H.node_matrix(A, 0, bs)
        assert N.nrows == A.nrows // bs and N.nnz * bs * bs == A.nnz
        want = node_matrix_py(A, bs)
        assert np.array_equal(N.col, want.col) and np.array_equal(N.val.view(np.uint64), want.val.view(np.uint64))


@pytest.mark.parametrize("agglomerate", [0, 32768])
def test_two_parts_with_offsets(built, agglomerate):
    bs = 3
    M = O.generate("elastic3d", 5, 5, 5)
    A = to_hcsr(M)
    cut = 52  # nodes in part 0: not half, a multiple of nothing in particular
    offs = np.array([0, bs * cut, M.nrows], np.int64)
    parts = {}
    for p in range(2):
        a, b = int(offs[p]), int(offs[p + 1])
        lo, hi = int(A.rowptr[a]), int(A.rowptr[b])
        parts[p] = H.HCSR.from_arrays(A.rowptr[a:b + 1] - lo, A.col[lo:hi].copy(), A.val[lo:hi].copy(), A.ncols)
    hier = pa.build_hierarchy(pa.SequentialBackend(2), parts, offs,
                              pa.SAParams(theta=THETA, max_coarse=MAX_COARSE, block_size=bs, agglomerate=agglomerate))
    levels, ainv = restate(A, bs, node_offsets=offs // bs, agglomerate=agglomerate)
    assert len(levels) >= 2 and np.all(hier.offsets(1) % bs == 0)
    compare(hier, levels, ainv, bs)


def test_block_size_one_is_todays_hierarchy(built):
    be = pa.SequentialBackend(1)
    A, offs, _xs = pa.generate_problem(be, "elastic3d", 5)
    h0 = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=MAX_COARSE))
    h1 = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=MAX_COARSE, block_size=1))
    assert h0.nlevels == h1.nlevels >= 2
    for l in range(h0.nlevels):
        a, b = h0.levels[l][0], h1.levels[l][0]
        for which in ("A", "P", "R"):
            X, Y = getattr(a, which), getattr(b, which)
            if X is None:
                assert Y is None
                continue
            same_csr((X.rowptr, X.col, X.val), Y, (l, which))
        assert a.omega == b.omega and (a.agg is None) == (b.agg is None)
        assert a.agg is None or np.array_equal(a.agg, b.agg)
    assert np.array_equal(h0.ainv.view(np.uint64), h1.ainv.view(np.uint64))


def test_nodal_differs_from_scalar_aggregation(built):
    """The node aggregates are not the scalar ones: elastic3d's scalar strength mixes a node's unknowns."""
    M = O.generate("elastic3d", 5, 5, 5)
    nodal = build(M, 3)
    scalar = build(M, 1)
    assert len(nodal.levels[0][0].agg) == M.nrows // 3 and len(scalar.levels[0][0].agg) == M.nrows
    assert nodal.levels[1][0].A.nrows % 3 == 0


def drop(M, pairs):
    keep = np.ones(M.nnz, bool)
    row = np.repeat(np.arange(M.nrows), np.diff(M.rowptr))
    for r, c in pairs:
        keep &= ~((row == r) & (M.col == c))
    rp = np.concatenate(([0], np.cumsum(np.bincount(row[keep], minlength=M.nrows))))
    return O.CSR(rp.astype(np.int64), M.col[keep], M.val[keep], M.ncols)


def test_errors(built):
    M = O.generate("elastic3d", 2, 2, 2)
    # a partial block in node 5 (row 16 loses its entry in node 2's block)
    with pytest.raises(PamgError, match=r"PAMG_E_ARG.*node 5 ") as e:
        H.node_matrix(to_hcsr(drop(M, [(16, 7)])), 0, 3)
    assert e.value.code == -1
    # rows of a part from global row 12: the message names the global node
    A = to_hcsr(drop(M, [(16, 7)]))
    lo, hi = int(A.rowptr[12]), int(A.rowptr[24])
    tail = H.HCSR.from_arrays(A.rowptr[12:] - lo, A.col[lo:hi].copy(), A.val[lo:hi].copy(), A.ncols)
    with pytest.raises(PamgError, match=r"PAMG_E_ARG.*node 5 \(rows 15\.\.17\)"):
        H.node_matrix(tail, 12, 3)
    # a missing diagonal block is not node-blocked either
    with pytest.raises(PamgError, match=r"PAMG_E_ARG.*node 0 "):
        H.node_matrix(to_hcsr(drop(M, [(d, e) for d in range(3) for e in range(3)])), 0, 3)
    for bs in (1, 5):
        with pytest.raises(PamgError, match="outside 2..4") as e:
            H.node_matrix(to_hcsr(M), 0, bs)
        assert e.value.code == -1
    with pytest.raises(PamgError, match="PAMG_E_ARG"):
        H.node_matrix(to_hcsr(M), 4, 3)          # row0 not a multiple of bs
    with pytest.raises(PamgError, match="PAMG_E_ARG"):
        H.node_matrix(to_hcsr(O.generate("elastic3d", 4, 1, 1)), 0, 4)   # 12 rows, but rows of 6 and 9 entries
    with pytest.raises(PamgError, match="PAMG_E_ARG"):
        H.node_matrix(to_hcsr(O.generate("elastic3d", 3, 3, 1)), 0, 2)   # 27 rows: not whole blocks of 2
    with pytest.raises(PamgError, match="outside 2..4"):
        H.tentative_nodal(np.zeros(4, np.int32), 1, 0, 5, 5)
    # a stored diagonal block that is all zero
    Z = from_blocks(2, 2, np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1]),
                    np.array([2.0 * np.eye(2), -np.eye(2), -np.eye(2), np.zeros((2, 2))]))
    with pytest.raises(PamgError, match=r"PAMG_E_SETUP.*node 1 ") as e:
        H.node_matrix(to_hcsr(Z), 0, 2)
    assert e.value.code == -5
    # build_hierarchy: offsets and block sizes
    be = pa.SequentialBackend(2)
    A2 = {0: to_hcsr(M), 1: to_hcsr(M)}
    with pytest.raises(ValueError, match="not multiples of block_size 3"):
        pa.build_hierarchy(be, A2, np.array([0, 10, 24], np.int64), pa.SAParams(block_size=3))
    for bs in (0, 5):
        with pytest.raises(ValueError, match="outside 1..4"):
            pa.build_hierarchy(be, A2, np.array([0, 12, 24], np.int64), pa.SAParams(block_size=bs))


def test_the_entry_points_are_declared_exported_and_bound(built):
    header = open(os.path.join(ROOT, "include", "pamg.h")).read()
    julia = open(os.path.join(ROOT, "julia", "PamgHIP", "src", "PamgHIP.jl")).read()
    for name, nargs, must in (("pamg_setup_node_matrix", 4, "int bs"), ("pamg_setup_tentative_nodal", 7, "int bs"),
                              ("pamg_mat_upload_block_rows", 11, "int bs")):
        proto = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert proto and proto.group(1).count(",") == nargs - 1 and must in proto.group(1), name
        assert hasattr(_lib.lib(), name)
        assert len(_lib.SIGNATURES[name]) == nargs
        assert f"(:{name}, libpamg)" in julia
    assert "block_rows::Integer = 1" in julia
