"""The block-row layout's host-side rules (no GPU): the Python wrappers refuse a permutation together with a
block size before anything is uploaded, and the entry point is declared, exported and bound."""
import os
import re

import numpy as np
import pytest

import parallel_amg_amd as pa
from oracle import oracle as O
from parallel_amg_amd import _lib
from parallel_amg_amd import hcsr as HC
from parallel_amg_amd.partitioned import PSparseMatrix
from parallel_amg_amd.solver import AMGSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hierarchy(built):
    be = pa.SequentialBackend(1)
    A, offs, _xs = pa.generate_problem(be, "elastic3d", 4)
    return pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=20))


def test_psparsematrix_rejects_a_permutation_with_a_block_size(built):
    M = O.generate("elastic3d", 2, 2, 2)
    H = HC.HCSR.from_arrays(M.rowptr, M.col.astype(np.int32), M.val, M.ncols)
    perm = np.arange(M.nrows)[::-1].copy()
    for kw in (dict(row_perm=perm), dict(col_perm=perm), dict(row_perm=perm, col_perm=perm)):
        with pytest.raises(ValueError, match="block_size > 1 cannot be combined"):
            PSparseMatrix(None, H, block_size=3, **kw)


def test_amgsolver_raises_for_a_permuted_blocked_level(hierarchy):
    assert hierarchy.nlevels >= 2
    with pytest.raises(ValueError, match="level 0 is uploaded with a locality permutation"):
        AMGSolver(None, hierarchy, reorder="on", block_layout=3)
    with pytest.raises(ValueError, match="level 0 is uploaded with a locality permutation"):
        AMGSolver(None, hierarchy, reorder="on", block_layout={0: 3})
    with pytest.raises(ValueError, match="outside 1..4"):
        AMGSolver(None, hierarchy, reorder="off", block_layout=5)


def test_the_entry_point_is_declared_exported_and_bound(built):
    header = open(os.path.join(ROOT, "include", "pamg.h")).read()
    proto = re.search(r"int pamg_mat_upload_blocked\(([^;]*)\);", header)
    assert proto and proto.group(1).count(",") == 10 and "int bs" in proto.group(1)
    assert hasattr(_lib.lib(), "pamg_mat_upload_blocked")
    assert len(_lib.SIGNATURES["pamg_mat_upload_blocked"]) == 11
    julia = open(os.path.join(ROOT, "julia", "PamgHIP", "src", "PamgHIP.jl")).read()
    assert "(:pamg_mat_upload_blocked, libpamg)" in julia and "block_size::Integer = 1" in julia
