"""Operators stored in binary32 (SPEC §S15), the host side: ``hierarchy.round_values`` against an element-wise
restatement, its overflow error, and a static check that the default ``AMGSolver`` path constructs nothing new.
No GPU: the hierarchies are built by the host setup."""
import ast
import dataclasses
import inspect
import textwrap

import numpy as np
import pytest

import parallel_amg_amd as pa
from parallel_amg_amd import hierarchy as HY
from parallel_amg_amd.hcsr import HCSR
from parallel_amg_amd.solver import AMGSolver


@pytest.fixture(scope="module")
def small(built):
    be = pa.SequentialBackend(2)
    A, offs, _xs = pa.generate_problem(be, "elastic3d", 4)
    H = pa.build_hierarchy(be, A, offs, pa.SAParams(max_coarse=40))
    assert H.nlevels >= 2
    return H


def rn32(v):
    """Element by element: the binary32 nearest to v (ties to even), widened again."""
    return np.array([float(np.float32(float(a))) for a in v], np.float64)


def test_round_values_is_the_elementwise_rounding(small):
    H = small
    Hr = HY.round_values(H)
    assert Hr is not H and Hr.nlevels == H.nlevels and Hr.nparts == H.nparts
    changed = 0
    for l in range(H.nlevels):
        assert sorted(Hr.levels[l]) == sorted(H.levels[l])
        for p, lp in H.levels[l].items():
            lr = Hr.levels[l][p]
            for which in ("A", "P", "R"):
                M, Mr = getattr(lp, which), getattr(lr, which)
                if M is None:
                    assert Mr is None
                    continue
                assert Mr is not M and (Mr.nrows, Mr.ncols, Mr.nnz) == (M.nrows, M.ncols, M.nnz)
                assert np.array_equal(Mr.rowptr, M.rowptr) and np.array_equal(Mr.col, M.col)
                want = rn32(M.val)
                assert np.array_equal(Mr.val.view(np.int64), want.view(np.int64)), (l, p, which)
                changed += int(np.count_nonzero(want != M.val))
            # everything else is H's own
            assert lr.omega == lp.omega and lr.rho == lp.rho and lr.whole == lp.whole
            for f in ("offsets", "planA", "planP", "planR", "agg"):
                assert getattr(lr, f) is getattr(lp, f), f
    assert changed > 0                      # (the smoothed operators are not exact in binary32)
    assert Hr.ainv is H.ainv and Hr.n_coarse == H.n_coarse and Hr.rep_level == H.rep_level
    assert Hr.rep_offsets is H.rep_offsets and Hr.block_size == H.block_size and Hr.parts is H.parts
    # H itself is untouched, and rounding twice changes nothing more
    Hrr = HY.round_values(Hr)
    for l in range(H.nlevels):
        for p in H.levels[l]:
            assert np.array_equal(Hrr.levels[l][p].A.val.view(np.int64), Hr.levels[l][p].A.val.view(np.int64))


def test_rounding_edges_on_the_host(built):
    big = float(np.finfo(np.float32).max)
    below = np.nextafter(2.0 ** 128 - 2.0 ** 103, 0.0)
    v = np.array([1.0 + 2.0 ** -24, 1.0 + 2.0 ** -23 + 2.0 ** -24, 1e-40, 1e-50, -1e-50, big, below, np.inf, -np.inf])
    M = HCSR.from_arrays(np.array([0, len(v)], np.int64), np.arange(len(v), dtype=np.int32), v, len(v))
    Mr = HY.round_f32(M)                                      # (kept: val is a view into it)
    r = Mr.val
    assert r[0] == 1.0 and r[1] == 1.0 + 2.0 ** -22          # ties go to the even significand
    assert r[2] == 71362 * 2.0 ** -149                        # an f32 subnormal, kept
    assert r[3] == 0.0 and not np.signbit(r[3]) and r[4] == 0.0 and np.signbit(r[4])
    assert r[5] == big and r[6] == big and r[7] == np.inf and r[8] == -np.inf
    nan = HCSR.from_arrays(np.array([0, 1], np.int64), np.array([0], np.int32), np.array([np.nan]), 1)
    nr = HY.round_f32(nan)
    assert np.isnan(nr.val[0])


@pytest.mark.parametrize("which", ["A", "P", "R"])
def test_overflow_raises(small, which):
    H = small
    lp = H.levels[0][1]
    M = getattr(lp, which)
    val = M.val.copy()
    k = int(M.rowptr[2])                                      # the first entry of row 2
    val[k] = -(2.0 ** 128 - 2.0 ** 103)                       # the smallest magnitude that rounds to an infinity
    bad = HCSR.from_arrays(M.rowptr, M.col, val, M.ncols)
    levels = [dict(lev) for lev in H.levels]
    levels[0][1] = dataclasses.replace(lp, **{which: bad})
    with pytest.raises(ValueError, match=rf"row 2, column {int(M.col[k])}\b.*infinite binary32"):
        HY.round_values(dataclasses.replace(H, levels=levels))
    val[k] = np.nextafter(val[k], 0.0)                        # the double just inside: FLT_MAX
    levels[0][1] = dataclasses.replace(lp, **{which: HCSR.from_arrays(M.rowptr, M.col, val, M.ncols)})
    Hr = HY.round_values(dataclasses.replace(H, levels=levels))
    assert getattr(Hr.levels[0][1], which).val[k] == -float(np.finfo(np.float32).max)


def test_the_default_path_constructs_nothing_new():
    """Static: ``values`` defaults to "f64", and everything the feature adds to ``AMGSolver.__init__`` — the
    rounded hierarchy, the second upload of A_0, the outer operator — sits under an ``if values == "f32"``."""
    sig = inspect.signature(AMGSolver.__init__)
    assert sig.parameters["values"].default == "f64"
    assert list(sig.parameters)[:7] == ["self", "ctx", "H", "part", "graph", "reorder", "block_layout"]
    tree = ast.parse(textwrap.dedent(inspect.getsource(AMGSolver.__init__)))

    def is_f32_test(t):
        if isinstance(t, ast.BoolOp) and isinstance(t.op, ast.And):
            return any(is_f32_test(v) for v in t.values)
        return (isinstance(t, ast.Compare) and isinstance(t.left, ast.Name) and t.left.id == "values"
                and len(t.ops) == 1 and isinstance(t.ops[0], ast.Eq)
                and isinstance(t.comparators[0], ast.Constant) and t.comparators[0].value == "f32")

    guarded, seen = set(), set()
    for node in ast.walk(tree):
        if isinstance(node, ast.If) and is_f32_test(node.test):
            for stmt in node.body:
                guarded.update(id(n) for n in ast.walk(stmt))
    new = {"round_values", "set_fine_operator", "pamg_hier_set_outer", "H_exact"}
    for node in ast.walk(tree):
        name = (node.id if isinstance(node, ast.Name) and isinstance(node.ctx, ast.Load) else
                node.attr if isinstance(node, ast.Attribute) else
                node.value if isinstance(node, ast.Constant) and isinstance(node.value, str) else None)
        if name in new:
            seen.add(name)
            assert id(node) in guarded, f"{name} is reached outside `if values == \"f32\"` (line {node.lineno})"
        if isinstance(node, (ast.Import, ast.ImportFrom)) and id(node) not in guarded:
            assert "round_values" not in [a.name for a in node.names]
    assert {"round_values", "set_fine_operator", "H_exact"} <= seen
    with pytest.raises(ValueError, match="'f64' or 'f32'"):
        AMGSolver(None, None, values="f16")
