"""pamg_setup_block_diag (SPEC §S12) on the host: the node blocks against a numpy extraction and their
inverses against a pure-Python restatement of §S5, both bit for bit; rho_b against scipy; the errors."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from parallel_amg_amd import hcsr as HC
from parallel_amg_amd._lib import PamgError


def bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def to_hcsr(M, r0=0, r1=None):
    r1 = M.nrows if r1 is None else r1
    sl = slice(M.rowptr[r0], M.rowptr[r1])
    return HC.HCSR.from_arrays(M.rowptr[r0:r1 + 1] - M.rowptr[r0], M.col[sl].astype(np.int32), M.val[sl], M.ncols)


def blocks_ref(M, bs):
    """Row i's entries a_ij with j in i's block, absent ones 0.0 (a numpy extraction)."""
    rows = np.repeat(np.arange(M.nrows), np.diff(M.rowptr))
    inb = M.col // bs == rows // bs
    out = np.zeros((M.nrows, bs))
    out[rows[inb], M.col[inb] % bs] = M.val[inb]
    return out


def cholinv_ref(D):
    """SPEC §S5 on one small dense block, in Python floats: inv[i][c] = z_i of the unit vector e_c."""
    n = len(D)
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        d = D[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        assert d > 0.0
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, n):
            s = D[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    inv = [[0.0] * n for _ in range(n)]
    for c in range(n):
        y = [0.0] * n
        for i in range(n):
            s = 1.0 if i == c else 0.0
            for k in range(i):
                s = s - L[i][k] * y[k]
            y[i] = s / L[i][i]
        for i in range(n - 1, -1, -1):
            s = y[i]
            for k in range(n - 1, i, -1):
                s = s - L[k][i] * inv[k][c]
            inv[i][c] = s / L[i][i]
    return inv


def inv_ref(blocks, bs):
    out = np.zeros_like(blocks)
    for m in range(len(blocks) // bs):
        D = [[float(v) for v in row] for row in blocks[m * bs:(m + 1) * bs]]
        out[m * bs:(m + 1) * bs] = cholinv_ref(D)
    return out


def rho_ref(M, inv, bs):
    import scipy.sparse as sp
    nb = M.nrows // bs
    Dinv = sp.block_diag([inv[m * bs:(m + 1) * bs] for m in range(nb)], format="csr")
    return abs(Dinv @ M.to_scipy()).sum(axis=1).max()


def hand_3x3():
    a = np.array([[4.0, -1.0, 0.5], [-1.0, 3.0, -0.25], [0.5, -0.25, 2.0]])
    return O.CSR(np.array([0, 3, 6, 9], np.int64), np.tile(np.arange(3, dtype=np.int64), 3), a.reshape(-1).copy(), 3)


CASES = {"elastic3d4-bs3": (lambda: O.generate("elastic3d", 4, 4, 4), 3),
         "poisson3d8-bs2": (lambda: O.generate("poisson3d", 8, 8, 8), 2),
         "poisson3d8-bs4": (lambda: O.generate("poisson3d", 8, 8, 8), 4),
         "hand3x3-bs3": (hand_3x3, 3)}


@pytest.mark.parametrize("name", list(CASES))
def test_blocks_inverse_and_bound(built, name):
    gen, bs = CASES[name]
    M = gen()
    blocks, inv, rho = HC.block_diag(to_hcsr(M), 0, bs)
    want_b = blocks_ref(M, bs)
    assert np.array_equal(bits(blocks), bits(want_b))
    assert np.array_equal(bits(inv), bits(inv_ref(want_b, bs)))
    want_rho = rho_ref(M, inv, bs)
    print(f"\n  {name}: rho_b {rho!r}, scipy {want_rho!r}")
    assert abs(rho - want_rho) <= 1e-12 * want_rho
    if name.startswith("elastic3d"):
        assert abs(rho - 2.0) <= 1e-12


def test_a_part_of_the_rows(built):
    """Rows [96, 192) of elastic3d 4^3 with global columns: the blocks of those rows, and rho_b over
    them alone."""
    M, bs = O.generate("elastic3d", 4, 4, 4), 3
    fb, fi, _ = HC.block_diag(to_hcsr(M), 0, bs)
    blocks, inv, rho = HC.block_diag(to_hcsr(M, 96, 192), 96, bs)
    assert np.array_equal(bits(blocks), bits(fb[96:192]))
    assert np.array_equal(bits(inv), bits(fi[96:192]))
    import scipy.sparse as sp
    Dinv = sp.block_diag([fi[m * bs:(m + 1) * bs] for m in range(M.nrows // bs)], format="csr")
    want = abs(Dinv @ M.to_scipy()).sum(axis=1)[96:192].max()
    assert abs(rho - want) <= 1e-12 * want


def test_errors(built):
    M = O.generate("poisson3d", 3, 3, 3)  # 27 rows
    H = to_hcsr(M)
    for bs in (1, 5):
        with pytest.raises(PamgError) as e:
            HC.block_diag(H, 0, bs)
        assert e.value.code == -1
    for row0, bs in ((0, 2), (0, 4), (1, 3)):  # 27 rows are no multiple of 2 or 4; row0 = 1 none of 3
        with pytest.raises(PamgError) as e:
            HC.block_diag(H, row0, bs)
        assert e.value.code == -1, e.value
    a = np.array([[4.0, 0.0, 0.0, 0.0], [0.0, 1.0, 2.0, 0.0], [0.0, 2.0, 1.0, 0.0], [0.0, 0.0, 0.0, 3.0]])
    rp = np.arange(0, 17, 4, dtype=np.int64)
    Hd = HC.HCSR.from_arrays(rp, np.tile(np.arange(4, dtype=np.int32), 4), a.reshape(-1), 4)
    with pytest.raises(PamgError) as e:  # one block of 4 whose middle [[1, 2], [2, 1]] makes it indefinite
        HC.block_diag(Hd, 0, 4)
    assert e.value.code == -5 and "block 0" in str(e.value), e.value
    b2 = np.array([[2.0, 0.0, 0.0, 0.0], [0.0, 2.0, 0.0, 0.0], [0.0, 0.0, 1.0, 2.0], [0.0, 0.0, 2.0, 1.0]])
    Hb = HC.HCSR.from_arrays(rp, np.tile(np.arange(4, dtype=np.int32), 4), b2.reshape(-1), 4)
    with pytest.raises(PamgError) as e:  # the second block of two, [[1, 2], [2, 1]], is indefinite
        HC.block_diag(Hb, 0, 2)
    assert e.value.code == -5 and "block 1" in str(e.value), e.value
