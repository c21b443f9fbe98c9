"""Chebyshev smoother, host side (SPEC §S9): pamg_chebyshev_coeffs against a restatement in Python
floats, bit for bit, and the argument errors of the new entry points. No GPU."""
import ctypes as C

import numpy as np
import pytest

from parallel_amg_amd import _lib
from parallel_amg_amd._lib import PamgError, call, ptr
from parallel_amg_amd.partitioned import chebyshev_coeffs

E_ARG = -1  # include/pamg.h PAMG_E_ARG


def coeffs_ref(lmax, ratio, m):
    """SPEC §S9 in Python floats (IEEE doubles, one rounding per operation, never fused)."""
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
    return np.array(c1), np.array(c2)


CASES = [(2.0, 4.0, m) for m in range(1, 6)] + [(3.3333333333333335, 30.0, 4), (2.159, 1.5, 64)]


@pytest.mark.parametrize("lmax,ratio,m", CASES)
def test_coeffs_bits(built, lmax, ratio, m):
    c1, c2 = chebyshev_coeffs(lmax, ratio, m)
    w1, w2 = coeffs_ref(lmax, ratio, m)
    assert len(c1) == m and len(c2) == m
    assert np.array_equal(c1.view(np.int64), w1.view(np.int64))
    assert np.array_equal(c2.view(np.int64), w2.view(np.int64))
    assert c1[0] == 0.0 and c2[0] == 1.0 / ((lmax + lmax / ratio) / 2.0)
    assert np.all(c2 > 0) and np.all(c1[1:] > 0) and np.all(c1 < 1)


def test_coeffs_are_a_prefix_of_any_higher_degree(built):
    """Step k's coefficients do not depend on the degree (the hierarchy stores one table per level)."""
    a1, a2 = chebyshev_coeffs(2.159, 4.0, 64)
    for m in (1, 2, 3, 7):
        c1, c2 = chebyshev_coeffs(2.159, 4.0, m)
        assert np.array_equal(c1.view(np.int64), a1[:m].view(np.int64))
        assert np.array_equal(c2.view(np.int64), a2[:m].view(np.int64))


@pytest.mark.parametrize("lmax,ratio,m", [(2.0, 1.0, 2), (2.0, 0.5, 2), (2.0, float("nan"), 2), (0.0, 4.0, 2),
                                          (-1.0, 4.0, 2), (2.0, 4.0, 0), (2.0, 4.0, 65), (2.0, 4.0, -3)])
def test_coeffs_argument_errors(built, lmax, ratio, m):
    c1, c2 = np.zeros(80), np.zeros(80)
    rc = _lib.lib().pamg_chebyshev_coeffs(lmax, ratio, m, ptr(c1), ptr(c2))
    assert rc == E_ARG
    assert "chebyshev_coeffs" in _lib.last_error()
    with pytest.raises(PamgError):
        chebyshev_coeffs(lmax, ratio, m)


def test_null_arguments(built):
    L = _lib.lib()
    c = np.zeros(4)
    assert L.pamg_chebyshev_coeffs(2.0, 4.0, 2, None, ptr(c)) == E_ARG
    assert L.pamg_chebyshev_coeffs(2.0, 4.0, 2, ptr(c), None) == E_ARG
    assert L.pamg_chebyshev(None, None, None, None, None, None, 2.0, 4.0, 2) == E_ARG
    assert L.pamg_hier_set_smoother(None, 1, None, 4.0) == E_ARG
    with pytest.raises(PamgError):
        call("pamg_hier_set_smoother", None, 0, None, C.c_double(4.0))
