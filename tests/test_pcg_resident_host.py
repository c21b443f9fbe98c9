"""The host side of pamg_pcg_resident (SPEC §S11), without a GPU: the stopping bound
pamg_pcg_rr_threshold — the largest double whose correctly rounded square root is <= thr, so that
the device's rr_k <= rr_max is §S8's RN(sqrt(rr_k)) <= thr — and the argument checks that come
before any device call."""
import ctypes as C
import sys

import numpy as np
import pytest

from parallel_amg_amd import _lib

E_ARG = -1
DBL_MAX = sys.float_info.max
EDGES = [
    3.0,                               # an exact square
    1e-160, 1e-170,                    # thr^2 subnormal / zero
    5e-324,
    2.0 ** -537, 2.0 ** -538,          # thr^2 = the smallest subnormal / a quarter of it
    1.3407807929942596e154,            # thr^2 at the overflow edge ...
    float(np.nextafter(1.3407807929942596e154, np.inf)),  # ... and past it
    1e200,
    DBL_MAX,
]


@pytest.fixture(scope="module")
def threshold(built):
    L = _lib.lib()

    def f(thr):
        out = C.c_double(-1.0)
        rc = L.pamg_pcg_rr_threshold(float(thr), C.byref(out))
        return rc, out.value
    return f


def check(threshold, thr):
    rc, c = threshold(thr)
    assert rc == 0, (thr, _lib.last_error())
    with np.errstate(over="ignore"):
        assert np.sqrt(np.float64(c)) <= thr, (thr, c)
        if c < DBL_MAX:
            assert np.sqrt(np.nextafter(np.float64(c), np.inf)) > thr, (thr, c)
        else:  # nothing above DBL_MAX but inf, whose root is > every finite thr
            assert c == DBL_MAX and np.isfinite(thr)
    return c


@pytest.mark.parametrize("thr", EDGES)
def test_threshold_edges(threshold, thr):
    check(threshold, thr)


def test_threshold_values(threshold):
    assert check(threshold, 3.0) == 9.0
    assert check(threshold, 1e-170) == 0.0
    assert check(threshold, 2.0 ** -538) == 0.0
    assert check(threshold, 2.0 ** -537) == 5e-324
    assert check(threshold, DBL_MAX) == DBL_MAX
    assert threshold(0.0) == (0, 0.0)
    assert threshold(float("inf")) == (0, float("inf"))


def test_threshold_random(threshold):
    rng = np.random.default_rng(20251)
    # exponents over the whole range (subnormals included), random mantissas
    e = rng.integers(-1074, 1024, 10000)
    m = 1.0 + rng.random(10000)
    with np.errstate(over="ignore", under="ignore"):
        thr = np.ldexp(m, e)
    thr = thr[np.isfinite(thr) & (thr > 0)]
    assert len(thr) > 9900 and thr.min() < 1e-300 and thr.max() > 1e300
    for t in thr:
        check(threshold, float(t))


def test_threshold_bad_arguments(threshold):
    L = _lib.lib()
    assert threshold(float("nan"))[0] == E_ARG
    assert threshold(-1.0)[0] == E_ARG
    assert L.pamg_pcg_rr_threshold(1.0, None) == E_ARG


@pytest.mark.parametrize("rtol,maxit,lookahead", [(1e-8, 10, 0), (1e-8, 10, -1), (1e-8, -1, 0), (float("nan"), 10, 0)])
def test_argument_errors_need_no_device(built, rtol, maxit, lookahead):
    """NULL handles and out-of-range values are refused before the device is touched."""
    L = _lib.lib()
    it, stats = C.c_int(7), (C.c_int * 2)(7, 7)
    rc = L.pamg_pcg_resident(None, None, None, None, rtol, maxit, lookahead, C.byref(it), None, stats)
    assert rc == E_ARG
    assert "pcg_resident" in _lib.last_error()
    assert it.value == 7 and list(stats) == [7, 7]
