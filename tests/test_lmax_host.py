"""The lambda_max estimate's entry points (SPEC §S10) on the CPU: bound by the ctypes table, and
their NULL-argument errors, which are decided before any device call (no GPU in the CPU suite)."""
import numpy as np
import pytest

NEW = ("pamg_vec_fill_xstar", "pamg_estimate_lmax", "pamg_hier_set_omega")


def test_signatures_list_the_entry_points(built):
    from parallel_amg_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert getattr(_lib.lib(), name) is not None
    assert len(_lib.SIGNATURES["pamg_vec_fill_xstar"]) == 4
    assert len(_lib.SIGNATURES["pamg_estimate_lmax"]) == 7
    assert len(_lib.SIGNATURES["pamg_hier_set_omega"]) == 2


@pytest.mark.parametrize("name,args", [
    ("pamg_vec_fill_xstar", (None, None, 0, 1)),
    ("pamg_estimate_lmax", (None, None, None, None, 10, 1, None)),
    ("pamg_hier_set_omega", (None, None)),
])
def test_null_arguments(built, name, args):
    from parallel_amg_amd._lib import PamgError, call, last_error
    with pytest.raises(PamgError) as e:
        call(name, *args)
    assert e.value.code == -1
    assert name[len("pamg_"):] in last_error()


def test_null_hierarchy_with_weights(built):
    """A NULL hierarchy is refused before the weights are looked at."""
    from parallel_amg_amd._lib import PamgError, call, ptr
    om = np.array([0.5, 0.5])
    with pytest.raises(PamgError) as e:
        call("pamg_hier_set_omega", None, ptr(om))
    assert e.value.code == -1
