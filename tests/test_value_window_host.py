"""
Argument checks of ``subset_by_value`` (the eigenvalue window, scipy's semantics) that run before any device call, so
they hold on a host without a GPU: the errors are the ones ``scipy.linalg.eigh`` raises for the same arguments.
"""
import numpy as np
import pytest

import springcraft_amd as sc
from springcraft_amd import nma
from springcraft_amd.batch import DeviceBatchSolver

BAD_WINDOWS = [(2.0, 1.0), (1.0, 1.0), (np.inf, np.inf), (-np.inf, -np.inf), (np.nan, 1.0), (0.0, np.nan),
               (np.nan, np.nan)]


def _scipy_message(**kw):
    import scipy.linalg

    with pytest.raises(ValueError) as e:
        scipy.linalg.eigh(np.eye(3), **kw)
    return str(e.value)


def _model(kind):
    coord = np.random.RandomState(0).rand(12, 3) * 10
    ff = sc.InvariantForceField(7.0)
    return sc.ANM(coord, ff) if kind == "anm" else sc.GNM(coord, ff)


@pytest.mark.parametrize("window", BAD_WINDOWS, ids=str)
def test_bad_bounds_raise_as_scipy(window):
    msg = _scipy_message(subset_by_value=window)
    with pytest.raises(ValueError) as e:
        nma.eigh(np.eye(3), subset_by_value=window)
    assert str(e.value) == msg, (str(e.value), msg)


@pytest.mark.parametrize("window", BAD_WINDOWS, ids=str)
@pytest.mark.parametrize("kind", ["anm", "gnm"])
def test_bad_bounds_raise_on_models(kind, window):
    with pytest.raises(ValueError, match="eigenvalue bounds are not valid"):
        _model(kind).eigen(subset_by_value=window)
    with pytest.raises(ValueError, match="eigenvalue bounds are not valid"):
        nma.eigen(_model(kind), subset_by_value=window)


def test_both_subsets_raise_as_scipy():
    msg = _scipy_message(subset_by_index=(0, 1), subset_by_value=(0.0, 1.0))
    with pytest.raises(ValueError) as e:
        nma.eigh(np.eye(3), subset_by_index=(0, 1), subset_by_value=(0.0, 1.0))
    assert str(e.value) == msg
    for kind in ("anm", "gnm"):
        with pytest.raises(ValueError, match="Either index or value subset"):
            _model(kind).eigen(subset_by_index=(0, 1), subset_by_value=(0.0, 1.0))


def test_batch_solver_checks_before_the_device():
    ff = sc.InvariantForceField(7.0)
    with pytest.raises(ValueError, match="needs max_modes"):
        DeviceBatchSolver(10, 2, ff, subset_by_value=(0.0, 1.0))
    for k in (0, -1, 31):
        with pytest.raises(ValueError, match="max_modes"):
            DeviceBatchSolver(10, 2, ff, subset_by_value=(0.0, 1.0), max_modes=k)
    with pytest.raises(ValueError, match="max_modes"):
        DeviceBatchSolver(10, 2, ff, dim=1, subset_by_value=(0.0, 1.0), max_modes=11)
    with pytest.raises(ValueError, match="max_modes applies to subset_by_value"):
        DeviceBatchSolver(10, 2, ff, max_modes=4)
    with pytest.raises(ValueError, match="Either index or value subset"):
        DeviceBatchSolver(10, 2, ff, subset_by_index=(0, 3), subset_by_value=(0.0, 1.0), max_modes=4)
    for window in BAD_WINDOWS:
        with pytest.raises(ValueError, match="eigenvalue bounds are not valid"):
            DeviceBatchSolver(10, 2, ff, subset_by_value=window, max_modes=4)


def test_value_window_accepts_infinite_bounds():
    assert nma._value_window((-np.inf, np.inf)) == (-np.inf, np.inf)
    assert nma._value_window((0, 1)) == (0.0, 1.0)
    assert nma._value_window(None, (0, 3)) is None
