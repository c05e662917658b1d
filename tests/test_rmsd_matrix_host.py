"""
CPU checks of the pairwise RMSD matrix: the NumPy specification (tests/rmsd_matrix_model.py) against superposition RMSDs summed
from the residuals (tests/ensemble_model.py), its recorded float64 errors re-measured, the C ABI's two entries, the workspace's
closed form and the host-side argument checks of springcraft_amd.ensemble.
"""
import re
from os.path import dirname, join

import numpy as np
import pytest

from springcraft_amd import _hip, ensemble as ens_mod
from tests import ensemble_model as em, rmsd_matrix_model as rm

ROOT = dirname(dirname(__file__))
ENTRIES = {"sc_rmsd_matrix_workspace": 3, "sc_dev_rmsd_matrix_f64": 9}
MODEL_CASES = [(n, w, f) for n in rm.ATOMS for w in (False, True) for f in (True, False)] + [
    ("rigid", False, True), ("rigid", True, True), ("rigid", False, False), ("mirror", False, True),
    ("collinear", False, True)]


# ---- the specification against RMSDs summed from the residuals ---------------------------------------------------------------------
def _against_superposition(frames, target, weights, case, fitter=em.horn):
    """msd of every frame with the target by the model against ``fitter``'s rmsd^2; the gate adds the reference's own."""
    n = frames.shape[1]
    got = rm.rmsd_matrix(frames, target[None], weights, squared=True)[:, 0]
    ref = np.array([fitter(target, x, weights)[3] for x in frames])
    size = rm.scale(frames, target[None], weights)
    g_msd = em.gate(rm.model_errors(frames, target[None], weights), n, size)
    g_ref = em.superpose_gates(case, n, float(np.abs(target - target.mean(axis=0)).max()))[2]
    print(f"{case}: |msd - rmsd^2| {np.abs(got - ref ** 2).max():.2e}, gates {g_msd:.2e} + {(2 * ref * g_ref).max():.2e}")
    assert np.all(np.abs(got - ref ** 2) <= g_msd + 2 * ref * g_ref + g_ref ** 2)
    return got, ref


@pytest.mark.parametrize("n_atoms", [1, 2, 3, 7, 65])
@pytest.mark.parametrize("weighted", [False, True])
def test_model_against_fitted_residuals(n_atoms, weighted):
    target, frames = em.rotated_ensemble(n_atoms, 65)
    frames = frames[:12]
    w = rm.case_weights(n_atoms, weighted)
    _against_superposition(frames, target, w, n_atoms)
    if n_atoms >= 3 and not (weighted and n_atoms == 3):      # (Kabsch's SVD: float64 only, a rank the SVD can work with)
        _against_superposition(frames, target, w, n_atoms, em.kabsch)


def test_model_zero_for_rigid_copies():
    frames = rm.case_frames("rigid", 12)
    for weighted in (False, True):
        w = rm.case_weights("rigid", weighted)
        msd = rm.rmsd_matrix(frames, None, w, squared=True)
        g = rm.gate("rigid", weighted, True, rm.scale(frames, None, w))
        print(f"rigid copies: largest msd {msd.max():.2e} / {g:.2e}")
        assert msd.max() <= g and msd.min() >= 0


def test_model_zero_weight_leaves_the_atom_out():
    frames = em.perturbed_ensemble(9, 6).copy()
    w = np.ones(9)
    w[4] = 0.0
    moved = frames.copy()
    moved[:, 4] += 100.0
    a, b = rm.rmsd_matrix(frames, None, w, squared=True), rm.rmsd_matrix(moved, None, w, squared=True)
    assert np.abs(a - b).max() <= em.gate(rm.model_errors(frames, None, w), 9, rm.scale(frames, None, w))
    sub = rm.rmsd_matrix(np.delete(frames, 4, axis=1), squared=True)
    assert np.abs(a - sub).max() <= em.gate(rm.model_errors(frames, None, w), 9, rm.scale(frames, None, w))


def test_model_mirror_image_takes_the_proper_rotation():
    target, frames = em.rotated_ensemble(65, 3)
    got, ref = _against_superposition(frames * rm.MIRROR, target, None, "mirror")
    assert np.sqrt(got).min() > 1.0              # far from a fit: the reflection would give a small RMSD
    _against_superposition(frames * rm.MIRROR, target, None, "mirror", em.kabsch)


def test_model_collinear_frames():
    frames = rm.case_frames("collinear", 6)
    msd = rm.rmsd_matrix(frames, squared=True)
    assert np.all(np.isfinite(msd))
    ref = np.array([[em.kabsch(t, x)[3] for t in frames] for x in frames])
    g = rm.gate("collinear", False, True, rm.scale(frames))
    # (the reference's own error, on frames of extent 20: far below the gate's 1e-13)
    assert np.abs(msd - ref ** 2).max() <= g + 1e-14 * rm.scale(frames)


@pytest.mark.parametrize("weighted", [False, True])
def test_model_without_fit_is_the_direct_sum(weighted):
    a, b = em.perturbed_ensemble(9, 8), em.perturbed_ensemble(9, 5, seed=1)
    w = rm.case_weights(9, weighted)
    ww = np.ones(9) if w is None else w
    for other in (None, b):
        o = a if other is None else other
        direct = (ww[None, None, :] * ((a[:, None] - o[None]) ** 2).sum(axis=3)).sum(axis=2) / ww.sum()
        got = rm.rmsd_matrix(a, other, w, fit=False, squared=True)
        g = em.gate(rm.model_errors(a, other, w, fit=False), 9, rm.scale(a, other, w, fit=False))
        assert np.abs(got - direct).max() <= g
        assert np.abs(rm.rmsd_matrix(a, other, w, fit=False) - np.sqrt(got)).max() == 0


def test_model_symmetric_with_a_zero_diagonal_and_nan_frames():
    frames = em.perturbed_ensemble(7, 6).copy()
    for fit in (True, False):
        m = rm.rmsd_matrix(frames, fit=fit)
        assert np.array_equal(m, m.T) and np.all(np.diag(m) == 0) and np.all(m >= 0)
    frames[2, 3, 1] = np.nan
    for fit in (True, False):
        m = rm.rmsd_matrix(frames, fit=fit)
        bad = np.zeros((6, 6), dtype=bool)
        bad[2, :] = bad[:, 2] = True
        assert np.array_equal(np.isnan(m), bad)
    # the designed medoid: the frame in the middle of a line of frames, the first of two equal ones, never a NaN frame
    msd = np.array([[0.0, 1.0, 4.0], [1.0, 0.0, 1.0], [4.0, 1.0, 0.0]])
    assert rm.medoid(msd) == 1
    assert rm.medoid(np.array([[0.0, 2.0], [2.0, 0.0]])) == 0
    msd[1, :] = msd[:, 1] = np.nan
    assert rm.medoid(msd) == 0


@pytest.mark.parametrize("case,weighted,fit", MODEL_CASES)
def test_recorded_model_errors(case, weighted, fit):
    frames = rm.case_frames(case, rm.MODEL_FRAMES)
    measured = rm.model_errors(frames, None, rm.case_weights(case, weighted), fit)
    print(case, weighted, fit, measured)
    assert measured <= rm.MODEL_ERR[(case, weighted, fit)]


def test_every_gpu_case_has_a_recorded_error():
    assert set(MODEL_CASES) == set(rm.MODEL_ERR)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_entries_declared_exported_and_typed():
    header = open(join(ROOT, "include", "springcraft_hip.h")).read()
    assert {n for n in _hip.EXPORTED_SYMBOLS if "rmsd" in n} == set(ENTRIES)
    assert not [n for n in ENTRIES for word in ("potr", "subsystem", "vsa_batch") if word in n]
    L = _hip.lib()
    for name, nargs in ENTRIES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        args = re.search(rf"\b(?:int|int64_t) {name}\(([^;]*)\);", header).group(1)
        assert len(args.split(",")) == nargs, name
    # the entry refuses a missing context before anything else
    assert L.sc_dev_rmsd_matrix_f64(None, None, 1, None, 1, 1, None, 1, None) == _hip.SC_ERR_INVALID_ARG


def _closed_form(n_a, n_b, n_atoms):
    up = lambda v, m: (v + m - 1) // m * m        # noqa: E731
    rows = 3 * up(n_atoms, 8)
    regions = [8 * rows * up(n_a, 64), 8 * up(n_a, 64)]
    regions += [8 * rows * up(n_b, 64), 8 * up(n_b, 64)] if n_b else [1, 1]      # (an empty region occupies one byte)
    regions.append(8)
    off = 0
    for r in regions:
        off = up(off, 256) + r
    return off


@pytest.mark.parametrize("n_a,n_b,n_atoms", [(1, 0, 1), (64, 0, 8), (65, 0, 9), (130, 0, 257), (65, 3, 65), (3, 130, 7),
                                            (10000, 0, 2000), (200, 10000, 50000)])
def test_workspace_closed_form(n_a, n_b, n_atoms):
    assert _hip.lib().sc_rmsd_matrix_workspace(n_a, n_b, n_atoms) == _closed_form(n_a, n_b, n_atoms)


def test_workspace_refuses_what_cannot_be_indexed():
    ws = _hip.lib().sc_rmsd_matrix_workspace
    for bad in ((0, 0, 5), (-1, 0, 5), (5, -1, 5), (5, 0, 0), (2 ** 31, 0, 5), (5, 2 ** 31, 5), (5, 0, 2 ** 31 // 3),
                (2 ** 30, 0, 2 ** 29), (2 ** 24, 0, 8)):
        assert ws(*bad) == -1, bad
    assert ws(2 ** 20, 0, 8) > 0


# ---- host-side argument checks: all raise before any device call (there is no device here) ------------------------------------------------
def test_convenience_argument_checks():
    import springcraft_amd as sc

    assert sc.rmsd_matrix is ens_mod.rmsd_matrix and "rmsd_matrix" in ens_mod.__all__
    for bad in (np.zeros((4, 5)), np.zeros((4, 5, 2))):
        with pytest.raises(ValueError, match="shape"):
            sc.rmsd_matrix(bad)
    with pytest.raises(ValueError, match="at least one frame"):
        sc.rmsd_matrix(np.zeros((0, 5, 3)))
    with pytest.raises(ValueError, match="other with shape"):
        sc.rmsd_matrix(np.zeros((4, 5, 3)), other=np.zeros((5, 3)))
    with pytest.raises(ValueError, match="other has 4 atoms, coords 5"):
        sc.rmsd_matrix(np.zeros((4, 5, 3)), other=np.zeros((2, 4, 3)))
    with pytest.raises(IndexError, match="weights for 5 atoms"):
        sc.rmsd_matrix(np.zeros((4, 5, 3)), weights=np.ones(4))
    with pytest.raises(ValueError, match="not negative"):
        sc.rmsd_matrix(np.zeros((4, 5, 3)), weights=[1, 1, -1, 1, 1])


def test_shape_and_weight_checks():
    ws = _hip.lib().sc_rmsd_matrix_workspace
    assert ens_mod._checked_matrix_shape(130, None, 257, ws) == (130, 130)
    assert ens_mod._checked_matrix_shape(65, 3, 9, ws) == (65, 3)
    with pytest.raises(ValueError, match="2\\^31 - 1 entries per side"):
        ens_mod._checked_matrix_shape(2 ** 31, None, 9, ws)
    with pytest.raises(ValueError, match="2\\^31 - 1 entries per side"):
        ens_mod._checked_matrix_shape(5, 2 ** 31, 9, ws)
    with pytest.raises(ValueError, match="index range"):
        ens_mod._checked_matrix_shape(2 ** 30, None, 2 ** 29, ws)
    w = np.arange(5.0)
    assert ens_mod._same_weights(None, None) and ens_mod._same_weights(w, w.copy())
    assert not ens_mod._same_weights(None, w) and not ens_mod._same_weights(w, None)
    assert not ens_mod._same_weights(w, w + 1) and not ens_mod._same_weights(w, np.arange(4.0))


class _Stub(ens_mod.Ensemble):
    """An ensemble's host side alone, for the checks of ``other`` that come before any device call."""

    def __init__(self, n_frames, n_atoms, weights=None, device="cuda:0"):
        self.n_frames, self.n_atoms, self.weights, self.device = n_frames, n_atoms, weights, device


def test_other_must_match():
    me = _Stub(4, 5, np.ones(5))
    assert me._checked_other(None) is None
    assert me._checked_other(_Stub(7, 5, np.ones(5))).n_frames == 7
    with pytest.raises(ValueError, match="must be an Ensemble"):
        me._checked_other(np.zeros((4, 5, 3)))
    with pytest.raises(ValueError, match="other has 6 atoms"):
        me._checked_other(_Stub(4, 6, np.ones(6)))
    with pytest.raises(ValueError, match="same atom weights"):
        me._checked_other(_Stub(4, 5, None))
    with pytest.raises(ValueError, match="same atom weights"):
        me._checked_other(_Stub(4, 5, 2 * np.ones(5)))
    with pytest.raises(ValueError, match="other is on cuda:1"):
        me._checked_other(_Stub(4, 5, np.ones(5), device="cuda:1"))
