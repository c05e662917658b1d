"""
GPU checks of the pairwise RMSD matrix (csrc/rmsd_matrix.hip) against the NumPy specification of tests/rmsd_matrix_model.py,
gated as that module's docstring says: in msd, 8 times the specification's own float64 error (recorded there, re-measured by
tests/test_rmsd_matrix_host.py) with the floor N eps scale; rmsd where msd is above 1e4 gates.  Every comparison prints its
measured / gate ratio.
"""
import numpy as np
import pytest

from tests import ensemble_model as em, rmsd_matrix_model as rm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


def both(sc, frames, weights, fit, other=None):
    """(msd, rmsd) of the device as ndarrays: one ensemble, two calls."""
    ens = sc.Ensemble(frames, weights=weights)
    oth = None if other is None else sc.Ensemble(other, weights=weights)
    msd, rmsd = ens.rmsd_matrix(oth, fit=fit, squared=True), ens.rmsd_matrix(oth, fit=fit)
    assert msd.is_cuda and str(msd.dtype) == "torch.float64"
    assert tuple(msd.shape) == (len(frames), len(frames) if other is None else len(other))
    return msd.cpu().numpy(), rmsd.cpu().numpy()


# ---- 1. against the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n_atoms", rm.ATOMS)
@pytest.mark.parametrize("n_frames", rm.FRAMES)
def test_matches_the_model(sc, n_frames, n_atoms, weighted, fit):
    frames, w, ref, _ = rm.reference(n_atoms, weighted, fit)
    x = frames[:n_frames]
    msd, rmsd = both(sc, x, w, fit)
    g = rm.gate(n_atoms, weighted, fit, rm.scale(x, None, w, fit))
    rm.compare(msd, rmsd, ref[:n_frames, :n_frames], g, f"M={n_frames} N={n_atoms} w={weighted} fit={fit}")


# ---- 2. other= --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n_a,n_b", [(65, 3), (3, 130), (64, 64)])
def test_other_agrees_with_the_self_result(sc, n_a, n_b, weighted, fit):
    frames, w, ref, _ = rm.reference(65, weighted, fit)
    a, b = frames[:n_a], frames[:n_b]
    msd, rmsd = both(sc, a, w, fit, other=b)
    g = rm.gate(65, weighted, fit, rm.scale(a, b, w, fit))
    # the model's self result: the pair (f, g) and the diagonal come from other arithmetic here (S^T; no exact zero)
    rm.compare(msd, rmsd, ref[:n_a, :n_b], g, f"other {n_a} x {n_b} w={weighted} fit={fit}")
    self_msd = both(sc, frames[:max(n_a, n_b)], w, fit)[0]
    assert np.abs(msd - self_msd[:n_a, :n_b]).max() <= g


def test_other_with_other_frames(sc):
    a, b = rm.case_frames(9, 65), em.perturbed_ensemble(9, 70, seed=1)
    w = rm.case_weights(9, True)
    for fit in (True, False):
        msd, rmsd = both(sc, a, w, fit, other=b)
        ref = rm.rmsd_matrix(a, b, w, fit, squared=True)
        rm.compare(msd, rmsd, ref, rm.gate(9, True, fit, rm.scale(a, b, w, fit)), f"other frames fit={fit}")


# ---- 3. structure of the self result ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
def test_symmetric_bit_for_bit_with_a_zero_diagonal(sc, weighted, fit):
    frames, w, _, _ = rm.reference(65, weighted, fit)
    for m in both(sc, frames, w, fit):
        assert np.array_equal(m.view(np.int64), m.T.view(np.int64))
        assert np.all(np.diag(m).view(np.int64) == 0)          # +0.0
        assert np.all(m >= 0)


@pytest.mark.parametrize("weighted", [False, True])
def test_rigid_copies_are_within_the_gate_of_zero(sc, weighted):
    frames, w = rm.case_frames("rigid"), rm.case_weights("rigid", weighted)
    msd, rmsd = both(sc, frames, w, True)
    g = rm.gate("rigid", weighted, True, rm.scale(frames, None, w))
    print(f"rigid copies w={weighted}: largest msd {msd.max():.2e} / {g:.2e} = {msd.max() / g:.3f}")
    assert msd.min() >= 0 and msd.max() <= g
    assert rmsd.max() <= np.sqrt(g) * (1 + 4 * rm.EPS)


# ---- 4. bits do not depend on size, position or neighbours ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms", [9, 65])
def test_bits_depend_on_the_pair_alone(sc, n_atoms):
    frames, w = rm.case_frames(n_atoms), rm.case_weights(n_atoms, True)
    bits = lambda x, fit: both(sc, x, w, fit)[1].view(np.int64)       # noqa: E731
    full = bits(frames, True)
    assert np.array_equal(bits(frames, True), full)                               # two calls
    assert np.array_equal(bits(frames[:70], True), full[:70, :70])                # another size, another pad
    assert np.array_equal(bits(frames[5:], True), full[5:, 5:])                   # other positions, lanes and tiles
    assert np.array_equal(bits(frames[60:70], True), full[60:70, 60:70])          # pairs of two tiles in one
    # without the fit the common origin is the first frame's centroid: the same first frame, the same bits
    flat = bits(frames, False)
    assert np.array_equal(bits(frames, False), flat)
    assert np.array_equal(bits(frames[:70], False), flat[:70, :70])


# ---- 5. non-finite frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", [True, False])
@pytest.mark.parametrize("where,value", [(0, np.nan), (3, np.nan), (64, np.nan), (3, np.inf)])
def test_a_non_finite_frame_is_its_row_and_column(sc, where, value, fit):
    frames = rm.case_frames(9, 65).copy()
    frames[where, 4, 1] = value
    w = rm.case_weights(9, True)          # (atom 5 has weight 0, atom 4 has not)
    msd, rmsd = both(sc, frames, w, fit)
    bad = np.zeros((65, 65), dtype=bool)
    bad[where, :] = bad[:, where] = True
    assert np.array_equal(np.isnan(msd), bad) and np.array_equal(np.isnan(rmsd), bad)
    ref = rm.rmsd_matrix(frames, None, w, fit, squared=True)
    rm.compare(msd, rmsd, ref, rm.gate(9, True, fit, rm.scale(frames, None, w, fit)), f"NaN frame {where} fit={fit}")


def test_a_nan_under_a_zero_weight_counts(sc):
    frames = rm.case_frames(9, 65).copy()
    frames[7, 5, 2] = np.nan
    w = rm.case_weights(9, True)
    assert w[5] == 0
    for fit in (True, False):
        msd = both(sc, frames, w, fit)[0]
        bad = np.zeros((65, 65), dtype=bool)
        bad[7, :] = bad[:, 7] = True
        assert np.array_equal(np.isnan(msd), bad)


@pytest.mark.parametrize("fit", [True, False])
def test_a_non_finite_frame_in_other(sc, fit):
    a, b = rm.case_frames(9, 65), rm.case_frames(9, 70)[5:].copy()
    b[64, 0, 0] = np.nan
    a = a.copy()
    a[2, 8, 2] = np.nan
    msd, rmsd = both(sc, a, None, fit, other=b)
    bad = np.zeros((65, 65), dtype=bool)
    bad[2, :] = bad[:, 64] = True
    assert np.array_equal(np.isnan(msd), bad)
    ref = rm.rmsd_matrix(a, b, None, fit, squared=True)
    rm.compare(msd, rmsd, ref, rm.gate(9, False, fit, rm.scale(a, b, None, fit)), f"NaN in other fit={fit}")


# ---- 6. degenerate frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mirror", "collinear"])
def test_degenerate_frames(sc, case):
    frames, w, ref, size = rm.reference(case, False, True)
    msd, rmsd = both(sc, frames, w, True)
    assert np.all(np.isfinite(msd)) and np.all(np.isfinite(rmsd))
    rm.compare(msd, rmsd, ref, rm.gate(case, False, True, size), case)
    if case == "mirror":          # a frame and a mirror image: the proper rotation, far from a fit
        assert rmsd[1, 0] > 1.0 and rmsd[2, 0] < 1.0


# ---- 7. medoid, and consistency with Ensemble.rmsd ------------------------------------------------------------------------------------------
def test_medoid(sc):
    import torch

    frames, w, ref, _ = rm.reference(9, True, True)
    x = frames[:20]
    idx = sc.Ensemble(x, weights=w).medoid()
    assert idx.is_cuda and idx.ndim == 0 and not idx.dtype.is_floating_point
    best = rm.medoid(ref[:20, :20])
    assert int(idx) == best
    assert int(sc.Ensemble(x, weights=w).medoid(fit=False)) == rm.medoid(rm.reference(9, True, False)[2][:20, :20])
    # a NaN frame is skipped: the medoid itself made NaN gives another frame, the model's
    y = x.copy()
    y[best, 0, 0] = np.nan
    got = int(sc.Ensemble(y, weights=w).medoid())
    assert got != best and got == rm.medoid(rm.rmsd_matrix(y, None, w, squared=True))
    # designed ties: two frames (one number twice), and a frame twice (its two rows hold the same bits): the first wins
    assert int(sc.Ensemble(x[:2], weights=w).medoid()) == 0
    tie = np.stack([x[0] + 50.0 * np.arange(9.0)[:, None], x[1], x[1]])
    assert int(sc.Ensemble(tie, weights=w).medoid()) == 1
    assert int(sc.Ensemble(x[:1]).medoid()) == 0
    assert isinstance(idx, torch.Tensor)


@pytest.mark.parametrize("weighted", [False, True])
def test_consistent_with_the_superposition_rmsd(sc, weighted):
    frames, w, _, size = rm.reference(65, weighted, True)
    ens = sc.Ensemble(frames, weights=w)
    matrix = ens.rmsd_matrix().cpu().numpy()
    g_msd = rm.gate(65, weighted, True, size)
    for f in (0, 64, 129):
        fitted = ens.rmsd(reference=f).cpu().numpy()
        extent = float(np.abs(frames[f] - frames[f].mean(axis=0)).max())
        g_fit = em.superpose_gates("weights" if weighted else 65, 65, extent)[2]
        d = np.abs(matrix[:, f] ** 2 - fitted ** 2)
        allowed = g_msd + 2 * fitted * g_fit + g_fit ** 2        # (the two gates, the second one carried over to msd)
        print(f"reference {f} w={weighted}: largest |msd - rmsd^2| / allowed {(d / allowed).max():.3f}")
        assert np.all(d <= allowed)


# ---- 8. the host convenience function ---------------------------------------------------------------------------------------------------------
def test_host_convenience(sc):
    frames, w, ref, _ = rm.reference(9, True, True)
    x = frames[:65]
    got = sc.rmsd_matrix(x, weights=w, squared=True)
    assert isinstance(got, np.ndarray) and got.shape == (65, 65)
    g = rm.gate(9, True, True, rm.scale(x, None, w))
    rm.compare(got, sc.rmsd_matrix(x, weights=w), ref[:65, :65], g, "host function")
    other = sc.rmsd_matrix(x[:3], other=x[:5], weights=w, squared=True)
    assert other.shape == (3, 5)
    rm.compare(other, None, ref[:3, :5], g, "host function, other")
    flat = sc.rmsd_matrix(x[:7], fit=False, squared=True)
    rm.compare(flat, None, rm.reference(9, False, False)[2][:7, :7], rm.gate(9, False, False, rm.scale(x[:7], fit=False)),
               "host function, no fit")
