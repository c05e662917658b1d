"""
GPU checks of the conformational-ensemble feature against the NumPy specification of tests/ensemble_model.py, gated as that
module's docstring says: 8 times the float64 specification's own error against its longdouble evaluation on the same inputs
(the constants recorded there, re-measured by tests/test_ensemble_host.py), with the floor n eps scale.
"""
import functools

import numpy as np
import pytest

from tests import ensemble_model as em
from tests.subspace import (CUTOFF, cov_overlap_interval, cov_weights, np_S, pinv_rows, rmsip_interval, s_bound)

pytestmark = pytest.mark.gpu
EPS = em.EPS
MIRROR = np.array([-1.0, 1.0, 1.0])


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@functools.lru_cache(maxsize=None)
def spec_fit(n_atoms, n_frames, case=None):
    """(target, frames, weights, R, t, fitted, rmsd, scale) of the specification on rotated_ensemble(n_atoms, n_frames): once per shape."""
    fixed, frames = em.rotated_ensemble(n_atoms, n_frames)
    weights = em.atom_weights(n_atoms) if case == "weights" else None
    if case == "mirror":
        frames = frames * MIRROR
    out = (fixed, frames, weights) + em.horn_frames(fixed, frames, weights) + (float(np.abs(fixed - fixed.mean(axis=0)).max()),)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def check_fit(sc, case, n_atoms, got, spec, count):
    """The device's (fitted, rmsd, (R, t)) of the first ``count`` frames against the specification, inside the case's gates."""
    fitted, rmsd, (rot, trans) = got
    _, _, _, s_rot, s_trans, s_fit, s_rmsd, scale = spec
    g_fit, g_rot, g_rmsd = em.superpose_gates(case, n_atoms, scale)
    d_fit, d_rmsd = np.abs(fitted - s_fit[:count]).max(), np.abs(rmsd - s_rmsd[:count]).max()
    d_rot = np.abs(rot - s_rot[:count]).max()
    print(f"{case} N={n_atoms} M={count}: fitted {d_fit:.2e} / {g_fit:.2e}, R {d_rot:.2e} / {g_rot}, rmsd {d_rmsd:.2e} / {g_rmsd:.2e}")
    assert np.all(np.isfinite(fitted)) and np.all(np.isfinite(rot))
    assert d_fit <= g_fit and d_rmsd <= g_rmsd
    if g_rot is not None:
        assert d_rot <= g_rot
        # t = c_target - R c: the centroids' errors and R's, on vectors of the coordinates' size
        assert np.abs(trans - s_trans[:count]).max() <= g_fit + 3 * g_rot * np.abs(spec[1]).max()
    # a proper rotation, to rounding, also where it is not unique
    assert np.abs(np.einsum("fij,fik->fjk", rot, rot) - np.eye(3)).max() <= 16 * EPS
    assert np.abs(np.linalg.det(rot) - 1).max() <= 16 * EPS


# ---- superposition -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames", em.SUPERPOSE_FRAMES)
@pytest.mark.parametrize("n_atoms", em.SUPERPOSE_ATOMS)
def test_superposition_matches_the_specification(sc, n_atoms, n_frames):
    spec = spec_fit(n_atoms, max(em.SUPERPOSE_FRAMES))
    got = sc.superimpose(spec[0], spec[1][:n_frames], return_transform=True)
    check_fit(sc, n_atoms, n_atoms, got, spec, n_frames)


@pytest.mark.parametrize("n_atoms", em.LIMIT_ATOMS)
def test_either_side_of_the_lds_limit(sc, n_atoms, monkeypatch):
    from springcraft_amd import _hip

    monkeypatch.delenv("SPRINGCRAFT_SUPERPOSE_FORM", raising=False)
    assert _hip.lib().sc_superpose_form(n_atoms) == (0 if n_atoms <= em.LDS_LIMIT else 1)
    spec = spec_fit(n_atoms, em.LIMIT_FRAMES)
    check_fit(sc, n_atoms, n_atoms, sc.superimpose(spec[0], spec[1], return_transform=True), spec, em.LIMIT_FRAMES)


@pytest.mark.parametrize("form", ["lds", "stream"])
def test_both_forms_forced_agree_with_the_specification(sc, form, monkeypatch):
    from springcraft_amd import _hip

    monkeypatch.setenv("SPRINGCRAFT_SUPERPOSE_FORM", form)
    assert _hip.lib().sc_superpose_form(257) == (0 if form == "lds" else 1)
    spec = spec_fit(257, max(em.SUPERPOSE_FRAMES))
    check_fit(sc, 257, 257, sc.superimpose(spec[0], spec[1], return_transform=True), spec, max(em.SUPERPOSE_FRAMES))


@pytest.mark.parametrize("n_atoms", [3, 65, 257])
def test_a_moved_copy_of_the_target_comes_back(sc, n_atoms):
    fixed = em.rotated_ensemble(n_atoms, max(em.SUPERPOSE_FRAMES))[0]
    rs = np.random.RandomState(7)
    frames = np.stack([fixed] + [fixed @ em.random_rotation(rs).T + rs.uniform(-3, 3, 3) for _ in range(4)])
    fitted, rmsd = sc.superimpose(fixed, frames)
    g_fit = em.superpose_gates(n_atoms, n_atoms, float(np.abs(fixed - fixed.mean(axis=0)).max()))[0]
    print(f"N={n_atoms}: |fitted - target| {np.abs(fitted - fixed).max():.2e} / {g_fit:.2e}, rmsd {rmsd.max():.2e}")
    assert np.abs(fitted - fixed).max() <= g_fit
    assert rmsd.max() <= np.sqrt(3) * g_fit          # (the RMSD of residuals each inside the gate; frame 0 IS the target)


def test_a_mirror_image_gets_a_proper_rotation(sc):
    spec = spec_fit(65, 3, "mirror")
    got = sc.superimpose(spec[0], spec[1], return_transform=True)
    check_fit(sc, "mirror", 65, got, spec, 3)
    assert np.all(np.linalg.det(got[2][0]) > 0.999)
    kabsch_rmsd = np.array([em.kabsch(spec[0], x)[3] for x in spec[1]])
    g_rmsd = em.superpose_gates("mirror", 65, spec[7])[2]
    assert np.abs(got[1] - kabsch_rmsd).max() <= 2 * g_rmsd and got[1].min() > 1.0     # the corrected-Kabsch RMSD


def test_weights_with_zeros(sc):
    spec = spec_fit(65, 65, "weights")
    check_fit(sc, "weights", 65, sc.superimpose(spec[0], spec[1], weights=spec[2], return_transform=True), spec, 65)


@pytest.mark.parametrize("n_atoms,form", [(65, "auto"), (257, "lds"), (257, "stream")])
def test_a_frames_bits_do_not_depend_on_the_batch(sc, n_atoms, form, monkeypatch):
    monkeypatch.setenv("SPRINGCRAFT_SUPERPOSE_FORM", form)
    fixed, frames = em.rotated_ensemble(n_atoms, 65)
    fit, rmsd, (rot, trans) = sc.superimpose(fixed, frames, return_transform=True)
    for f in (0, 37, 64):
        one = sc.superimpose(fixed, frames[f], return_transform=True)
        assert np.array_equal(one[0], fit[f]) and one[1] == rmsd[f]
        assert np.array_equal(one[2][0], rot[f]) and np.array_equal(one[2][1], trans[f])
    moved = sc.superimpose(fixed, frames[::-1], return_transform=True)      # every frame at another position
    assert np.array_equal(moved[0][::-1], fit) and np.array_equal(moved[1][::-1], rmsd)
    assert np.array_equal(moved[2][0][::-1], rot) and np.array_equal(moved[2][1][::-1], trans)


@pytest.mark.parametrize("form", ["lds", "stream"])
def test_a_nan_frame_poisons_only_itself(sc, form, monkeypatch):
    monkeypatch.setenv("SPRINGCRAFT_SUPERPOSE_FORM", form)
    fixed, frames = em.rotated_ensemble(65, 3)
    clean = sc.superimpose(fixed, frames, return_transform=True)
    bad = frames.copy()
    bad[1, 40, 2] = np.nan
    fit, rmsd, (rot, trans) = sc.superimpose(fixed, bad, return_transform=True)
    assert np.all(np.isnan(fit[1])) and np.isnan(rmsd[1]) and np.all(np.isnan(rot[1])) and np.all(np.isnan(trans[1]))
    for f in (0, 2):
        assert np.array_equal(fit[f], clean[0][f]) and rmsd[f] == clean[1][f] and np.array_equal(rot[f], clean[2][0][f])


# ---- mean frame, MSD, iterative fitting ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames,n_atoms", [(1, 7), (3, 65), (65, 65), (130, 7)])
def test_mean_and_rmsf_agree_with_numpy(sc, n_frames, n_atoms):
    frames = em.perturbed_ensemble(n_atoms, n_frames)
    ens, again = sc.Ensemble(frames), sc.Ensemble(frames)
    mean, rmsf = ens.mean().cpu().numpy(), ens.rmsf().cpu().numpy()
    assert np.array_equal(mean, again.mean().cpu().numpy()) and np.array_equal(rmsf, again.rmsf().cpu().numpy())
    # a mean of M numbers of size <= s: sequential and pairwise sums are each within M u s of the truth, M eps s apart
    s = np.abs(frames).max()
    ref_mean = frames.mean(axis=0)
    assert np.abs(mean - ref_mean).max() <= n_frames * EPS * s
    # |x - mean| carries the mean's error and one rounding of the coordinates, (M + 1) eps s at most; the squares of d <= dmax
    # move by 2 dmax times that, and their sum of 3 M terms adds 3 M eps dmax^2
    dev2 = ((frames - ref_mean) ** 2).sum(axis=2)
    dmax = np.sqrt(dev2.max())
    ref_msd = dev2.sum(axis=0) / max(n_frames - 1, 1)
    bound = (2 * dmax * (n_frames + 1) * EPS * s + 3 * n_frames * EPS * dmax ** 2) * n_frames / max(n_frames - 1, 1)
    print(f"M={n_frames} N={n_atoms}: mean {np.abs(mean - ref_mean).max():.2e}, msd {np.abs(rmsf ** 2 - ref_msd).max():.2e} / {bound:.2e}")
    assert np.abs(rmsf ** 2 - ref_msd).max() <= bound + 4 * EPS * ref_msd.max()
    assert np.array_equal(ens.deviations().cpu().numpy(), frames - mean)


def test_iterative_fitting_follows_the_specification(sc):
    frames = em.perturbed_ensemble(65, 9)
    fitted, mean, passes, converged = em.iterative_fit(frames, tol=1e-4)
    ens = sc.Ensemble(frames)
    assert ens.superpose(tol=1e-4) == (passes, True) and converged
    g = em.gate(em.SPEC_ERR_ITER_MEAN, 65, float(np.abs(mean - mean.mean(axis=0)).max()))
    got = ens.mean().cpu().numpy()
    print(f"iterative: {passes} passes, |mean - spec| {np.abs(got - mean).max():.2e} / {g:.2e}")
    assert np.abs(got - mean).max() <= g
    per_pass = em.superpose_gates(65, 65, float(np.abs(mean - mean.mean(axis=0)).max()))[0]
    assert np.abs(ens.frames.cpu().numpy() - fitted).max() <= passes * per_pass    # (every pass's fit inside its gate)
    assert sc.Ensemble(frames).superpose(max_iter=1) == (1, False)       # out of passes: reported, not raised
    # a frame or a structure as the reference: one pass; rmsd() fits in a temporary and moves nothing
    one = sc.Ensemble(frames)
    assert one.superpose(reference=3) == (1, True)
    spec = em.horn_frames(frames[3], frames)
    g_fit, _, g_rmsd = em.superpose_gates(65, 65, float(np.abs(frames[3] - frames[3].mean(axis=0)).max()))
    assert np.abs(one.frames.cpu().numpy() - spec[2]).max() <= g_fit
    assert np.abs(one.fit_rmsd.cpu().numpy() - spec[3]).max() <= g_rmsd
    other = sc.Ensemble(frames)
    assert np.abs(other.rmsd(reference=frames[3]).cpu().numpy() - spec[3]).max() <= g_rmsd
    assert np.array_equal(other.frames.cpu().numpy(), frames)
    with pytest.raises(IndexError):
        other.superpose(reference=9)


# ---- PCA ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames,n_atoms", em.PCA_CASES)
def test_pca_of_the_designed_spectrum(sc, torch, n_frames, n_atoms):
    frames, var, _ = em.designed_ensemble(n_frames, n_atoms)
    k = len(var)
    ens = sc.Ensemble(frames)
    ed = ens.pca(k)
    w, v = (t.cpu().numpy() for t in ed.finish())
    assert w.shape == (1, k) and v.shape == (1, k, 3 * n_atoms) and ed._first_row == 6 and ed.subset == (6, 5 + k)
    got_var = ed.variances.cpu().numpy()
    s_var, s_comp, s_total = em.pca(frames, k)
    g_var, g_comp = em.pca_gates(("designed", n_frames, n_atoms), n_frames, n_atoms, float(s_var[0]))
    lapack = np.linalg.eigvalsh(em.covariance(frames))[::-1][:k]
    cos = np.abs((v[0] * s_comp).sum(axis=1))
    n = max(n_frames, 3 * n_atoms)
    # orthogonality: the eigenvectors' own (n eps) and, on the Gram route, the residual n eps mu_1 of the small problem
    # divided by sqrt(mu_i mu_j) >= mu_k when the rows are expanded and normalised
    g_orth = em.GATE_MULTIPLE * n * EPS * s_var[0] / s_var[-1]
    orth = np.abs(v[0] @ v[0].T - np.eye(k)).max()
    print(f"M={n_frames} N={n_atoms}: var {np.abs(got_var - lapack).max():.2e} / {g_var:.2e}, 1 - |cos| {(1 - cos).max():.2e} / "
          f"{g_comp:.2e}, orthonormality {orth:.2e} / {g_orth:.2e}")
    assert np.all(np.diff(got_var) < 0) and np.all(np.diff(w[0]) > 0) and np.array_equal(w[0], 1.0 / got_var)
    assert np.abs(got_var - lapack).max() <= g_var and np.abs(got_var - s_var).max() <= g_var
    assert np.all(cos >= 1 - g_comp)
    assert orth <= g_orth
    total = float(ed.total_variance)
    assert abs(total - s_total) <= em.GATE_MULTIPLE * n * EPS * s_total
    ratio = ed.explained_variance_ratio.cpu().numpy()
    assert abs(ratio.sum() - 1) <= em.GATE_MULTIPLE * n * EPS          # all the components this ensemble has
    if k > 2:
        part = ens.pca(k - 2)
        part.finish()
        r = part.explained_variance_ratio.cpu().numpy()
        assert r.sum() < 1 and np.abs(r - ratio[:k - 2]).max() <= 2 * g_var / total


@pytest.mark.parametrize("n_frames,n_atoms", [(5, 7), (65, 64)])
def test_closure_msf_of_all_components_is_the_rmsf_squared(sc, n_frames, n_atoms):
    ens = sc.Ensemble(em.perturbed_ensemble(n_atoms, n_frames))
    assert ens.superpose()[1]
    fitted = ens.frames.cpu().numpy()
    k = n_frames - 1
    ed = ens.pca(k)
    ed.finish()
    got_var = ed.variances.cpu().numpy()
    g_var = em.pca_gates(("perturbed", n_frames, n_atoms), n_frames, n_atoms, float(got_var[0]))[0]
    lapack = np.linalg.eigvalsh(em.covariance(fitted))[::-1][:k]
    assert np.abs(got_var - lapack).max() <= g_var
    total = float(ed.total_variance)
    n = max(n_frames, 3 * n_atoms)
    # every entry of the covariance, by the frames or by the modes, is a sum of n terms bounded by the trace
    g = em.GATE_MULTIPLE * n * EPS * total
    msf, rmsf = ed.mean_square_fluctuation().cpu().numpy(), ens.rmsf().cpu().numpy()
    print(f"M={n_frames} N={n_atoms}: |msf - rmsf^2| {np.abs(msf[0] - rmsf ** 2).max():.2e} / {g:.2e}")
    assert msf.shape == (1, n_atoms) and np.abs(msf[0] - rmsf ** 2).max() <= g
    assert abs(float(ed.explained_variance_ratio.sum()) - 1) <= em.GATE_MULTIPLE * n * EPS
    v = ed.v.cpu().numpy()[0]
    assert np.abs(v @ v.T - np.eye(k)).max() <= em.GATE_MULTIPLE * n * EPS * got_var[0] / got_var[-1]


def test_pca_with_masses(sc):
    fitted = em.iterative_fit(em.perturbed_ensemble(7, 40))[0]
    masses = 1.0 + np.arange(7.0)
    ed = sc.Ensemble(fitted).pca(15, masses=masses)
    ed.finish()
    s_var, _, s_total = em.pca(fitted, 15, masses=masses)
    g_var = em.pca_gates(("masses", 40, 7), 40, 7, float(s_var[0]))[0]
    got = ed.variances.cpu().numpy()
    print(f"masses: var {np.abs(got - s_var).max():.2e} / {g_var:.2e}")
    assert np.abs(got - s_var).max() <= g_var and abs(float(ed.total_variance) - s_total) <= 8 * 40 * EPS * s_total
    assert np.array_equal(ed.inv_sqrt_mass.cpu().numpy(), (1.0 / np.sqrt(masses))[None, :])


def test_pca_argument_and_rank_checks(sc):
    frames = em.perturbed_ensemble(7, 5)
    ens = sc.Ensemble(frames)
    with pytest.raises(ValueError, match="n_modes 5 outside 1..4"):
        ens.pca(5)
    with pytest.raises(ValueError, match="n_modes"):
        sc.Ensemble(em.perturbed_ensemble(3, 9)).pca(4)            # 3 N - 6 = 3
    with pytest.raises(IndexError):
        ens.pca(2, masses=np.ones(6))
    # three distinct frames, each twice: the centred frames have rank 2
    dup = sc.Ensemble(np.concatenate([frames[:3], frames[:3]]))
    ed = dup.pca(4)
    with pytest.raises(ValueError, match="only 2 of the 4 selected components"):
        ed.finish()


# ---- as a mode source ------------------------------------------------------------------------------------------------------------
def test_enm_against_the_ensemble(sc, torch):
    from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver

    n_atoms, n_frames, k = 24, 30, 12
    ens = sc.Ensemble(em.perturbed_ensemble(n_atoms, n_frames))
    assert ens.superpose()[1]
    ed = ens.pca(k)
    wb, vb = (t.cpu().numpy()[0] for t in ed.finish())
    anm = DeviceBatchSolver(n_atoms, 1, sc.InvariantForceField(CUTOFF))
    anm.solve(ens.mean()[None].contiguous())
    wa, va = (t.cpu().numpy()[0] for t in anm.finish())
    m = 3 * n_atoms

    rows_a, rows_b = np.arange(6, 16), np.arange(10)
    model = np_S(va, vb, rows_a, rows_b, np.ones(10), np.ones(10))
    lo, hi = rmsip_interval(model, 10.0, 10.0, s_bound(m, 10.0, 10.0))
    got = float(anm.rmsip(other=ed)[0, 0])
    print(f"rmsip(ANM, ensemble) = {got:.6f} in [{lo:.6f}, {hi:.6f}]")
    assert lo <= got <= hi and lo <= float(ed.rmsip(other=anm)[0, 0]) <= hi

    rows_a, rows_b = pinv_rows(wa), np.arange(k)
    pa, pb = cov_weights(wa, rows_a), cov_weights(wb, rows_b)
    Ta, Tb = (pa ** 2).sum(), (pb ** 2).sum()
    model = np_S(va, vb, rows_a, rows_b, pa, pb)
    lo, hi = cov_overlap_interval(model, Ta, Tb, s_bound(m, pa.sum(), pb.sum()), max(len(rows_a), k))
    got = float(anm.covariance_overlap(other=ed)[0, 0])
    print(f"covariance_overlap(ANM, ensemble) = {got:.6f} in [{lo:.6f}, {hi:.6f}]")
    assert lo <= got <= hi

    table = ed.mode_overlap_matrix([(0, 0)], [6, 7, 8], other=anm).cpu().numpy()[0]
    assert np.abs(table - vb[:3] @ va[6:9].T).max() <= 2 * m * EPS

    dev = ens.deviations()[:4][None].contiguous()
    ov = ed.overlap(dev).cpu().numpy()[0]
    d = dev.cpu().numpy()[0].reshape(4, m)
    ref = (d @ vb.T) / np.linalg.norm(d, axis=1)[:, None] / np.linalg.norm(vb, axis=1)[None, :]
    assert ov.shape == (4, k) and np.abs(ov - ref).max() <= 2 * m * EPS

    with pytest.raises(ValueError, match="uniform batch solver"):
        ed.rmsip(other=RaggedBatchSolver([n_atoms], sc.InvariantForceField(CUTOFF)))
    with pytest.raises(ValueError, match="no common coordinates"):
        ed.rmsip(other=DeviceBatchSolver(n_atoms + 1, 1, sc.InvariantForceField(CUTOFF)))
    with pytest.raises(ValueError, match="Trivial modes"):
        ed.mean_square_fluctuation(mode_subset=[5])
