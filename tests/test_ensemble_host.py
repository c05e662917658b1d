"""
CPU checks of the conformational-ensemble feature: the NumPy specification (tests/ensemble_model.py) against known facts,
the form-switch policy, every host-side argument check of springcraft_amd.ensemble, the specification's own float64 error
against its longdouble evaluation on the inputs of tests/test_ensemble_gpu.py (the recorded gates), and the pure host logic
under sanitizers.
"""
import os
import shutil
import subprocess
from os.path import dirname, join

import numpy as np
import pytest

from springcraft_amd import _hip, ensemble as ens_mod
from tests import ensemble_model as em

ROOT = dirname(dirname(__file__))


# ---- the specification against known facts ---------------------------------------------------------------------------------------
def test_known_transform_recovered():
    rs = np.random.RandomState(1)
    x = rs.randn(40, 3) * 5
    rot, shift = em.random_rotation(rs), np.array([3.0, -7.0, 11.0])
    y = x @ rot.T + shift
    for fit in (em.kabsch, em.horn):
        r, t, fitted, rmsd = fit(y, x)
        assert np.abs(r - rot).max() < 1e-13 and np.abs(t - shift).max() < 1e-12
        assert np.abs(fitted - y).max() < 1e-12 and rmsd < 1e-13


@pytest.mark.parametrize("weighted", [False, True])
def test_kabsch_and_horn_agree(weighted):
    fixed, frames = em.rotated_ensemble(65, 3)
    w = em.atom_weights(65) if weighted else None
    for x in frames:
        a, b = em.kabsch(fixed, x, w), em.horn(fixed, x, w)
        assert np.abs(a[0] - b[0]).max() < 1e-13 and np.abs(a[2] - b[2]).max() < 1e-12 and abs(a[3] - b[3]) < 1e-13
        assert abs(np.linalg.det(b[0]) - 1) < 1e-14 and np.abs(b[0].T @ b[0] - np.eye(3)).max() < 1e-14


def test_mirror_image_gets_a_proper_rotation():
    fixed, frames = em.rotated_ensemble(65, 3)
    for x in frames * np.array([-1.0, 1.0, 1.0]):
        a, b = em.kabsch(fixed, x), em.horn(fixed, x)
        assert abs(np.linalg.det(b[0]) - 1) < 1e-14
        assert abs(a[3] - b[3]) < 1e-12 * a[3] and a[3] > 1.0     # the corrected-Kabsch RMSD, far from a fit
        # the uncorrected SVD solution would be a reflection with a smaller RMSD
        c, ct = x.mean(axis=0), fixed.mean(axis=0)
        u, _, vt = np.linalg.svd((x - c).T @ (fixed - ct))
        improper = vt.T @ u.T
        assert np.linalg.det(improper) < 0
        assert np.sqrt((((x - c) @ improper.T + ct - fixed) ** 2).sum(axis=1).mean()) < b[3]


@pytest.mark.parametrize("kind", ["one", "two", "collinear", "planar"])
def test_degenerate_frames_stay_finite(kind):
    rs = np.random.RandomState(5)
    if kind == "one":
        x = rs.randn(1, 3)
    elif kind == "two":
        x = rs.randn(2, 3)
    elif kind == "collinear":
        x = np.outer(np.arange(6.0), [1.0, 2.0, -1.0]) + 0.5
    else:
        x = np.c_[rs.randn(8, 2), np.zeros(8)]
    y = x @ em.random_rotation(rs).T + 1.0
    r, t, fitted, rmsd = em.horn(y, x)
    assert np.all(np.isfinite(r)) and np.all(np.isfinite(fitted)) and np.isfinite(rmsd)
    assert np.abs(r.T @ r - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(r) - 1) < 1e-14
    assert rmsd <= em.kabsch(y, x)[3] + 1e-12          # a minimiser


def test_jacobi_against_lapack():
    rs = np.random.RandomState(2)
    a = rs.randn(9, 9)
    a = a + a.T
    lam, v = em.jacobi_eigh(a)
    assert np.abs(np.sort(lam) - np.linalg.eigvalsh(a)).max() < 1e-13
    assert np.abs(a @ v - v * lam).max() < 1e-13 and np.abs(v.T @ v - np.eye(9)).max() < 1e-14


@pytest.mark.parametrize("m,n", em.PCA_CASES)
def test_gram_and_covariance_routes_agree(m, n):
    frames, var, comp = em.designed_ensemble(m, n)
    k = len(var)
    a, b = em.pca(frames, k, route="gram"), em.pca(frames, k, route="cov")
    assert np.abs(a[0] - b[0]).max() < 1e-14 and np.abs(a[0] - var).max() < 1e-14
    assert (1 - np.abs((a[1] * b[1]).sum(axis=1))).max() < 1e-12       # the same components up to sign
    assert (1 - np.abs((a[1] * comp).sum(axis=1))).max() < 1e-12
    assert abs(a[2] - var.sum()) < 1e-14 and abs(a[2] - b[2]) < 1e-15
    assert np.abs(a[0] - np.linalg.eigvalsh(em.covariance(frames))[::-1][:k]).max() < 1e-14
    # the designed components are orthogonal to the rigid-body fields of the mean structure
    assert np.abs(em.rigid_body_fields(frames.mean(axis=0)) @ comp.T).max() < 1e-11


def test_iterative_fit_converges():
    frames = em.perturbed_ensemble(65, 9)
    fitted, mean, passes, converged = em.iterative_fit(frames)
    assert converged and 2 <= passes < 10
    assert np.abs(fitted.mean(axis=0) - mean).max() < 1e-13
    assert em.iterative_fit(frames, max_iter=1)[2:] == (1, False)


# ---- the recorded gates: float64 specification against its longdouble evaluation on the GPU tests' inputs ---------------------------------
def _within(measured, recorded):
    return all(r is None or m <= r for m, r in zip(measured, recorded))


@pytest.mark.parametrize("n", em.SUPERPOSE_ATOMS + em.LIMIT_ATOMS)
def test_superposition_gates(n):
    fixed, frames = em.rotated_ensemble(n, em.LIMIT_FRAMES if n in em.LIMIT_ATOMS else max(em.SUPERPOSE_FRAMES))
    measured = em.superpose_errors(fixed, frames)
    print(n, measured)
    assert _within(measured[:3], em.SPEC_ERR_SUPERPOSE[n])


def test_superposition_gates_weights_and_mirror():
    fixed, frames = em.rotated_ensemble(65, 65)
    assert _within(em.superpose_errors(fixed, frames, em.atom_weights(65))[:3], em.SPEC_ERR_SUPERPOSE["weights"])
    assert _within(em.superpose_errors(fixed, frames[:3] * np.array([-1.0, 1.0, 1.0]))[:3], em.SPEC_ERR_SUPERPOSE["mirror"])


@pytest.mark.parametrize("m,n", em.PCA_CASES)
def test_pca_gates(m, n):
    frames, var, _ = em.designed_ensemble(m, n)
    assert _within(em.pca_errors(frames, len(var))[:2], em.SPEC_ERR_PCA[("designed", m, n)])
    fitted = em.iterative_fit(em.perturbed_ensemble(n, m))[0]
    assert _within(em.pca_errors(fitted, ens_mod.max_components(m, n))[:2], em.SPEC_ERR_PCA[("perturbed", m, n)])


def test_pca_gate_masses_and_iterative_mean():
    fitted = em.iterative_fit(em.perturbed_ensemble(7, 40))[0]
    assert _within(em.pca_errors(fitted, 15, masses=1.0 + np.arange(7.0))[:2], em.SPEC_ERR_PCA[("masses", 40, 7)])
    frames = em.perturbed_ensemble(65, 9)
    a, b = em.iterative_fit(frames), em.iterative_fit(frames, dtype=np.longdouble)
    assert a[2:] == b[2:]
    assert float(np.abs(a[1] - b[1]).max()) <= em.SPEC_ERR_ITER_MEAN


# ---- the form-switch policy --------------------------------------------------------------------------------------------------------
def test_superpose_form_policy(monkeypatch):
    form = _hip.lib().sc_superpose_form
    monkeypatch.delenv("SPRINGCRAFT_SUPERPOSE_FORM", raising=False)
    assert [form(n) for n in (1, 257, 2000, em.LDS_LIMIT, em.LDS_LIMIT + 1, 50000)] == [0, 0, 0, 0, 1, 1]
    monkeypatch.setenv("SPRINGCRAFT_SUPERPOSE_FORM", "stream")
    assert [form(n) for n in (1, 257, em.LDS_LIMIT + 1)] == [1, 1, 1]
    monkeypatch.setenv("SPRINGCRAFT_SUPERPOSE_FORM", "lds")        # never beyond what fits
    assert [form(n) for n in (257, em.LDS_LIMIT, em.LDS_LIMIT + 1)] == [0, 0, 1]
    monkeypatch.setenv("SPRINGCRAFT_SUPERPOSE_FORM", "auto")
    assert [form(n) for n in (257, em.LDS_LIMIT + 1)] == [0, 1]


# ---- host-side argument checks: all raise before any device call (there is no device here) ---------------------------------------------
def test_ensemble_argument_checks():
    sc = pytest.importorskip("springcraft_amd")
    good = np.zeros((4, 5, 3))
    for bad in (np.zeros((4, 5)), np.zeros((4, 5, 2)), np.zeros((4, 3))):
        with pytest.raises(ValueError, match="shape"):
            sc.Ensemble(bad)
    with pytest.raises(ValueError, match="at least one frame"):
        sc.Ensemble(np.zeros((0, 5, 3)))
    with pytest.raises(ValueError, match="at least one atom"):
        sc.Ensemble(np.zeros((4, 0, 3)))
    with pytest.raises(IndexError, match="weights for 5 atoms"):
        sc.Ensemble(good, weights=np.ones(4))
    with pytest.raises(ValueError, match="not negative"):
        sc.Ensemble(good, weights=[1, 1, -1, 1, 1])
    with pytest.raises(ValueError, match="not negative"):
        sc.Ensemble(good, weights=[1, 1, np.nan, 1, 1])
    with pytest.raises(ValueError, match="positive sum"):
        sc.Ensemble(good, weights=np.zeros(5))
    import torch

    with pytest.raises(ValueError, match="CUDA float64 tensor"):
        sc.Ensemble(torch.zeros((4, 5, 3), dtype=torch.float64))          # a host tensor: not on a device


def test_helper_argument_checks():
    with pytest.raises(IndexError, match="out of bounds"):
        ens_mod._checked_reference(4, 4, 5)
    with pytest.raises(IndexError, match="out of bounds"):
        ens_mod._checked_reference(-5, 4, 5)
    assert ens_mod._checked_reference(-1, 4, 5) == 3 and ens_mod._checked_reference(None, 4, 5) is None
    with pytest.raises(ValueError, match=r"shape \(5, 3\)"):
        ens_mod._checked_reference(np.zeros((4, 3)), 4, 5)
    assert ens_mod._checked_reference(np.zeros((5, 3)), 4, 5).shape == (5, 3)
    assert ens_mod.max_components(5, 7) == 4 and ens_mod.max_components(40, 7) == 15 and ens_mod.max_components(1, 7) == 0
    for bad in (0, 5, 16):
        with pytest.raises(ValueError, match="n_modes"):
            ens_mod._checked_n_modes(bad, 5 if bad != 16 else 40, 7)
    assert ens_mod._checked_n_modes(15, 40, 7) == 15
    with pytest.raises(IndexError, match="masses for 7 atoms"):
        ens_mod._checked_masses(np.ones(6), 7)
    with pytest.raises(ValueError, match="positive"):
        ens_mod._checked_masses(np.zeros(7), 7)


def test_superimpose_argument_checks():
    import springcraft_amd as sc

    with pytest.raises(ValueError, match=r"shape \(N, 3\)"):
        sc.superimpose(np.zeros((5, 2)), np.zeros((5, 3)))
    with pytest.raises(ValueError, match="atoms"):
        sc.superimpose(np.zeros((5, 3)), np.zeros((2, 4, 3)))
    with pytest.raises(ValueError, match="shape"):
        sc.superimpose(np.zeros((5, 3)), np.zeros((2, 2, 5, 3)))
    with pytest.raises(IndexError, match="weights"):
        sc.superimpose(np.zeros((5, 3)), np.zeros((5, 3)), weights=np.ones(3))


def test_rank_check_names_the_usable_components():
    ens_mod.rank_check(np.array([1.0, 0.5, 1e-3]), 10, 4)
    with pytest.raises(ValueError, match="only 2 of the 4 selected components"):
        ens_mod.rank_check(np.array([1.0, 0.5, 1e-16, -1e-17]), 10, 4)
    with pytest.raises(np.linalg.LinAlgError):
        ens_mod.rank_check(np.array([np.nan, 0.5]), 10, 4)


# ---- pure host logic (form policy, scratch sizes, PCA plan) under sanitizers --------------------------------------------------------------
def test_ensemble_logic_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_ensemble_logic")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", join(ROOT, "include"), "-I", join(ROOT, "springcraft_amd", "csrc"),
           join(ROOT, "tests", "host_sanitize", "test_ensemble_logic.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower()) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if k != "SPRINGCRAFT_SUPERPOSE_FORM"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ensemble logic ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
