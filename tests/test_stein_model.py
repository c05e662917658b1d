"""
CPU check of the partial-spectrum eigenvector algorithm of stein.hip (tools/models/stein_model.py restates k_stein and
CholQR2 in NumPy; tests/test_partial_spectrum_gpu.py checks the kernels) on the cluster cases of the GPU tests, against
LAPACK: glued Wilkinson matrices and tridiagonal reductions of Q diag(lambda) Q^T with exact and close multiplicities,
ranges that hold whole clusters and ranges that cut them.  Gates as on the GPU; the figures are printed.  The model also
shows what the kernel does not report: the Cholesky of the first CholQR round never reaches k_chol_inv's clamp on these
cases, and the second round is what makes the set orthonormal.
"""
import numpy as np
import pytest

from tests.util import clustered_spectrum, glued_wilkinson, random_orthogonal, subspace_error, tridiagonal
from tools.models import stein_model as sm

TOL_RES, TOL_ORTH = 1e-10, 1e-10


def _solve(d, e, lo, hi, **kw):
    """The model's vectors for LAPACK's eigenvalues lo..hi of (d, e) and the figures of every gate."""
    from scipy.linalg import eigh_tridiagonal

    t = tridiagonal(d, e)
    w_ref, v_ref = np.linalg.eigh(t)
    scale = np.abs(w_ref).max()
    w = eigh_tridiagonal(d, e, eigvals_only=True, select="i", select_range=(lo, hi))
    q, diag = sm.eigenvectors(d, e, w, **kw)
    r = t @ q - q * w[None, :]
    out = {"res": float(np.linalg.norm(r, axis=0).max() / scale),
           "orth": float(np.abs(q.T @ q - np.eye(len(w))).max())}
    out["sub"], out["sub_bound"], _ = subspace_error(t, w_ref, v_ref, lo, hi, q.T, np.linalg.norm(r))
    out.update(diag)
    return out


def _check(label, out):
    print(f"{label}: res {out['res']:.1e}, orth {out['orth']:.1e}, sub {out['sub']:.1e} (bound {out['sub_bound']:.1e}), "
          f"replaced pivots {out['replaced_pivots']}, Cholesky pivots {out['chol_min_pivot'][0]:.1e} / "
          f"{out['chol_min_pivot'][1]:.1e} of the largest")
    assert out["res"] <= TOL_RES and out["orth"] <= TOL_ORTH, (label, out)
    assert out["sub"] <= out["sub_bound"], (label, out)
    assert out["chol_min_pivot"][0] > 1e-14, (label, out)        # far from k_chol_inv's clamp (1e-300)


@pytest.mark.parametrize("glue", [1e-4, 1e-8, 1e-12, 1e-14])
@pytest.mark.parametrize("lo,hi", [(272, 335), (304, 335), (290, 320), (316, 335), (310, 310), (0, 40)])
def test_glued_wilkinson(glue, lo, hi):
    d, e = glued_wilkinson(16, glue)
    _check(f"W21 glue {glue:g} [{lo}, {hi}]", _solve(d, e, lo, hi))


@pytest.mark.parametrize("rel_spacing", [0.0, 1e-13, 1e-10, 1e-7])
def test_reduced_clustered_spectrum(rel_spacing):
    """The tridiagonal form (Householder, scipy's hessenberg) of Q diag(lambda) Q^T; lo / hi inside clusters."""
    from scipy.linalg import hessenberg

    n = 300
    lam = clustered_spectrum(rel_spacing, seed=2, n=n)
    q = random_orthogonal(8, n)
    a = (q * lam[None, :]) @ q.T
    h = hessenberg(0.5 * (a + a.T))
    d, e = np.diag(h).copy(), np.diag(h, -1).copy()
    starts = np.concatenate([[0], np.where(np.diff(lam) > 1e-3 * np.abs(lam).max())[0] + 1])
    sizes = np.diff(np.concatenate([starts, [n]]))
    big = [int(s0) for s0, sz in zip(starts, sizes) if sz >= 8]
    for lo, hi in [(big[0], big[0] + 11), (big[0] + 3, big[1] + 4), (big[2] + 1, big[2] + 1)]:
        _check(f"clusters spacing {rel_spacing:g} [{lo}, {hi}]", _solve(d, e, lo, hi))


def test_decoupled_identical_blocks():
    """Exact multiplicities from exactly decoupled blocks (e = 0), as a lattice Hessian's reduction produces them."""
    d = np.tile([2.0, 2.0, 2.0, 2.0, 1.5], 30)
    e = np.tile([1.0, 1.0, 0.7, 1.0, 0.0], 30)[:-1]
    _check("identical blocks [0, 59]", _solve(d, e, 0, 59))
    _check("identical blocks [20, 95]", _solve(d, e, 20, 95))


def test_second_cholqr_round_is_needed():
    """One CholQR round leaves the glued W21 (glue 1e-12) set visibly non-orthogonal: the second round is not decoration.
    The range 200..335 was chosen to keep the threshold of 1e-9: with every shift kept 10 eps |T| above the one before it,
    the top 64 alone (272..335, the range this test used under the former shift rule) come to 1.2e-11 after one round."""
    d, e = glued_wilkinson(16, 1e-12)
    once = _solve(d, e, 200, 335, rounds=1)
    twice = _solve(d, e, 200, 335)
    print(f"orthogonality after one round {once['orth']:.1e}, after two {twice['orth']:.1e}")
    assert once["orth"] > 1e-9 and twice["orth"] <= 1e-14


def test_hash_start_vectors():
    """hash_unit: uniform in [-0.5, 0.5), different for every vector and row."""
    x = sm.hash_unit(np.arange(64)[None, :] + 1, np.arange(1000)[:, None] + 1)
    assert x.min() >= -0.5 and x.max() < 0.5 and abs(x.mean()) < 0.01
    assert len(np.unique(x)) == x.size
    g = x.T @ x / 1000.0
    assert np.abs(g - np.diag(np.diag(g))).max() < 0.02          # nearly orthogonal start vectors


def test_run_shift_stays_inside_the_run():
    """Every shift is at least 10 eps |T| above the one before it: 64 equal values end up 10 eps |T| apart and move by
    < 640 eps |T|; the eigenvalues on either side of the run stay where they are."""
    tiny = sm.EPS * 3.0
    w = np.concatenate([[-1.0], np.full(64, 0.5), [0.75]])
    lam = sm.shifts(w, tiny)
    assert lam[0] == -1.0 and lam[-1] == 0.75
    assert np.array_equal(lam[1:65], 0.5 + np.arange(64) * 10.0 * tiny)
