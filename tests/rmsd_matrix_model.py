"""
What tests/test_rmsd_matrix_host.py and tests/test_rmsd_matrix_gpu.py share: the NumPy specification of the pairwise
least-squares RMSD matrix, its inputs and its gates.

Specification.  Atom weights w >= 0 (1 if none), W = sum w.  Per frame c_f = sum w x_f / W, y_f = x_f - c_f, G_f = sum_a w_a
|y_f[a]|^2.  Per pair S = sum_a w_a y_f[a] y_g[a]^T, lambda the largest eigenvalue of Horn's 4 x 4 matrix N(S) by
``ensemble_model.jacobi_eigh`` (so the whole runs in float64 and in ``np.longdouble``),

    msd(f, g) = max(0, (G_f + G_g) - 2 lambda) / W,     rmsd = sqrt(msd).

``fit=False``: y_f = x_f - o with o the weighted centroid of the first frame of the first ensemble (0 where that is not
finite: the frame is NaN anyway and the others keep their values), and lambda = tr S.  A self-comparison computes the pairs
f > g, mirrors them and sets the diagonal to 0; a frame whose G is not finite gives a NaN row and column, diagonal included.

Gates.  Comparisons are made in msd, where the cancellation (G_f + G_g) - 2 lambda is linear: every term is of the size
``scale = max_f G_f / W`` and carries a rounding error proportional to it, whatever the difference comes to.  The gate follows
``ensemble_model.gate``: ``max(GATE_MULTIPLE x the model's own error, N EPS scale)``, the model's own error being the largest
|float64 - longdouble| of msd on the first MODEL_FRAMES frames of the case's input, recorded below and re-measured by the host
test.  rmsd = sqrt(msd) is compared only where msd exceeds RMSD_FLOOR gates: there d sqrt(msd) = d msd / (2 sqrt(msd)) to
first order with a relative second-order term below 1e-4, and ``gate / sqrt(msd)`` leaves a factor of two for it and for the
root's own rounding.  Below that floor the root of a difference that is mostly rounding has no digits to compare.
"""
import functools

import numpy as np

from tests import ensemble_model as em

EPS = em.EPS
RMSD_FLOOR = 1e4
# the GPU cases: frame counts around the 64-frame tile (a diagonal tile, a partial one, an off-diagonal one) and atom
# counts around the staged group of 8 atoms and its multiples
FRAMES = (1, 2, 3, 63, 64, 65, 130)
ATOMS = (1, 2, 3, 7, 8, 9, 65, 257)
MAX_FRAMES = max(FRAMES)
MODEL_FRAMES = 32          # the model's own error is measured on the first frames of a case's input
MIRROR = np.array([-1.0, 1.0, 1.0])


# ---- the specification ----------------------------------------------------------------------------------------------------------
def _horn_matrix(s, dtype):
    (sxx, sxy, sxz), (syx, syy, syz), (szx, szy, szz) = s
    return np.array([[sxx + syy + szz, syz - szy, szx - sxz, sxy - syx],
                     [syz - szy, sxx - syy - szz, sxy + syx, szx + sxz],
                     [szx - sxz, sxy + syx, syy - sxx - szz, syz + szy],
                     [sxy - syx, szx + sxz, syz + szy, szz - sxx - syy]], dtype=dtype)


def _origin(first, w):
    o = (w[:, None] * first).sum(axis=0) / w.sum()
    return o if np.all(np.isfinite(o)) else np.zeros(3, dtype=first.dtype)


def _centred(frames, w, origin):
    """(y (M, N, 3), G (M,)): the frames about their own weighted centroids (origin None) or about ``origin``."""
    with np.errstate(invalid="ignore", over="ignore"):
        c = (w[None, :, None] * frames).sum(axis=1) / w.sum() if origin is None else origin[None, :]
        y = frames - c[:, None, :]
        return y, (w[None, :] * (y * y).sum(axis=2)).sum(axis=1)


def moments(frames_a, frames_b=None, weights=None, fit=True, dtype=np.float64):
    """``(G_a, G_b or None, W)`` of the definition (``fit=False``: about the common origin)."""
    a = np.asarray(frames_a, dtype=dtype)
    w = np.ones(a.shape[1], dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype)
    origin = None if fit else _origin(a[0], w)
    ga = _centred(a, w, origin)[1]
    gb = None if frames_b is None else _centred(np.asarray(frames_b, dtype=dtype), w, origin)[1]
    return ga, gb, w.sum()


def scale(frames_a, frames_b=None, weights=None, fit=True):
    """max_f G_f / W over the finite frames of both ensembles: the size of the terms of msd."""
    ga, gb, wsum = moments(frames_a, frames_b, weights, fit)
    g = ga if gb is None else np.concatenate([ga, gb])
    g = g[np.isfinite(g)]
    return float(g.max() / wsum) if len(g) else 0.0


def rmsd_matrix(frames_a, frames_b=None, weights=None, fit=True, squared=False, dtype=np.float64):
    """The (M, M) or (M, K) matrix of the definition above in the arithmetic of ``dtype``."""
    a = np.asarray(frames_a, dtype=dtype)
    w = np.ones(a.shape[1], dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype)
    wsum = w.sum()
    origin = None if fit else _origin(a[0], w)
    ya, ga = _centred(a, w, origin)
    self_cmp = frames_b is None
    yb, gb = (ya, ga) if self_cmp else _centred(np.asarray(frames_b, dtype=dtype), w, origin)
    with np.errstate(invalid="ignore"):
        wya = w[None, :, None] * ya
    out = np.zeros((len(ya), len(yb)), dtype=dtype)
    for f in range(len(ya)):
        for g in range(f if self_cmp else len(yb)):
            if not (np.isfinite(ga[f]) and np.isfinite(gb[g])):
                continue
            s = wya[f].T @ yb[g]
            lam = em.jacobi_eigh(_horn_matrix(s, dtype))[0].max() if fit else (s[0, 0] + s[1, 1]) + s[2, 2]
            out[f, g] = max(dtype(0), (ga[f] + gb[g]) - 2 * lam) / wsum
    if self_cmp:
        out = out + out.T
    out[~np.isfinite(ga), :] = np.nan
    out[:, ~np.isfinite(gb)] = np.nan
    return out if squared else np.sqrt(out)


def model_errors(frames_a, frames_b=None, weights=None, fit=True):
    """Largest |float64 - longdouble| of msd over the pairs."""
    lo = rmsd_matrix(frames_a, frames_b, weights, fit, squared=True)
    hi = rmsd_matrix(frames_a, frames_b, weights, fit, squared=True, dtype=np.longdouble)
    return float(np.abs(lo - hi).max())


def medoid(msd):
    """The device's rule on a squared matrix: NaN frames neither count nor are counted, the first index among equals."""
    bad = np.isnan(np.diag(msd))
    total = np.where(bad[None, :], 0.0, msd).sum(axis=1)
    total[bad] = np.inf
    return int(np.argmin(total))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def case_frames(case, n_frames=MAX_FRAMES):
    """
    The (M, N, 3) input of a case.  An int N: ``ensemble_model.perturbed_ensemble(N, M)``, perturbed copies of one cloud
    under random rotations and translations (the first frames of a larger ensemble are the smaller one).  "rigid": copies of
    one 65-atom frame under random rigid motions, every exact msd 0.  "mirror": the 65-atom ensemble with every odd frame
    reflected.  "collinear": frames of 9 atoms on a line with perturbed spacings.
    """
    rs = np.random.RandomState(11)
    if case == "rigid":
        base = em.perturbed_ensemble(65, 1)[0]
        return np.stack([base] + [base @ em.random_rotation(rs).T + rs.uniform(-3, 3, 3) for _ in range(n_frames - 1)])
    if case == "mirror":
        frames = em.perturbed_ensemble(65, n_frames).copy()
        frames[1::2] *= MIRROR
        return frames
    if case == "collinear":
        axis = np.array([1.0, 2.0, -1.0])
        out = []
        for _ in range(n_frames):
            t = np.arange(9.0) + 0.1 * rs.randn(9)
            out.append(np.outer(t, axis) @ em.random_rotation(rs).T + rs.uniform(-3, 3, 3))
        return np.stack(out)
    return em.perturbed_ensemble(int(case), n_frames)


def case_atoms(case):
    return {"rigid": 65, "mirror": 65, "collinear": 9}.get(case, case if isinstance(case, int) else None)


def case_weights(case, weighted):
    """None, or ``ensemble_model.atom_weights`` (zeros included); its single weight for N = 1 is a zero: 0.7 there."""
    if not weighted:
        return None
    return em.atom_weights(case_atoms(case)) if case_atoms(case) > 1 else np.array([0.7])


# Measured here (x86-64, longdouble = 80-bit extended): model_errors of the first MODEL_FRAMES frames of case_frames(case),
# {(case, weighted, fit): largest |float64 - longdouble| of msd}; tests/test_rmsd_matrix_host.py re-measures every one and
# holds it to these.  N = 1 and, with atom_weights(2), N = 2 have one weighted atom: every term of a fit is 0 or the rounding of w x / w.
MODEL_ERR = {
    (1, False, True): 0.0, (1, False, False): 8.8e-14, (1, True, True): 8.5e-31, (1, True, False): 9.1e-14,
    (2, False, True): 1.1e-15, (2, False, False): 9.8e-14, (2, True, True): 0.0, (2, True, False): 8.5e-14,
    (3, False, True): 5.9e-15, (3, False, False): 1.8e-13, (3, True, True): 4.9e-15, (3, True, False): 1.3e-13,
    (7, False, True): 2.5e-14, (7, False, False): 2.8e-13, (7, True, True): 1.8e-14, (7, True, False): 3.2e-13,
    (8, False, True): 2.1e-14, (8, False, False): 2.3e-13, (8, True, True): 2.0e-14, (8, True, False): 4.2e-13,
    (9, False, True): 2.8e-14, (9, False, False): 2.6e-13, (9, True, True): 2.3e-14, (9, True, False): 2.9e-13,
    (65, False, True): 1.4e-13, (65, False, False): 1.5e-12, (65, True, True): 1.4e-13, (65, True, False): 1.5e-12,
    (257, False, True): 4.5e-13, (257, False, False): 3.5e-12, (257, True, True): 5.1e-13, (257, True, False): 4.3e-12,
    ("rigid", False, True): 1.2e-13, ("rigid", True, True): 8.6e-14, ("rigid", False, False): 1.2e-12,
    ("mirror", False, True): 9.8e-14, ("collinear", False, True): 5.0e-14,
}


def gate(case, weighted, fit, size):
    """The msd gate of a case whose terms have the size ``size`` (:func:`scale` of the input compared)."""
    return em.gate(MODEL_ERR[(case, bool(weighted), bool(fit))], case_atoms(case), size)


@functools.lru_cache(maxsize=None)
def reference(case, weighted, fit):
    """``(frames, weights, msd, scale)`` of a case at MAX_FRAMES frames, float64, computed once and read-only."""
    frames, w = case_frames(case), case_weights(case, weighted)
    msd = rmsd_matrix(frames, None, w, fit, squared=True)
    for a in (frames, msd):
        a.setflags(write=False)
    return frames, w, msd, scale(frames, None, w, fit)


def compare(got_msd, got_rmsd, ref_msd, gate_msd, label=""):
    """
    Asserts a device msd (and rmsd, unless None) against the model's msd inside the gate; prints and returns the largest
    measured / gate ratio.
    """
    assert got_msd.shape == ref_msd.shape
    assert np.array_equal(np.isnan(got_msd), np.isnan(ref_msd)), f"{label}: NaN pattern differs"
    ok = ~np.isnan(ref_msd)
    d_msd = float(np.abs(got_msd - ref_msd)[ok].max()) if ok.any() else 0.0
    ratio = d_msd / gate_msd if gate_msd > 0 else (0.0 if d_msd == 0 else np.inf)      # (a gate of 0: exact)
    line = f"{label}: msd {d_msd:.2e} / {gate_msd:.2e} = {ratio:.3f}"
    if got_rmsd is not None:
        assert np.array_equal(np.isnan(got_rmsd), np.isnan(ref_msd)), f"{label}: NaN pattern of rmsd differs"
        big = ok & (ref_msd > RMSD_FLOOR * gate_msd)
        if big.any():
            r = float((np.abs(got_rmsd - np.sqrt(ref_msd))[big] * np.sqrt(ref_msd[big])).max() / gate_msd)
            line += f", rmsd (x sqrt(msd)) ratio {r:.3f} on {int(big.sum())} pairs"
            ratio = max(ratio, r)
        small = ok & ~big
        # below the floor: the roots of what the msd comparison allows
        assert np.all(got_rmsd[small] <= np.sqrt(ref_msd[small] + gate_msd) * (1 + 4 * EPS))
        assert np.all(got_rmsd[small] >= np.sqrt(np.maximum(ref_msd[small] - gate_msd, 0.0)) * (1 - 4 * EPS))
    print(line)
    assert ratio <= 1.0, line
    assert np.all(got_msd[ok] >= 0)
    return ratio
