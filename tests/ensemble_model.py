"""
What tests/test_ensemble_host.py and tests/test_ensemble_gpu.py share: the NumPy specification of superposition, iterative
mean fitting and ensemble PCA, the inputs, and the gates.

Specification.  :func:`kabsch` is the textbook SVD solution with the reflection correction (float64 only: LAPACK).
:func:`horn` is Horn's quaternion method with :func:`jacobi_eigh`, a cyclic Jacobi written in plain arithmetic, so that both
run in float64 and in ``np.longdouble``; :func:`pca` (covariance or Gram route) uses the same Jacobi.  The device kernels
follow :func:`horn` step for step, with their sums in a tree where NumPy sums pairwise or in sequence.

Gates.  A device result is compared with the float64 specification.  How far the float64 specification itself is from the
truth is measured against its longdouble evaluation on the same inputs (tests/test_ensemble_host.py measures it and checks it
against the constants below); the gate of a comparison is ``GATE_MULTIPLE`` times that error, with the floor ``n eps scale``:
n the length of the sums (atoms for a superposition, frames for a mean, max(M, 3N) for a PCA), scale the largest centred
coordinate or the largest variance.  The kernels sum in a tree where the specification sums pairwise or in sequence, so they
should do no worse; 8 leaves room for the different order.
"""
import functools

import numpy as np

from tests import subspace

EPS = 2.0 ** -52
GATE_MULTIPLE = 8

SUPERPOSE_ATOMS = (1, 2, 3, 7, 63, 64, 65, 257)
SUPERPOSE_FRAMES = (1, 3, 65)
LDS_LIMIT = 2560            # csrc/ensemble_policy.h: kSuperposeLdsMaxAtoms
LIMIT_ATOMS = (LDS_LIMIT, LDS_LIMIT + 1)
LIMIT_FRAMES = 3
# (M, N) of the PCA cases: Gram, covariance, the boundary M - 1 = 3N (covariance), and more than one tile (Gram)
PCA_CASES = ((5, 7), (40, 7), (22, 7), (65, 64))
DESIGNED_RANK = 12


def gate(measured, n, scale):
    return max(GATE_MULTIPLE * measured, n * EPS * scale)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def random_rotation(rs):
    q, r = np.linalg.qr(rs.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


@functools.lru_cache(maxsize=None)
def rotated_ensemble(n_atoms, n_frames, seed=0):
    """
    ``(target, frames)``: the cloud of ``subspace.ensemble`` as the target and its perturbed members, each under a random
    proper rotation and a translation of up to 3 per axis.  The first frames of a larger ensemble are the smaller one.
    """
    members = subspace.ensemble(n_atoms, n_frames + 1, seed)
    rs = np.random.RandomState(2000 + seed)
    frames = np.empty((n_frames, n_atoms, 3))
    for f in range(n_frames):
        rot, shift = random_rotation(rs), rs.uniform(-3, 3, 3)
        frames[f] = members[f + 1] @ rot.T + shift
    return members[0].copy(), frames


def perturbed_ensemble(n_atoms, n_frames, seed=0):
    """(M, N, 3) like :func:`rotated_ensemble` without its target: what the iterative fit and the closure tests take."""
    return rotated_ensemble(n_atoms, n_frames, seed)[1]


def atom_weights(n_atoms, seed=0):
    w = np.random.RandomState(3000 + seed).rand(n_atoms) + 0.1
    w[::5] = 0.0
    if n_atoms > 1:
        w[1] = 2.0
    return w


def rigid_body_fields(x):
    """(6, 3N) translations and infinitesimal rotations of the structure ``x`` (N, 3) about its centroid."""
    n = len(x)
    d = x - x.mean(axis=0)
    out = np.zeros((6, n, 3))
    for k in range(3):
        out[k, :, k] = 1.0
        e = np.zeros(3)
        e[k] = 1.0
        out[3 + k] = np.cross(e, d)
    return out.reshape(6, 3 * n)


@functools.lru_cache(maxsize=None)
def designed_ensemble(n_frames, n_atoms, seed=0):
    """
    ``(frames, variances, components)``: an ensemble whose covariance is ``sum_j 2^-j q_j q_j^T``, j = 1 .. r, r =
    min(DESIGNED_RANK, M - 1, 3N - 6), exactly up to rounding: the q_j orthonormal and orthogonal to the six rigid-body fields of
    the mean structure, the scores orthonormal centred columns scaled to the variances.  Every eigenvalue is separated from its
    neighbours by half of itself, so every component can be compared as a vector.
    """
    rs = np.random.RandomState(4000 + seed)
    x0 = subspace.cloud(n_atoms, seed)
    r = min(DESIGNED_RANK, n_frames - 1, 3 * n_atoms - 6)
    rigid = np.linalg.qr(rigid_body_fields(x0).T)[0]
    q = rs.randn(3 * n_atoms, r)
    q -= rigid @ (rigid.T @ q)
    q = np.linalg.qr(q)[0]
    u = rs.randn(n_frames, r)
    u -= u.mean(axis=0)
    u = np.linalg.qr(u)[0]
    u -= u.mean(axis=0)          # (the factor's columns sum to zero to rounding; once more for the mean)
    var = 2.0 ** -np.arange(1, r + 1)
    dev = (u * np.sqrt((n_frames - 1) * var)) @ q.T
    return x0[None] + dev.reshape(n_frames, n_atoms, 3), var, q.T.copy()


# ---- plain-arithmetic Jacobi ---------------------------------------------------------------------------------------------------
def jacobi_eigh(a, max_sweeps=30):
    """
    ``(w, v)``: eigenvalues (as they end up on the diagonal, unsorted) and eigenvectors (columns) of the symmetric matrix
    ``a`` by cyclic Jacobi in the arithmetic of ``a.dtype``.  An off-diagonal entry not above ``eps / 256`` of the Frobenius
    norm of ``a`` is set to zero instead of rotated away; the sweeps end when none was rotated.
    """
    a = np.array(a, copy=True)
    dt = a.dtype.type
    n = len(a)
    v = np.eye(n, dtype=a.dtype)
    thr = np.sqrt((a * a).sum()) * dt(np.finfo(a.dtype).eps) / dt(256)
    one = dt(1)
    for _ in range(max_sweeps):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = a[p, q]
                if abs(apq) <= thr:
                    a[p, q] = a[q, p] = 0
                    continue
                rotated = True
                theta = (a[q, q] - a[p, p]) / (2 * apq)
                t = (-one if theta < 0 else one) / (abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                s = t * c
                ap, aq = a[:, p].copy(), a[:, q].copy()
                app, aqq = a[p, p], a[q, q]
                a[:, p] = a[p, :] = c * ap - s * aq
                a[:, q] = a[q, :] = s * ap + c * aq
                a[p, p], a[q, q] = app - t * apq, aqq + t * apq
                a[p, q] = a[q, p] = 0
                vp, vq = v[:, p].copy(), v[:, q].copy()
                v[:, p], v[:, q] = c * vp - s * vq, s * vp + c * vq
        if not rotated:
            break
    return np.diag(a).copy(), v


# ---- superposition -------------------------------------------------------------------------------------------------------------
def _weights(weights, n, dtype):
    return np.ones(n, dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype)


def _finish(rot, x, c, t, ct, w):
    fitted = (x - c) @ rot.T + ct
    res = fitted - t
    rmsd = np.sqrt((w * (res * res).sum(axis=1)).sum() / w.sum())
    return rot, ct - rot @ c, fitted, rmsd


def kabsch(fixed, mobile, weights=None):
    """``(R, t, fitted, rmsd)`` by the SVD of the weighted cross-covariance, the last singular vector flipped for det = +1."""
    t, x = np.asarray(fixed, dtype=np.float64), np.asarray(mobile, dtype=np.float64)
    w = _weights(weights, len(x), np.float64)
    c, ct = (w[:, None] * x).sum(axis=0) / w.sum(), (w[:, None] * t).sum(axis=0) / w.sum()
    s = ((x - c) * w[:, None]).T @ (t - ct)          # S[i, j] = sum w x_i t_j
    u, _, vt = np.linalg.svd(s)
    d = np.sign(np.linalg.det(vt.T @ u.T))
    rot = vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ u.T
    return _finish(rot, x, c, t, ct, w)


def horn(fixed, mobile, weights=None, dtype=np.float64):
    """``(R, t, fitted, rmsd)`` by Horn's quaternion method and :func:`jacobi_eigh`, in the arithmetic of ``dtype``."""
    t, x = np.asarray(fixed, dtype=dtype), np.asarray(mobile, dtype=dtype)
    w = _weights(weights, len(x), dtype)
    c, ct = (w[:, None] * x).sum(axis=0) / w.sum(), (w[:, None] * t).sum(axis=0) / w.sum()
    s = ((x - c) * w[:, None]).T @ (t - ct)
    (sxx, sxy, sxz), (syx, syy, syz), (szx, szy, szz) = s
    n = np.array([[sxx + syy + szz, syz - szy, szx - sxz, sxy - syx],
                  [syz - szy, sxx - syy - szz, sxy + syx, szx + sxz],
                  [szx - sxz, sxy + syx, syy - sxx - szz, syz + szy],
                  [sxy - syx, szx + sxz, syz + szy, szz - sxx - syy]], dtype=dtype)
    lam, v = jacobi_eigh(n)
    q0, q1, q2, q3 = v[:, int(np.argmax(lam))] / np.sqrt((v[:, int(np.argmax(lam))] ** 2).sum())
    rot = np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                    [2 * (q1 * q2 + q0 * q3), q0 * q0 + q2 * q2 - q1 * q1 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                    [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 + q3 * q3 - q1 * q1 - q2 * q2]], dtype=dtype)
    return _finish(rot, x, c, t, ct, w)


def horn_frames(fixed, frames, weights=None, dtype=np.float64):
    """:func:`horn` per frame: ``(R (M, 3, 3), t (M, 3), fitted (M, N, 3), rmsd (M,))``."""
    out = [horn(fixed, x, weights, dtype) for x in frames]
    return tuple(np.array([o[i] for o in out], dtype=dtype) for i in range(4))


def iterative_fit(frames, weights=None, tol=1e-4, max_iter=50, dtype=np.float64):
    """
    ProDy's ``iterpose``: fit on frame 0, then on the running mean, until the RMSD between two successive means is below
    ``tol``.  ``(fitted, mean, passes, converged)``.
    """
    x = np.array(frames, dtype=dtype)
    target = x[0].copy()
    passes, converged = 0, False
    while passes < max_iter:
        x = horn_frames(target, x, weights, dtype)[2]
        passes += 1
        mean = x.mean(axis=0)
        step = np.sqrt(((mean - target) ** 2).sum(axis=1).mean())
        target = mean
        if step < tol:
            converged = True
            break
    return x, target, passes, converged


# ---- PCA ---------------------------------------------------------------------------------------------------------------------------
def centred(frames, masses=None, dtype=np.float64):
    x = np.asarray(frames, dtype=dtype)
    xc = (x - x.mean(axis=0)).reshape(len(x), -1)
    if masses is not None:
        xc = xc * np.repeat(np.sqrt(np.asarray(masses, dtype=dtype)), 3)
    return xc


def covariance(frames, masses=None, dtype=np.float64):
    xc = centred(frames, masses, dtype)
    return xc.T @ xc / (len(xc) - 1)


def pca(frames, n_modes, masses=None, route=None, dtype=np.float64):
    """
    ``(variances (k,) descending, components (k, 3N) unit rows, total variance)`` by the covariance (``route="cov"``), the
    Gram matrix (``"gram"``) or the device's rule (None: Gram while M - 1 < 3N), with :func:`jacobi_eigh`.
    """
    xc = centred(frames, masses, dtype)
    m, n3 = xc.shape
    if route is None:
        route = "gram" if m - 1 < n3 else "cov"
    if route == "gram":
        lam, u = jacobi_eigh(xc @ xc.T / (m - 1))
        order = np.argsort(-lam, kind="stable")[:n_modes]
        comp = (xc.T @ u[:, order]).T
    else:
        lam, u = jacobi_eigh(xc.T @ xc / (m - 1))
        order = np.argsort(-lam, kind="stable")[:n_modes]
        comp = u[:, order].T
    comp = comp / np.sqrt((comp * comp).sum(axis=1))[:, None]
    return lam[order], comp, (xc * xc).sum() / (m - 1)


# ---- the specification's own error: float64 against longdouble ------------------------------------------------------------------------
def superpose_errors(fixed, frames, weights=None):
    """Largest |float64 - longdouble| of (fitted, R, rmsd) of :func:`horn_frames`, and the largest centred coordinate of the target."""
    lo, hi = horn_frames(fixed, frames, weights), horn_frames(fixed, frames, weights, np.longdouble)
    fit, rot, rmsd = (float(np.abs(lo[i] - hi[i]).max()) for i in (2, 0, 3))
    return fit, rot, rmsd, float(np.abs(fixed - fixed.mean(axis=0)).max())


def pca_errors(frames, n_modes, masses=None):
    """Largest |float64 - longdouble| of the variances and largest ``1 - |<v64, vld>|`` of :func:`pca`; the largest variance."""
    lo, hi = pca(frames, n_modes, masses), pca(frames, n_modes, masses, dtype=np.longdouble)
    var = float(np.abs(lo[0] - hi[0]).max())
    comp = float((1 - np.abs((lo[1] * hi[1]).sum(axis=1))).max())
    return var, max(comp, 0.0), float(lo[0][0])


# Measured here (x86-64, longdouble = 80-bit extended) by tests/test_ensemble_host.py's inputs; the host tests check that a
# new measurement stays within them.  {case: (fitted, R, rmsd)} for the superposition of rotated_ensemble(N, 65), and
# {case: (variance, component)} for the PCA cases.
#
# N = 1: every float64 result is exact.  N = 2: the rotation about the axis of the two atoms is free, so the two evaluations
# return different minimisers (|R64 - Rld| = 2.0) and R is compared for N >= 3 only; the fitted atoms lie on the axis and agree.
SPEC_ERR_SUPERPOSE = {
    1: (0.0, 0.0, 0.0),
    2: (1.1e-15, None, 6.6e-16),
    3: (2.7e-15, 9.8e-16, 6.2e-16),
    7: (5.7e-15, 9.7e-16, 7.4e-16),
    63: (1.7e-14, 6.5e-16, 5.6e-16),
    64: (1.8e-14, 6.6e-16, 5.2e-16),
    65: (1.6e-14, 7.3e-16, 4.2e-16),
    257: (3.7e-14, 8.1e-16, 3.3e-16),
    2560: (1.3e-13, 9.2e-16, 1.3e-16),
    2561: (1.1e-13, 5.3e-16, 2.3e-16),
    "weights": (1.3e-14, 6.8e-16, 7.8e-16),
    "mirror": (3.5e-14, 2.5e-15, 6.8e-16),
}
SPEC_ERR_PCA = {
    ("designed", 5, 7): (7.9e-17, 1.3e-17),
    ("perturbed", 5, 7): (1.3e-16, 4.5e-17),
    ("designed", 40, 7): (1.8e-16, 7.2e-17),
    ("perturbed", 40, 7): (4.9e-17, 6.7e-17),
    ("designed", 22, 7): (1.8e-16, 2.8e-17),
    ("perturbed", 22, 7): (8.8e-17, 7.0e-17),
    ("designed", 65, 64): (2.1e-16, 2.1e-16),
    ("perturbed", 65, 64): (3.8e-16, 5.0e-16),
    ("masses", 40, 7): (5.5e-16, 2.5e-18),
}
SPEC_ERR_ITER_MEAN = 6.7e-15    # the mean of iterative_fit(perturbed_ensemble(65, 9))


def superpose_gates(case, n_atoms, scale):
    """(fitted, R, rmsd) gates of a superposition case."""
    fit, rot, rmsd = SPEC_ERR_SUPERPOSE[case]
    return gate(fit, n_atoms, scale), None if rot is None else gate(rot, n_atoms, 1.0), gate(rmsd, n_atoms, scale)


def pca_gates(case, n_frames, n_atoms, largest):
    var, comp = SPEC_ERR_PCA[case]
    n = max(n_frames, 3 * n_atoms)
    return gate(var, n, largest), gate(comp, n, 1.0)
