"""
What tests/test_batch_prs_host.py and tests/test_batch_prs_gpu.py share: the definition of perturbation-response scanning
over selected modes in NumPy, the derived bound both are gated by, and the inputs (networks, selections).

The quantity, for the selected rows r of (w, v), v rows = modes of 3 N components:

    u_r[a]     = scale[a] * v[r, 3a .. 3a+2]                  scale None = 1
    C_ac[d, e] = sum_r u_r[a][d] u_r[c][e] / w[r]
    P[a, c]    = sum_{d, e} C_ac[d, e]^2                      norm: P[a, c] / P[a, a]

The bound is derived, not measured.  With Cabs[d, e] = sum_r |1 / w_r| |u_a,d| |u_c,e| every computed C[d, e] -- in the
kernel (weight times scale, times the entry, the other side's scale, and k - 1 rounded additions: the first lands on an
exact zero) and in NumPy alike -- is within (k + 2) eps Cabs[d, e] of the exact value, the standard bound of a dot product
of k terms; k = listed rows.  Two such values c1, c2 around the exact c differ in their squares by |c1 - c2| |c1 + c2|
<= 2 g Cabs (2 |C| + 2 g Cabs) with g = (k + 2) eps, so

    |P_got - P_model| <= 4 g sum_{d,e} (|C| Cabs)[d, e] + 9 g^2 sum_{d,e} Cabs[d, e]^2

(the nine g^2 terms bounded with 4 <= 9; eps = 2^-52 is twice the unit roundoff, which covers the nine roundings of the sum
of squares, a relative 9 * 2^-53 of P <= sum |C| Cabs, for k >= 3 and is not needed below that, where fewer than k + 2
roundings happen).
"""
import numpy as np

CUTOFF = 13.0
EPS = float(np.finfo(np.float64).eps)

#: uniform sizes of the parity tests: inside one tile with idle lanes, one below / above the 64-atom tile, two tiles and one atom
SIZES = (20, 63, 65, 129)
#: non-contiguous mode lists of 1, 3, 4, 5 and 17 modes (global indices, all >= 6 and < 60 = 3 * 20)
SUBSETS = {
    1: [9],
    3: [6, 8, 11],
    4: [6, 7, 9, 20],
    5: [7, 10, 12, 13, 30],
    17: [6, 8, 9, 11, 14, 15, 17, 20, 22, 25, 26, 29, 33, 38, 41, 50, 57],
}


def network(n_atoms, seed):
    """A compact random network: with InvariantForceField(13) lambda_6 / lambda_max >= 0.01 for the sizes used here."""
    np.random.seed(seed)
    return np.random.rand(n_atoms, 3) * 5 * n_atoms ** (1 / 3)


def pinv_rows(w, rcond=1e-6):
    """Rows the covariance rule keeps: |w| > rcond max|w| (numpy.linalg.pinv, hermitian)."""
    w = np.asarray(w)
    return np.nonzero(np.abs(w) > rcond * np.abs(w).max())[0]


def _blocks(w, v, rows, scale, dtype):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    n = v.shape[1] // 3
    u = np.asarray(v, dtype=dtype)[rows][:, : 3 * n]
    if scale is not None:
        u = u * np.repeat(np.asarray(scale, dtype=dtype), 3)[None, :]
    s = 1 / np.asarray(w, dtype=dtype)[rows]
    return n, u, s


def np_prs(w, v, rows, scale=None, norm=False, dtype=np.float64):
    """The definition above in ``dtype`` arithmetic; ``rows`` index w and the rows of v; returns (N, N)."""
    n, u, s = _blocks(w, v, rows, scale, dtype)
    c = (u * s[:, None]).T @ u                                    # (3N, 3N) covariance over the rows
    p = (c ** 2).reshape(n, 3, n, 3).sum(axis=(1, 3))
    if norm:
        p = p / np.diag(p)[:, None]
    return p


def np_prs_bound(w, v, rows, scale, k):
    """(N, N) bound on |P_got - P_model| for unnormalised results (module docstring); k = listed rows."""
    n, u, s = _blocks(w, v, rows, scale, np.float64)
    c = np.abs((u * s[:, None]).T @ u)
    cabs = (np.abs(u) * np.abs(s)[:, None]).T @ np.abs(u)
    g = (k + 2) * EPS
    first = (c * cabs).reshape(n, 3, n, 3).sum(axis=(1, 3))
    second = (cabs ** 2).reshape(n, 3, n, 3).sum(axis=(1, 3))
    return 4 * g * first + 9 * g * g * second


def check_prs(got, w, v, rows, what, scale=None, norm=False, k=None, factor=1.0):
    """
    Asserts |got - np_prs| <= factor * bound entry by entry (normalised results: both sides divided by the model's
    diagonal) and returns the largest |difference| / bound.  ``k``: listed rows, len(rows) unless the kernel was given more
    (rows without weight are staged as zeros and add exactly nothing).
    """
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    got = np.asarray(got)
    model = np_prs(w, v, rows, scale)
    bound = np_prs_bound(w, v, rows, scale, len(rows) if k is None else k)
    assert got.shape == model.shape, (what, got.shape, model.shape)
    assert np.all(np.isfinite(got)), what
    if norm:
        d = np.diag(model)[:, None]
        model, bound = model / d, bound / d
    ratio = float((np.abs(got - model) / bound).max())
    print(f"{what}: max |difference| / bound = {ratio:.3e}")
    assert ratio <= factor, (what, ratio)
    return ratio


def ref_prs(h, norm=False):
    """The reference's formula (nma.py:511-524) on a Hessian: pinv, cov**2, two reduceat."""
    cov = np.linalg.pinv(h, hermitian=True, rcond=1e-6)
    c2 = cov ** 2
    idx = np.arange(0, len(h), 3)
    mat = np.add.reduceat(np.add.reduceat(c2, idx, axis=0), idx, axis=1)
    if norm:
        mat = mat / np.diag(mat)[:, None]
    return mat

