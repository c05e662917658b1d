"""
What tests/test_subspace_host.py and tests/test_subspace_gpu.py share: the NumPy specification of the pairwise comparison
of mode subspaces, an independent reference of the covariance overlap, the derived bounds, and the inputs.

For the listed rows i of (w_a, v_a) and j of (w_b, v_b), v rows = modes, and weights p >= 0 per listed row:

    G[i, j] = <v_a[i], v_b[j]>        S = sum_ij p_a[i] p_b[j] G[i, j]^2        t = sum_i p[i]
    RMSIP              p = 1            sqrt(S / sqrt(t_a t_b))
    covariance overlap p = 1 / sqrt(w)  1 - sqrt(max(0, T_a + T_b - 2 S) / (T_a + T_b)),  T = sum 1 / w = sum p^2

(the bound on S is stated with t = sum p of the weights in use, also for the covariance overlap)

The bounds are derived, not measured.  The rows of v are unit vectors, eps = 2^-52 (twice the unit roundoff u).
A computed dot product of m terms is within m u (1 + o(1)) |a| |b| = m u of the exact one, so two computed values of G
differ by at most 2 m u = m eps: the gate on G is 2 m eps.  With g the staged sqrt(p_a p_b) G, |g| <= sqrt(p_a p_b), two
computed squares differ by |g1 - g2| |g1 + g2| <= (m eps p) (2 + m eps) with p = p_a p_b; summed over the pairs 2 m eps t_a
t_b (1 + ...).  The weights' own roundings (a quotient and two roots, 3 u relative each way) and the summation of at most
k_a k_b non-negative terms -- pairwise in NumPy and by a fixed tree on the device: log2 terms -- add a relative (6 + log2(k_a
k_b)) u of S <= t_a t_b, below m eps for the shapes used.  8 m eps t_a t_b leaves a factor of about three.
"""
import numpy as np

CUTOFF = 13.0
EPS = 2.0 ** -52


def cloud(n_atoms, seed):
    """A compact random network (the clouds of tests/batch_prs.py)."""
    rs = np.random.RandomState(seed)
    return rs.rand(n_atoms, 3) * 5 * n_atoms ** (1 / 3)


def ensemble(n_atoms, batch, seed=0, noise=0.25):
    """(batch, n_atoms, 3): one cloud and small random perturbations of it -- related subspaces, not equal ones."""
    base = cloud(n_atoms, seed)
    rs = np.random.RandomState(1000 + seed)
    return np.stack([base] + [base + noise * rs.randn(n_atoms, 3) for _ in range(batch - 1)])


def pinv_rows(w, rcond=1e-6):
    w = np.asarray(w)
    return np.nonzero(np.abs(w) > rcond * np.abs(w).max())[0]


def np_gram(va, vb, rows_a, rows_b, dtype=np.float64):
    ra, rb = np.asarray(rows_a, dtype=np.int64).reshape(-1), np.asarray(rows_b, dtype=np.int64).reshape(-1)
    return np.asarray(va, dtype=dtype)[ra] @ np.asarray(vb, dtype=dtype)[rb].T


def np_S(va, vb, rows_a, rows_b, pa, pb, dtype=np.float64):
    """S of the definition above; pa / pb: the weights of the listed rows."""
    g = np_gram(va, vb, rows_a, rows_b, dtype)
    pa, pb = np.asarray(pa, dtype=dtype).reshape(-1), np.asarray(pb, dtype=dtype).reshape(-1)
    return (pa[:, None] * pb[None, :] * g ** 2).sum()


def cov_weights(w, rows, dtype=np.float64):
    """p = 1 / sqrt(lambda) of the listed rows."""
    lam = np.asarray(w, dtype=dtype)[np.asarray(rows, dtype=np.int64).reshape(-1)]
    return 1 / np.sqrt(lam)


def np_rmsip(va, vb, rows_a, rows_b):
    ka, kb = np.size(rows_a), np.size(rows_b)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(np_S(va, vb, rows_a, rows_b, np.ones(ka), np.ones(kb)) / np.sqrt(float(ka) * float(kb)))


def np_cov_overlap(wa, va, wb, vb, rows_a, rows_b):
    pa, pb = cov_weights(wa, rows_a), cov_weights(wb, rows_b)
    ta, tb = (pa ** 2).sum(), (pb ** 2).sum()
    s = np_S(va, vb, rows_a, rows_b, pa, pb)
    return 1 - np.sqrt(max(0.0, ta + tb - 2 * s) / (ta + tb))


def _sqrtm_psd(a):
    """
    Root of a positive semi-definite matrix of known rank deficiency: eigenvalues below 1e-10 of the largest are the null
    space (the trivial modes and what was not selected; the covariances here have a condition below 1e4 on their range) and
    are set to 0 -- left at their rounding level, +-eps |A|, their roots would be 1e-8 sqrt|A|.
    """
    lam, q = np.linalg.eigh(a)
    lam = np.where(lam > 1e-10 * lam.max(), lam, 0.0)
    return (q * np.sqrt(lam)) @ q.T


def ref_cov_overlap(wa, va, wb, vb, rows_a, rows_b):
    """Independent route: the two dense covariances, their matrix square roots, tr(A) + tr(B) - 2 tr(sqrt(A) sqrt(B))."""
    def cov(w, v, rows):
        r = np.asarray(rows, dtype=np.int64).reshape(-1)
        return (v[r].T / w[r]) @ v[r]

    a, b = cov(wa, va, rows_a), cov(wb, vb, rows_b)
    d2 = np.trace(a) + np.trace(b) - 2 * np.trace(_sqrtm_psd(a) @ _sqrtm_psd(b))
    return 1 - np.sqrt(max(0.0, d2) / (np.trace(a) + np.trace(b)))


def s_bound(m, ta, tb):
    return 8 * m * EPS * ta * tb


def rmsip_interval(s, ta, tb, ds):
    """[lo, hi] a computed RMSIP may lie in when its S is within ``ds`` of ``s``: the bound propagated, four roundings' slack."""
    c = np.sqrt(ta * tb)
    return np.sqrt(max(s - ds, 0.0) / c) * (1 - 4 * EPS), np.sqrt((s + ds) / c) * (1 + 4 * EPS)


def cov_overlap_interval(s, Ta, Tb, ds, k):
    """
    The same for the covariance overlap, T = sum 1 / lambda.  x = (T_a + T_b - 2 S) / (T_a + T_b) = 1 - r, r = 2 S / (T_a +
    T_b): S within ``ds``, the T (k positive terms of one rounding each, added pairwise or by a tree) within (k + 4) eps
    relative, and four roundings of the cancelling difference and the quotient, absolute in x since every operand is <= T_a +
    T_b.
    """
    tt = Ta + Tb
    r = 2 * s / tt
    dx = 2 * ds / tt + r * (k + 4) * EPS + 4 * EPS
    x = 1 - r
    return 1 - np.sqrt(max(x + dx, 0.0)) - 2 * EPS, 1 - np.sqrt(max(x - dx, 0.0)) + 2 * EPS
