"""
NumPy restatement of the partial-spectrum eigenvectors of stein.hip: k_stein (inverse iteration) followed by CholQR2
(k_chol_inv and the two GEMMs, twice).  Every vector is a lane of the arrays here, the rows are walked in the kernel's
order, and the rules are the kernel's:

  - tnorm = max_i |d_i| + |e_i| + |e_{i-1}| (1 if 0), tiny = eps tnorm;
  - every shift is kept at least 10 tiny above the one before it (lam_j = max(w_j, lam_{j-1} + 10 tiny), dstein's rule):
    members of a run of equal eigenvalues end up multiples of 10 tiny apart;
  - LU of T - lam I with partial pivoting between rows k and k + 1 (swap when |e_k| > |p|), a kept pivot below tiny
    replaced by +-tiny (+tiny for an exact zero), the last one too;
  - the start vector hash_unit(j + 1, i + 1), 4 iterations of forward / backward substitution, each rescaled by its max
    norm, the last one normalised in the 2-norm;
  - CholQR2: G = X^T X, upper Cholesky with every diagonal entry clamped to >= 1e-300 before its square root, R^-1 by
    columns, X <- X R^-1; twice.

The kernel fuses multiply-adds where this model rounds twice, so the two agree to rounding, not bit for bit.  The model
also reports what the kernel does not: how many pivots were replaced and how small the Cholesky pivots got
(tests/test_stein_model.py).
"""
import numpy as np

EPS = 2.220446049250313e-16


def hash_unit(a, b):
    """hash_unit(a, b) of stein.hip (uint32 a, b; broadcast): a number in [-0.5, 0.5)."""
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (a << np.uint64(32)) ^ (b * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0xD1B54A32D192ED03)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) - 0.5


def tnorm(d, e):
    ae = np.abs(np.asarray(e, dtype=np.float64))
    row = np.abs(np.asarray(d, dtype=np.float64)).copy()
    if len(row) > 1:
        row[:-1] += ae
        row[1:] += ae
    t = float(row.max())
    return t if t != 0.0 else 1.0


def shifts(w, tiny):
    """The shifted eigenvalues k_stein factorises with: each at least 10 tiny above the one before it."""
    lam = np.asarray(w, dtype=np.float64).copy()
    for j in range(1, len(lam)):
        lam[j] = max(lam[j], lam[j - 1] + 10.0 * tiny)
    return lam


def stein(d, e, w, iterations=4, shift_rule=None):
    """
    k_stein: the vectors (n x m, columns) of the eigenvalues w (ascending, as k_sturm_range returns them) of the
    tridiagonal matrix (d, e), before the orthonormalisation.  Returns (X, replaced pivots per vector).
    shift_rule(w, tiny): another rule than shifts() -- what the kernel would deliver with it.
    """
    d = np.asarray(d, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    n, m = len(d), len(w)
    tiny = EPS * tnorm(d, e)
    lam = (shift_rule or shifts)(w, tiny)
    mult = np.zeros((max(n - 1, 0), m))
    swap = np.zeros((max(n - 1, 0), m), dtype=bool)
    b0, b1, b2 = np.zeros((n, m)), np.zeros((n, m)), np.zeros((n, m))
    replaced = np.zeros(m, dtype=np.int64)

    def clamp(p, keep):
        small = keep & (np.abs(p) < tiny)
        replaced[:] += small
        return np.where(small, np.copysign(tiny, np.where(p == 0.0, 1.0, p)), p)

    p = d[0] - lam
    q = np.full(m, e[0] if n > 1 else 0.0)
    r = np.zeros(m)
    for k in range(n - 1):
        sub = e[k]
        dn = d[k + 1] - lam
        en = e[k + 1] if k + 2 < n else 0.0
        sw = abs(sub) > np.abs(p)
        # swap: the pivot row is (sub, dn, en) (sub != 0 there); otherwise the row (p, q, r) is kept
        with np.errstate(divide="ignore", invalid="ignore"):
            m_sw = p / sub
            inv_sw = 1.0 / sub
        pc = np.where(sw, 1.0, clamp(p, ~sw))
        inv_ns = 1.0 / pc
        m_ns = sub * inv_ns
        swap[k] = sw
        mult[k] = np.where(sw, m_sw, m_ns)
        b0[k] = np.where(sw, inv_sw, inv_ns)
        b1[k] = np.where(sw, dn * inv_sw, q * inv_ns)
        b2[k] = np.where(sw, en * inv_sw, r * inv_ns)
        p, q, r = np.where(sw, q - m_sw * dn, dn - m_ns * q), np.where(sw, r - m_sw * en, en - m_ns * r), np.zeros(m)
    b0[n - 1] = 1.0 / clamp(p, np.ones(m, dtype=bool))

    x = hash_unit(np.arange(m)[None, :] + 1, np.arange(n)[:, None] + 1)
    for it in range(iterations):
        xk = x[0].copy()
        for k in range(n - 1):
            xv = x[k + 1].copy()
            s = swap[k]
            xk, xv = np.where(s, xv, xk), np.where(s, xk, xv)
            xv = xv - mult[k] * xk
            x[k] = xk
            xk = xv
        x[n - 1] = xk
        x1, x2, nrm = np.zeros(m), np.zeros(m), np.zeros(m)
        for k in range(n - 1, -1, -1):
            xv = x[k] * b0[k] - b1[k] * x1 - b2[k] * x2
            x[k] = xv
            x2, x1 = x1, xv
            nrm = np.maximum(nrm, np.abs(xv))
        x *= np.where(nrm > 0.0, 1.0 / np.where(nrm > 0.0, nrm, 1.0), 1.0)[None, :]
        if it == iterations - 1:
            x *= (1.0 / np.sqrt((x * x).sum(axis=0)))[None, :]
    return x, replaced


def chol_inv(g):
    """k_chol_inv: upper R with G = R^T R (diagonal clamped to >= 1e-300) and R^-1.  Returns (R^-1, diagonal before
    its square root)."""
    r = np.array(g, dtype=np.float64)
    m = len(r)
    piv = np.zeros(m)
    for k in range(m):
        piv[k] = r[k, k]
        r[k, k] = np.sqrt(max(r[k, k], 1e-300))
        r[k, k + 1:] /= r[k, k]
        r[k + 1:, k + 1:] -= np.triu(np.outer(r[k, k + 1:], r[k, k + 1:]))
    r = np.triu(r)
    ri = np.zeros((m, m))
    for c in range(m):
        for i in range(c, -1, -1):
            s = (1.0 if i == c else 0.0) - r[i, i + 1:c + 1] @ ri[i + 1:c + 1, c]
            ri[i, c] = s / r[i, i]
    return ri, piv


def cholqr2(x, rounds=2):
    """CholQR, `rounds` times; returns (Q, smallest Cholesky pivot of each round relative to the largest)."""
    rel = []
    for _ in range(rounds):
        ri, piv = chol_inv(x.T @ x)
        rel.append(float(piv.min() / piv.max()))
        x = x @ ri
    return x, rel


def eigenvectors(d, e, w, iterations=4, rounds=2, shift_rule=None):
    """The partial-spectrum vectors (n x m, columns) for the eigenvalues w of (d, e), and diagnostics."""
    x, replaced = stein(d, e, w, iterations, shift_rule)
    q, rel = cholqr2(x, rounds)
    return q, {"replaced_pivots": int(replaced.sum()), "chol_min_pivot": rel}
