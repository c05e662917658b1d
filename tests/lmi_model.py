"""
What tests/test_lmi_host.py and tests/test_lmi_gpu.py share: the NumPy specification of the generalized correlation from the
linear mutual information (Lange & Grubmueller 2006) over selected modes, the inputs, and the gate.

Specification, for the selected rows r of (w, v), v rows = modes of 3 N components (``scale``: None = 1):

    u_r[a] = scale[a] * v[r, 3a .. 3a+2]
    C_ac   = sum_r u_r[a] u_r[c]^T / w[r]                  (3 x 3; C_aa symmetric)
    P_a C_aa P_a^T = L_a L_a^T (Cholesky with diagonal pivoting),  W_a = L_a^-1 P_a           W_a C_aa W_a^T = I
    M      = W_a C_ac W_c^T
    delta  = det(I - M M^T)   clamped to [0, 1]
    I_ac   = -1/2 ln(delta)                                 mutual information, nats
    r_ac   = sqrt(1 - delta^(1/3))                          generalized correlation coefficient

Pivoting changes W_a by an orthogonal factor and leaves delta as it is; it bounds the growth of the elimination, so that the
last pivot of a rank-deficient block is O(eps) times its diagonal entry (without it: up to 1.2e-12 on the inputs below).
A Cholesky pivot that is not finite or is <= 2^-40 times the block's own diagonal entry makes W_a NaN, and with it row and
column a, the diagonal included; elsewhere r[a, a] = 1 and I[a, a] = +inf by definition.  :func:`whiten` and
:func:`pair_values` write the operations in the order of csrc/mode_lmi.hip; both run in float64 and in ``np.longdouble``.

Inputs.  :func:`lattice`: the n points of a cubic lattice of spacing 3.8 that lie nearest its centre, each moved by a
Gaussian of sigma 0.5, under the invariant force field with cutoff 8: a connected network at every size used here
(lambda_6 ~ 0.3 .. 0.8 against lambda_5 ~ 1e-15).  A random Gaussian cloud of these sizes is disconnected under any cutoff that
keeps the network sparse, and every block of a disconnected network is singular.

Gate.  A device result is compared with the float64 specification evaluated on the device's own (w, v).  How far the float64
specification is from the truth is measured against its longdouble evaluation on the same input (:func:`spec_error`); a
comparison passes within ``GATE_MULTIPLE`` times that error, with the floor ``N eps`` (N atoms) -- the rule of
tests/ensemble_model.py's ``gate``.  The multiple leaves room for the other summation order of the matrix units and for
fused multiply-adds.  tests/test_lmi_host.py measures the error on LAPACK's eigenpairs of the same networks and checks it
against ``SPEC_ERR`` below; the GPU tests measure it on the eigenpairs they are given and fall back to the entry of
``SPEC_ERR`` for the size and selection only where longdouble is a double.
"""
import functools

import numpy as np

EPS = 2.0 ** -52
GATE_MULTIPLE = 8
PIVOT_FLOOR = 2.0 ** -40
CUTOFF = 8.0
SPACING, JITTER = 3.8, 0.5

#: 5: one partial tile; 63 / 64 / 65: around the 64-atom tile (65: a one-atom second tile; 63, 65: odd, rows only 8-byte
#: aligned); 130: a full off-diagonal tile plus partial ones
SIZES = (5, 63, 64, 65, 130)
#: members of the ragged batch
RAGGED_SIZES = (30, 70, 130)


def subsets(n_atoms):
    """{name: global mode indices}: 3 (perfect correlation), 4, 8 and 9 (one staged group of rows, and its one-row tail), 20."""
    out = {"3": np.arange(6, 9), "4": np.array([6, 7, 9, 12]), "8": np.arange(6, 14),
           "9": np.array([13, 6, 9, 7, 14, 8, 11, 10, 12])}
    if 3 * n_atoms >= 6 + 20:
        out["20"] = np.concatenate([np.arange(6, 16), np.arange(17, 37, 2)])
    return out


@functools.lru_cache(maxsize=None)
def lattice(n_atoms, seed=0):
    side = 7
    g = np.arange(side) - (side - 1) / 2
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    order = np.argsort((pts * pts).sum(axis=1), kind="stable")[:n_atoms]
    coord = pts[order] * SPACING + np.random.RandomState(100 + seed).randn(n_atoms, 3) * JITTER
    coord.setflags(write=False)
    return coord


def pinv_rows(w, rcond=1e-6):
    """Rows the covariance rule keeps: |w| > rcond max|w| (numpy.linalg.pinv, hermitian)."""
    w = np.asarray(w)
    return np.nonzero(np.abs(w) > rcond * np.abs(w).max())[0]


# ---- the specification ---------------------------------------------------------------------------------------------------------
def covariance_blocks(w, v, rows, scale=None, dtype=np.float64):
    """(N, N, 3, 3): block [a, c] of the covariance over ``rows`` (they index w and the rows of v)."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    n = v.shape[1] // 3
    u = np.asarray(v, dtype=dtype)[rows][:, : 3 * n]
    if scale is not None:
        u = u * np.repeat(np.asarray(scale, dtype=dtype), 3)[None, :]
    s = 1 / np.asarray(w, dtype=dtype)[rows]
    c = (u * s[:, None]).T @ u
    return c.reshape(n, 3, n, 3).transpose(0, 2, 1, 3)


def whiten(blocks):
    """
    (N, 3, 3) factors W_a = L_a^-1 P_a of the symmetric blocks (N, 3, 3), P_a C_aa P_a^T = L_a L_a^T the Cholesky factorisation
    with diagonal pivoting (the largest remaining diagonal entry next, the lower index on a tie; written with the comparisons
    of k_lmi_whiten, so that NaN takes the same way); all NaN where a pivot fails the rule.
    """
    b = np.asarray(blocks)
    one, floor = b.dtype.type(1), b.dtype.type(PIVOT_FLOOR)
    out = np.zeros(b.shape, dtype=b.dtype)
    with np.errstate(all="ignore"):
        for n, a in enumerate(b):
            p0 = 1 if a[1, 1] > a[0, 0] else 0
            if a[2, 2] > a[p0, p0]:
                p0 = 2
            q1, q2 = (1 if p0 == 0 else 0), (1 if p0 == 2 else 2)
            b00 = a[p0, p0]
            l00 = np.sqrt(b00)
            l10, l20 = a[q1, p0] / l00, a[q2, p0] / l00
            s11, s22 = a[q1, q1] - l10 * l10, a[q2, q2] - l20 * l20
            s12 = a[q2, q1] - l20 * l10
            if s22 > s11:
                q1, q2, l10, l20, s11, s22 = q2, q1, l20, l10, s22, s11
            d1 = s11
            l11 = np.sqrt(d1)
            l21 = s12 / l11
            d2 = s22 - l21 * l21
            l22 = np.sqrt(d2)
            ok = (np.isfinite(b00) and b00 > floor * b00 and np.isfinite(d1) and d1 > floor * a[q1, q1]
                  and np.isfinite(d2) and d2 > floor * a[q2, q2])
            if not ok:
                out[n] = np.nan
                continue
            w00, w11, w22 = one / l00, one / l11, one / l22
            w10 = -(l10 * w00) * w11
            w21 = -(l21 * w11) * w22
            w20 = -(l20 * w00 + l21 * w10) * w22
            out[n][:, p0] = (w00, w10, w20)
            out[n][1:, q1] = (w11, w21)
            out[n][2, q2] = w22
    return out


def delta_of(c, wh):
    """(N, N) det(I - M M^T), M = W_a C_ac W_c^T, by the first row's cofactors; clamped to [0, 1], NaN stays NaN."""
    with np.errstate(all="ignore"):
        t = np.einsum("aij,acjk->acik", wh, c)
        m = np.einsum("acik,clk->acil", t, wh)
        s = np.einsum("acik,acjk->acij", m, m)
        one = c.dtype.type(1)
        a00, a11, a22 = one - s[..., 0, 0], one - s[..., 1, 1], one - s[..., 2, 2]
        a01, a02, a12 = -s[..., 0, 1], -s[..., 0, 2], -s[..., 1, 2]
        d = a00 * (a11 * a22 - a12 * a12) - a01 * (a01 * a22 - a12 * a02) + a02 * (a01 * a12 - a11 * a02)
        return np.where(d < 0, 0 * d, np.where(d > 1, 0 * d + 1, d))


def pair_values(delta, wh, information):
    with np.errstate(all="ignore"):
        half, one = delta.dtype.type(0.5), delta.dtype.type(1)
        out = -half * np.log(delta) if information else np.sqrt(one - np.cbrt(delta))
    bad = np.isnan(wh).any(axis=(1, 2))
    idx = np.arange(len(wh))
    out[idx, idx] = np.where(bad, np.nan, np.inf if information else 1.0)
    return out


def np_lmi(w, v, rows, scale=None, information=False, dtype=np.float64):
    """The specification in ``dtype`` arithmetic: (N, N) r, or I with ``information``."""
    c = covariance_blocks(w, v, rows, scale, dtype)
    idx = np.arange(len(c))
    wh = whiten(c[idx, idx])
    return pair_values(delta_of(c, wh), wh, information)


def np_lmi_logdet(cov, dim=3, information=False):
    """
    Lange & Grubmueller's form on a full covariance (dim N, dim N): I = 1/2 [ln det C_aa + ln det C_cc - ln det C_(ac)] on the
    2 dim x 2 dim block of every pair, r = sqrt(1 - exp(-2 I / dim)); the diagonal as defined.  float64, LAPACK.
    """
    n = len(cov) // dim
    out = np.empty((n, n))
    ld = [np.linalg.slogdet(cov[dim * a: dim * a + dim, dim * a: dim * a + dim])[1] for a in range(n)]
    for a in range(n):
        for c in range(n):
            if a == c:
                out[a, c] = np.inf
                continue
            ix = np.r_[dim * a: dim * a + dim, dim * c: dim * c + dim]
            out[a, c] = 0.5 * (ld[a] + ld[c] - np.linalg.slogdet(cov[np.ix_(ix, ix)])[1])
    return out if information else np.sqrt(1 - np.exp(-2 * out / dim))


# ---- the gate --------------------------------------------------------------------------------------------------------------------
def extended():
    return np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def spec_error(w, v, rows, scale=None):
    """Largest |float64 - longdouble| of r over the entries that are finite in both; the positions of the others must agree."""
    lo, hi = np_lmi(w, v, rows, scale), np_lmi(w, v, rows, scale, dtype=np.longdouble)
    assert np.array_equal(np.isfinite(lo), np.isfinite(hi))
    f = np.isfinite(lo)
    return float(np.abs(lo[f] - hi[f]).max()) if f.any() else 0.0


def gate(measured, n_atoms):
    return max(GATE_MULTIPLE * measured, n_atoms * EPS)


def recorded_error(n_atoms, n_rows):
    """
    The recorded constant nearest this input, for platforms without an extended long double: the entry of (N, selection) with
    the selection named by its number of rows ("all" above 20), else the largest entry of that selection over the sizes.
    """
    name = str(n_rows) if n_rows <= 20 and any(k[1] == str(n_rows) for k in SPEC_ERR) else "all"
    if (n_atoms, name) in SPEC_ERR:
        return SPEC_ERR[(n_atoms, name)]
    return max(e for k, e in SPEC_ERR.items() if k[1] == name)


def gate_for(w, v, rows, n_atoms, scale=None):
    """The gate of a comparison on this input: measured here, or from the recorded constants without a long double."""
    rows = np.asarray(rows).reshape(-1)
    return gate(spec_error(w, v, rows, scale) if extended() else recorded_error(n_atoms, len(rows)), n_atoms)


def info_of(r):
    """I = -3/2 ln(1 - r^2), the exact relation between the two results (+inf at r = 1)."""
    with np.errstate(all="ignore"):
        return -1.5 * np.log1p(-r * r)


def check_lmi(got, w, v, rows, what, scale=None, information=False):
    """
    Asserts ``got`` against the float64 specification on (w, v, rows); no entry is left out.  NaN must stand exactly where
    the specification has it.  r: every other entry within the gate.  I (``information``): the diagonal is exactly the
    specification's, and every other entry lies in [I(r - gate), I(r + gate)] with r the specification's coefficient and
    I(r) = -3/2 ln(1 - r^2) -- the gate scaled by dI/dr, without linearising it, so that it also holds where r + gate >= 1:
    there the upper end is +inf, and I may be large or +inf (fewer than six selected modes make every 6 x 6 block singular;
    delta is then 0 up to rounding, of either sign, in the kernel and in the specification alike).  Elsewhere +inf fails.
    Returns measured / gate (for I: of sqrt(1 - exp(-2 I / 3)) against r).
    """
    got = np.asarray(got)
    n = got.shape[0]
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    g = gate_for(w, v, rows, n, scale)
    r = np_lmi(w, v, rows, scale)
    assert got.shape == r.shape, (what, got.shape, r.shape)
    assert np.array_equal(np.isnan(got), np.isnan(r)), f"{what}: NaN at other places than the specification's"
    f = ~np.isnan(r)
    if not information:
        ratio = float((np.abs(got[f] - r[f]) / g).max()) if f.any() else 0.0
    else:
        spec = np_lmi(w, v, rows, scale, information=True)
        idx = np.arange(n)
        assert np.array_equal(got[idx, idx], spec[idx, idx], equal_nan=True), f"{what}: the diagonal"
        f[idx, idx] = False
        lo, hi = info_of(np.maximum(r[f] - g, 0.0)), info_of(np.minimum(r[f] + g, 1.0))
        assert np.all(got[f] >= lo * (1 - 8 * EPS)) and np.all(got[f] <= hi * (1 + 8 * EPS)), f"{what}: I outside the gate"
        with np.errstate(all="ignore"):
            back = np.sqrt(-np.expm1(-2 * got[f] / 3))
        ratio = float((np.abs(back - r[f]) / g).max()) if f.any() else 0.0
    print(f"{what}: measured / gate = {ratio:.3e} (gate {g:.2e})")
    if not information:                                     # (for I the interval above is the assertion; the ratio is reported)
        assert ratio <= 1.0, (what, ratio)
    return ratio


# Largest |float64 - longdouble| of r, measured by tests/test_lmi_host.py on LAPACK's eigenpairs of lattice(N) (2026-10-20,
# x86-64, longdouble = 80-bit extended, NumPy with OpenBLAS): {(N, selection): error}; "all" is the covariance rule, "masses"
# the Cartesian covariance of a mass-weighted solve.  With six or more modes r lay in 0.01 .. 0.98 and the error is a few
# eps / r; with three to five modes every 6 x 6 block is singular, r = 1 - delta^(1/3) / 2 with delta a rounding-level
# number: its cube root is what is listed ("4": one factor of delta is ~1e-16, the other two of order one).  These are maxima
# of rounding noise and move with the eigenvectors' last bits: the host test checks that the gate of a new measurement
# stays within four times the gate of the recorded one.
SPEC_ERR = {
    (5, '3'): 1.1e-14, (5, '4'): 5.0e-07, (5, '8'): 3.4e-16, (5, '9'): 6.5e-16, (5, 'all'): 3.3e-16,
    (63, '3'): 1.1e-13, (63, '4'): 1.0e-06, (63, '8'): 5.4e-14, (63, '9'): 1.8e-14, (63, '20'): 9.9e-16, (63, 'all'): 2.3e-15,
    (64, '3'): 8.4e-14, (64, '4'): 1.0e-06, (64, '8'): 1.3e-14, (64, '9'): 1.1e-14, (64, '20'): 1.7e-15, (64, 'all'): 2.7e-15,
    (65, '3'): 1.8e-13, (65, '4'): 1.0e-06, (65, '8'): 4.8e-14, (65, '9'): 5.7e-15, (65, '20'): 8.2e-16, (65, 'all'): 2.0e-15,
    (130, '3'): 9.0e-14, (130, '4'): 1.1e-06, (130, '8'): 2.3e-14, (130, '9'): 9.3e-15, (130, '20'): 2.7e-15,
    (130, 'all'): 3.3e-15,
    (30, '3'): 4.4e-13, (30, '4'): 8.8e-07, (30, '8'): 1.5e-14, (30, '9'): 7.6e-15, (30, '20'): 1.3e-15, (30, 'all'): 1.2e-15,
    (70, '3'): 9.1e-14, (70, '4'): 1.0e-06, (70, '8'): 8.7e-15, (70, '9'): 4.3e-15, (70, '20'): 1.3e-15, (70, 'all'): 2.1e-15,
    (63, 'masses'): 2.9e-15,
}
