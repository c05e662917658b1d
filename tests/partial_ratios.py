"""
References for the partial-spectrum stage (springcraft_amd/csrc/stein.hip: k_sturm_range, k_window_count, k_stein, CholQR2
with k_chol_inv, k_window_compact), and the ctypes binding of the staged debug entry sc_dbg_partial_tridiag_host
(include/springcraft_hip_debug.h), which runs the product's host functions on tridiagonal matrices from the host.

With ulp = np.finfo(float).eps, the 1-norm, T of order n and m vectors as the columns of Z:

    value(w, lam)  = max |w - lam| / (ulp |T|_1)                  lam: the exact eigenvalues (below)
    resid(T, w, Z) = |T Z - Z diag(w)|_1 / (n ulp |T|_1)          (dstein's test, dstt22 without the U^T)
    orth(Z)        = |I - Z^T Z|_1 / (n ulp)

The exact eigenvalues come from bisection on dstebz's ratio-form Sturm count in np.longdouble (64-bit significand: the
count's own error is 2000 times below ulp |T|), cross-checked against mpmath at 40 digits
(tests/test_partial_ratios_host.py).  stein_restated() is the float64 NumPy model of k_stein and the CholQR2 driver (tools/models/stein_model.py): what the
algorithm can deliver, apart from the kernel.  window_rule() / compact_rule() restate
k_window_count and k_window_compact.
"""
import ctypes as C

import numpy as np
import scipy.linalg

from tools.models import stein_model as sm

from tests.stage_ratios import GATE, LAPACK_GATE, ULP, norm1, toeplitz_exact, tridiagonal, tridiagonal_inputs  # noqa: F401

LD = np.longdouble
HAVE_LONGDOUBLE = bool(np.finfo(LD).eps < 2e-19)
DBL_MAX = np.finfo(float).max
SAFEMIN = np.finfo(float).tiny

ORDERS = [130, 257, 520, 1030]

# The worst value() of dstebz (scipy.linalg.eigh_tridiagonal, lapack_driver="stebz", its default abstol) per input over
# ORDERS x ranges(), rounded up; tests/test_partial_ratios_host.py holds dstebz to them, tests/test_partial_ratios_gpu.py
# holds k_sturm_range to three times as much (and never to less than 3).
DSTEBZ_VALUE = {"toeplitz": 1.04, "wilkinson": 1.0, "glued1e-4": 0.83, "glued1e-12": 0.79, "graded": 0.58, "torn": 0.96,
                "equal": 1.02, "negative": 0.74, "identity": 0.0}


def ranges(n):
    """(label, il, m): the lowest 70, 44 in the middle, the highest 65."""
    return [("low70", 0, 70), ("mid44", (n - 44) // 2, 44), ("top65", n - 65, 65)]


def t_norm1(d, e):
    n = len(d)
    ee = np.abs(np.asarray(e, dtype=float)[:n - 1])
    col = np.abs(d).astype(float)
    col[:n - 1] += ee
    col[1:] += ee
    return float(col.max())


# ---- exact eigenvalues ---------------------------------------------------------------------------------------------------
def sturm_count(d, e, x):
    """Number of eigenvalues of T below every shift of x (an array), dstebz's ratio form with pivmin, in the type of x."""
    n = len(d)
    x = np.asarray(x)
    ty = x.dtype.type
    dd = np.asarray(d, dtype=x.dtype)
    e2 = np.asarray(e, dtype=x.dtype)[:n - 1] ** 2
    pivmin = ty(SAFEMIN) * max(ty(1.0), e2.max() if n > 1 else ty(0.0))
    cnt = np.zeros(x.shape, dtype=np.int64)
    q = dd[0] - x
    q = np.where(np.abs(q) < pivmin, -pivmin, q)
    cnt += q < 0
    for i in range(1, n):
        q = dd[i] - x - e2[i - 1] / q
        q = np.where(np.abs(q) < pivmin, -pivmin, q)
        cnt += q < 0
    return cnt


def exact_eigenvalues(d, e, il, m):
    """Eigenvalues il .. il + m - 1 (0-based, ascending) of T in np.longdouble: bisection to a bracket of 2^-70 |T| (or to
    neighbouring long doubles)."""
    assert HAVE_LONGDOUBLE
    n = len(d)
    tn = LD(max(t_norm1(d, e), SAFEMIN))
    k = np.arange(il, il + m)
    lo = np.full(m, -tn * LD(1.0 + 1e-10) - LD(SAFEMIN), dtype=LD)
    hi = -lo
    stop = tn * LD(2.0) ** -70
    if n > 1:
        # start from dstebz's values +- 16 ulp |T| where the exact count confirms that bracket (a third of the steps)
        guess = scipy.linalg.eigvalsh_tridiagonal(np.asarray(d, dtype=float), np.asarray(e, dtype=float)[:n - 1],
                                                  select="i", select_range=(il, il + m - 1), lapack_driver="stebz")
        glo, ghi = guess.astype(LD) - LD(16.0 * ULP) * tn, guess.astype(LD) + LD(16.0 * ULP) * tn
        ok = (sturm_count(d, e, glo) <= k) & (sturm_count(d, e, ghi) > k)
        lo, hi = np.where(ok, glo, lo), np.where(ok, ghi, hi)
    for _ in range(200):
        mid = (lo + hi) / LD(2.0)
        live = (mid > lo) & (mid < hi) & (hi - lo > stop)
        if not live.any():
            break
        above = sturm_count(d, e, mid) > k
        hi = np.where(live & above, mid, hi)
        lo = np.where(live & ~above, mid, lo)
    assert n >= 1
    return (lo + hi) / LD(2.0)


def toeplitz_exact_ld(n):
    """stage_ratios.toeplitz_exact evaluated in np.longdouble, so that the formula's own rounding stays out of `value`."""
    pi = LD(4.0) * np.arctan(LD(1.0))
    return LD(2.0) - LD(2.0) * np.cos(np.arange(1, n + 1).astype(LD) * pi / LD(n + 1))


# ---- ratios --------------------------------------------------------------------------------------------------------------
def value(w, lam, tn):
    """max |w - lam| / (ulp |T|_1); the difference is taken in the type of lam."""
    return float(np.abs(np.asarray(w, dtype=lam.dtype) - lam).max() / (ULP * tn))


def resid(d, e, w, z):
    n = len(d)
    t = tridiagonal(d, e)
    diff, tn = norm1(t @ z - z * w[None, :]), t_norm1(d, e)
    if tn == 0.0:           # (the zero matrix: stage_ratios.recon's convention)
        return 0.0 if diff == 0.0 else np.inf
    return diff / (n * ULP * tn)


def orth(z):
    n, m = z.shape
    return norm1(np.eye(m) - z.T @ z) / (n * ULP)


def projector_difference(z, basis):
    """|Z Z^T - B B^T|_1 for two orthonormal bases (columns) of what should be one subspace."""
    return norm1(z @ z.T - basis @ basis.T)


# ---- k_stein + CholQR2, restated (tools/models/stein_model.py) ---------------------------------------------------------------
def shifts_additive(w, tiny):
    """The shift rule k_stein had before these tests: w[j] + (place in its run of gaps <= 10 tiny) x 10 tiny.  Kept to
    show what it does on runs whose members differ (tests/test_partial_ratios_host.py)."""
    w = np.asarray(w, dtype=float)
    run = np.zeros(len(w))
    for j in range(1, len(w)):
        run[j] = run[j - 1] + 1 if abs(w[j - 1] - w[j]) <= 10.0 * tiny else 0
    return w + run * 10.0 * tiny


def shifts_none(w, tiny):
    return np.asarray(w, dtype=float).copy()


def stein_restated(d, e, w, iterations=4, rounds=2, shift_rule=None):
    """Z (n, m) as k_stein and the CholQR2 driver compute it from the eigenvalues w: the NumPy model of the kernels.  A
    Gram matrix that is singular to working precision meets k_chol_inv's floor and overflows, in the model as in the
    kernel: the ratios of the result are then inf / nan, which no gate accepts."""
    n = len(d)
    with np.errstate(all="ignore"):
        z, _ = sm.eigenvectors(np.asarray(d, dtype=float), np.asarray(e, dtype=float)[:n - 1], np.asarray(w, dtype=float),
                               iterations, rounds, shift_rule)
    return z


_reduced = []


def reduced_multiplicities():
    """(d, e) of order 300: the Householder tridiagonal form (scipy's hessenberg) of Q diag(lambda) Q^T, lambda in clusters of
    exact multiplicities 1, 5, 12, 1, 8, 3, 20, 1, 7, 2 followed by simple eigenvalues (tests.util.clustered_spectrum)."""
    if not _reduced:
        from tests.util import clustered_spectrum, random_orthogonal

        n = 300
        lam = clustered_spectrum(0.0, seed=2, n=n)
        q = random_orthogonal(8, n)
        a = (q * lam[None, :]) @ q.T
        h = scipy.linalg.hessenberg(0.5 * (a + a.T))
        d, e = np.diag(h).copy(), np.append(np.diag(h, -1), 0.0)
        d.setflags(write=False)
        e.setflags(write=False)
        _reduced.append((d, e))
    return _reduced[0]


# ---- k_window_count / k_window_compact, restated -----------------------------------------------------------------------------
def window_rule(lam, vl, vu, K, f=1.0, own=None):
    """(il, count, start) of the window (vl, vu] on the ascending eigenvalues lam of the T = f A that was solved."""
    n = len(lam)
    n_own = n if own is None else own

    def count_le(bound):
        with np.errstate(over="ignore"):
            x = np.float64(bound) * np.float64(f)
        if np.isinf(x) and not np.isinf(bound):
            x = np.copysign(DBL_MAX, bound)
        return int(np.count_nonzero(np.asarray(lam) <= x))

    il = count_le(vl)
    count = max(min(count_le(vu) - il, n_own - il), 0)
    return il, count, min(il, n_own - K)


def compact_rule(il, count, start, K, w_slot, z_slot=None):
    """The slot after k_window_compact: w_slot (K), z_slot (K, n) hold eigenpairs start .. start + K - 1."""
    off = min(max(il - start, 0), K)
    keep = min(count, K - off)
    w = np.full(K, np.nan)
    w[:keep] = w_slot[off:off + keep]
    if z_slot is None:
        return w, None
    z = np.zeros_like(z_slot)
    z[:keep] = z_slot[off:off + keep]
    return w, z


# ---- the staged debug entry ------------------------------------------------------------------------------------------------
SC_ERR_INVALID_ARG = 1


def debug_lib():
    from tests import stage_ratios as sr

    L = sr.debug_lib()
    L.sc_dbg_partial_tridiag_host.restype = C.c_int
    L.sc_dbg_partial_tridiag_host.argtypes = [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_double, C.c_double, C.c_int] + \
        [C.c_void_p] * 4
    return L


def _ptr(x):
    return None if x is None else C.c_void_p(x.ctypes.data)


def partial_raw(L, ctx, d, e, il=0, m=1, window=None, f=None, own=None, vectors=True):
    """The library's return code and (w (batch, m), Z (batch, n, m) or None, win (batch, 4) or None, count or None).
    window: None for the index range il .. il + m - 1, or (vl, vu, K)."""
    d = np.ascontiguousarray(np.atleast_2d(d), dtype=np.float64)
    e = np.ascontiguousarray(np.atleast_2d(e), dtype=np.float64)
    batch, n = d.shape
    assert e.shape == d.shape
    vl, vu = 0.0, 0.0
    if window is not None:
        vl, vu, m = window
    f = None if f is None else np.ascontiguousarray(np.broadcast_to(np.asarray(f, dtype=np.float64), (batch,)))
    own = None if own is None else np.ascontiguousarray(np.broadcast_to(np.asarray(own, dtype=np.int32), (batch,)))
    mm = max(int(m), 1)
    w = np.full((batch, mm), -777.0)
    z = np.full((batch, mm, n), -777.0) if vectors else None
    win = np.full((batch, 4), -777, dtype=np.int32) if window is not None else None
    count = np.full(batch, -777, dtype=np.int64) if window is not None else None
    rc = L.sc_dbg_partial_tridiag_host(ctx.handle, _ptr(d), _ptr(e), _ptr(f), _ptr(own), n, batch,
                                       1 if window is not None else 0, int(il), int(m), float(vl), float(vu),
                                       1 if vectors else 0, _ptr(w), _ptr(z), _ptr(win), _ptr(count))
    if rc != 0:
        return rc, None
    if z is not None:
        z = np.ascontiguousarray(z.transpose(0, 2, 1))
    return rc, (w, z, win, count)


def partial_host(L, ctx, d, e, **kw):
    rc, out = partial_raw(L, ctx, d, e, **kw)
    ctx.check(rc)
    return out
