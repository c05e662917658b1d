"""
The backward-error ratios LAPACK's own test programs apply to the stages of a symmetric eigensolver (dsyt21 for dsytrd,
dsbt21 for dsbtrd, dstt21 for dstedc), restated in float64 NumPy, the inputs they are applied to here, and the ctypes
bindings of the staged debug entries sc_dbg_reduce_host / sc_dbg_stedc_host (include/springcraft_hip_debug.h).

With ulp = np.finfo(float).eps and the 1-norm:

    recon(A, Q, M) = |A - Q M Q^T|_1 / (n |A|_1 ulp)        (0 for A = 0 when the difference is 0 too)
    orth(Q)        = |I - Q Q^T|_1 / (n ulp)

M is the tridiagonal T, the band matrix B or diag(w).  A stage that is backward stable keeps both at a modest multiple of
1; LAPACK's test drivers accept up to GATE = 50 (the threshold line of TESTING/sep.in in the LAPACK distribution, kept
here as the convention).  LAPACK itself stays below GATE / 10 on every input of this file
(tests/test_stage_ratios_host.py); the GPU stages are held to GATE (tests/test_stage_ratios_gpu.py).
"""
import ctypes as C

import numpy as np

from tests.util import degenerate_members, glued_wilkinson

ULP = np.finfo(float).eps
GATE = 50.0
LAPACK_GATE = GATE / 10.0
BAND = 64                 # half-width of the stage-1 band
LDAB = 2 * BAND           # rows of its storage

MIXED = ["random", "identity", "band64", "band65", "rank1", "gluedW", "big"]      # (the order degenerate_members keeps)
SEED = 1


def norm1(a):
    return np.abs(a).sum(axis=0).max() if a.size else 0.0


def recon(a, q, m):
    """|A - Q M Q^T|_1 / (n |A|_1 ulp); q holds the factor's columns as columns."""
    n = len(a)
    na = norm1(a)
    diff = norm1(a - q @ m @ q.T)
    if na == 0.0:
        return 0.0 if diff == 0.0 else np.inf
    # (dsyt21's guard for |A| << |difference| is not needed: it only matters far above the gate)
    return diff / na / (n * ULP)


def orth(q):
    n = len(q)
    return norm1(np.eye(n) - q @ q.T) / (n * ULP)


# ---- the same two formulas on float64 torch tensors (torch.matmul: on a device tensor rocBLAS, which shares nothing with the
# kernels under test), for orders at which the NumPy triple products take too long
def norm1_t(a):
    return float(a.abs().sum(dim=0).max()) if a.numel() else 0.0


def recon_t(a, q, m):
    """recon(a, q, m) of float64 torch tensors on one device; q holds the factor's columns as columns."""
    import torch

    assert a.dtype == q.dtype == m.dtype == torch.float64
    n = a.shape[0]
    na = norm1_t(a)
    diff = norm1_t(a - q @ m @ q.T)
    if na == 0.0:
        return 0.0 if diff == 0.0 else np.inf
    return diff / na / (n * ULP)


def orth_t(q):
    import torch

    assert q.dtype == torch.float64
    n = q.shape[0]
    return norm1_t(torch.eye(n, dtype=q.dtype, device=q.device) - q @ q.T) / (n * ULP)


def tridiagonal(d, e):
    """Dense T from d (n) and e (n or n - 1 entries; only the first n - 1 count)."""
    n = len(d)
    e = np.asarray(e)[:n - 1]
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def band_matrix(ab):
    """Dense symmetric B from band storage ab (n x LDAB as the debug entry returns it: ab[j, k] = B(j + k, j))."""
    n = len(ab)
    b = np.zeros((n, n))
    for k in range(min(BAND, n - 1) + 1):
        idx = np.arange(n - k)
        b[idx + k, idx] = ab[idx, k]
        b[idx, idx + k] = ab[idx, k]
    return b


def band_beyond(ab):
    """Largest |entry| of the band storage beyond half-width BAND: must be exactly 0."""
    return float(np.abs(ab[:, BAND + 1:]).max())


# ---- inputs ------------------------------------------------------------------------------------------------------------
_cache = {}


def random_sym(n):
    if ("random", n) not in _cache:
        g = np.random.RandomState(n).randn(n, n)
        a = g + g.T
        a.setflags(write=False)
        _cache["random", n] = a
    return _cache["random", n]


def mixed_batch(n):
    """The members of tests.util.degenerate_members that produce tau = 0 reflectors and exact zeros, next to a control."""
    if ("mixed", n) not in _cache:
        members, _ = degenerate_members(n, SEED, names=MIXED)
        assert [name for name, _ in members] == MIXED
        a = np.stack([m for _, m in members])
        a.setflags(write=False)
        _cache["mixed", n] = a
    return MIXED, _cache["mixed", n]


TRIDIAGONALS = ["toeplitz", "wilkinson", "glued1e-4", "glued1e-12", "graded", "torn", "equal", "negative", "identity"]


def tridiagonal_inputs(n):
    """name -> (d, e) of order n, e with n entries (the last one 0 and not part of the matrix)."""
    rs = np.random.RandomState(1000 + n)
    out = {}

    def put(name, d, e):
        ee = np.zeros(n)
        ee[:n - 1] = np.asarray(e, dtype=float)[:n - 1]
        out[name] = (np.asarray(d, dtype=float).copy(), ee)

    def glued(glue):
        # Wilkinson blocks W21+ glued by `glue`, cut to order n
        blocks = n // 21 + 1
        d, e = glued_wilkinson(blocks, glue)
        return d[:n], np.concatenate([e, [0.0]])[:n]

    put("toeplitz", np.full(n, 2.0), np.ones(n))
    put("wilkinson", np.abs(np.arange(n) - (n - 1) / 2.0), np.ones(n))
    put("glued1e-4", *glued(1e-4))
    put("glued1e-12", *glued(1e-12))
    put("graded", np.logspace(0, -15, n), np.logspace(0, -15, n) * 0.5)
    e = rs.randn(n)
    e[2::3] = 0.0
    put("torn", rs.randn(n), e)
    put("equal", np.ones(n), np.full(n, 1e-9))
    put("negative", rs.randn(n), -np.abs(rs.randn(n)))
    put("identity", np.ones(n), np.zeros(n))
    assert list(out) == TRIDIAGONALS
    return out


def toeplitz_exact(n):
    return 2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1))


# ---- the staged debug entries --------------------------------------------------------------------------------------------
Q_ALL, Q_ONE, Q_TWO = 0, 1, 2


def debug_lib():
    from springcraft_amd import _hip

    L = _hip.lib()
    L.sc_dbg_set_chase.restype = C.c_int
    L.sc_dbg_set_chase.argtypes = [C.c_void_p, C.c_int, C.c_int]
    for f in (L.sc_dbg_set_panel_coop, L.sc_dbg_set_panel_coop_fail):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_int]
    L.sc_dbg_set_resident.restype = C.c_int
    L.sc_dbg_set_resident.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.sc_dbg_reduce_host.restype = C.c_int
    L.sc_dbg_reduce_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
    L.sc_dbg_stedc_host.restype = C.c_int
    L.sc_dbg_stedc_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sc_dbg_stedc_leaf_max.restype = C.c_int
    L.sc_dbg_stedc_leaf_max.argtypes = [C.c_int]
    return L


def reduce_raw(L, ctx, a, which, want_q=True, transpose=True):
    """The library's return code and (d, e, scale, band or None, Q or None, two_stage) of a batch a (batch, n, n); Q with
    the factor's columns as columns (transpose = False: as the entry returns it, the columns as rows -- no copy)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    batch, n, _ = a.shape
    d, e, scale = np.zeros((batch, n)), np.zeros((batch, n)), np.zeros(batch)
    band = np.full((batch, n, LDAB), np.nan)
    q = np.zeros((batch, n, n)) if want_q else None
    two = C.c_int(-1)
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)  # noqa: E731
    rc = L.sc_dbg_reduce_host(ctx.handle, p(a), n, batch, which, p(d), p(e), p(scale), p(band), p(q), C.byref(two))
    if rc != 0:
        return rc, None
    if q is not None and transpose:
        q = np.ascontiguousarray(q.transpose(0, 2, 1))
    return rc, (d, e, scale, band if two.value == 1 else None, q, two.value == 1)


def reduce_host(L, ctx, a, which, want_q=True, transpose=True):
    rc, out = reduce_raw(L, ctx, a, which, want_q, transpose)
    ctx.check(rc)
    return out


def stedc_host(L, ctx, d, e):
    """(w, Z) of the tridiagonal matrices d, e (batch, n each); Z with the eigenvectors as columns."""
    d = np.ascontiguousarray(d, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    batch, n = d.shape
    assert e.shape == d.shape
    w, z = np.zeros((batch, n)), np.zeros((batch, n, n))
    ctx.check(L.sc_dbg_stedc_host(ctx.handle, C.c_void_p(d.ctypes.data), C.c_void_p(e.ctypes.data), n, batch,
                                  C.c_void_p(w.ctypes.data), C.c_void_p(z.ctypes.data)))
    return w, np.ascontiguousarray(z.transpose(0, 2, 1))
