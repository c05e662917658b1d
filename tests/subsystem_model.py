"""
What tests/test_subsystem_host.py, tests/test_potrf_gpu.py and tests/test_subsystem_gpu.py share: the NumPy specification of
the Cholesky solver and of the subsystem reduction, the inputs, and the gates.

Specification.  :func:`cholesky`, :func:`forward` and :func:`backward` are the unblocked textbook algorithms in plain
arithmetic, so that they run in float64 and in ``np.longdouble``; :func:`effective_hessian` and :func:`follow` are built on
them exactly as the device code is built on its factorisation: ``L L^T = H_ee``, ``Y = L^-1 H_es``, ``H_eff = H_ss - Y^T Y``,
``x_e = -L^-T (Y x_s)``.  The device sums in blocks and on the matrix units where the specification sums in sequence.

Gates.  Factorisations and solves are held to LAPACK's test ratios (dpot01 / dpot02) in units of n ulp with the project's
stage-ratio gate :data:`RATIO_GATE` = 50 (tests/stage_ratios.py).  A subsystem result is compared with the float64
specification; how far that is from the truth is measured against its longdouble evaluation on the same inputs
(tests/test_subsystem_host.py measures it and checks it against :data:`SPEC_ERROR`), and the gate of a comparison is
``GATE_MULTIPLE`` times that error with the floor ``n eps scale``, n = dim N the order of the full matrix and scale the
largest magnitude of the quantity compared (as tests/ensemble_model.py).  On these inputs the floor governs.
"""
import functools

import numpy as np

EPS = 2.0 ** -52
GATE_MULTIPLE = 8
RATIO_GATE = 50.0

# (N atoms, n_s, force field, seed): coordinates synthetic_coord(N, seed), the system default_rng(seed).choice(N, n_s), sorted
CASES = ((24, 12, "invariant", 1), (40, 18, "hinsen", 2), (66, 23, "invariant", 3), (110, 40, "hinsen", 4),
         (150, 21, "invariant", 5))
CUTOFF = 13.0
# dim 1: (N, n_s, force field, seed, explicit system or None); n_e = 1 and n_e = 65 among them
CASES_DIM1 = ((24, 23, "invariant", 1), (110, 45, "hinsen", 4), (66, 23, "invariant", 3))

# max |H_eff(float64 specification) - H_eff(longdouble specification)| / (3 n_s eps max|H_eff|) per case, measured by
# tests/test_subsystem_host.py::test_specification_error_is_pinned (which fails when a measurement exceeds its entry)
SPEC_ERROR = (0.013, 0.024, 0.0075, 0.022, 0.0086)

POTRF_ORDERS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 129, 200, 513, 1030)
POTRF_CONDS = (1.0, 1e6, 1e12)
POTRS_Q = (1, 5, 64, 70)


def gate(measured, n, scale):
    return max(GATE_MULTIPLE * measured, n * EPS * scale)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def synthetic_coord(n, seed):
    return np.random.RandomState(seed).rand(n, 3) * 5.0 * n ** (1.0 / 3.0)


@functools.lru_cache(maxsize=None)
def case_inputs(index):
    """(coord (N, 3), system indices (n_s,) ascending, force-field name) of CASES[index]; read-only."""
    n, n_s, ff, seed = CASES[index]
    coord = synthetic_coord(n, seed)
    system = np.sort(np.random.default_rng(seed).choice(n, n_s, replace=False))
    coord.setflags(write=False)
    system.setflags(write=False)
    return coord, system, ff


@functools.lru_cache(maxsize=None)
def dim1_inputs(index):
    n, n_s, ff, seed = CASES_DIM1[index]
    coord = synthetic_coord(n, seed)
    system = np.sort(np.random.default_rng(seed).choice(n, n_s, replace=False))
    coord.setflags(write=False)
    system.setflags(write=False)
    return coord, system, ff


def oracle_ff(name):
    from oracle import enm_oracle as orc

    return orc.invariant_ff(CUTOFF) if name == "invariant" else orc.hinsen_ff()


def package_ff(sc, name):
    return sc.InvariantForceField(CUTOFF) if name == "invariant" else sc.HinsenForceField()


@functools.lru_cache(maxsize=None)
def oracle_matrix(index, dim=3):
    """The oracle's Hessian (dim 3) of CASES[index] or Kirchhoff matrix (dim 1) of CASES_DIM1[index]; read-only."""
    from oracle import enm_oracle as orc

    coord, _, ff = case_inputs(index) if dim == 3 else dim1_inputs(index)
    h = (orc.compute_hessian if dim == 3 else orc.compute_kirchhoff)(coord, oracle_ff(ff))[0]
    h.setflags(write=False)
    return h


def masses_of(n, seed=5):
    return np.random.RandomState(seed).uniform(50, 200, n)


@functools.lru_cache(maxsize=None)
def spd(n, cond, seed=0):
    """Q diag(lambda) Q^T with lambda spaced geometrically in [1 / cond, 1] and Q a random orthogonal matrix; symmetric, read-only."""
    rs = np.random.RandomState(100 + seed)
    q = np.linalg.qr(rs.randn(n, n))[0]
    lam = np.ones(n) if cond == 1.0 or n == 1 else cond ** (-np.arange(n) / (n - 1.0))
    a = (q * lam) @ q.T
    a = 0.5 * (a + a.T)
    a.setflags(write=False)
    return a


# ---- the specification ---------------------------------------------------------------------------------------------------------
def partition(n, system):
    """(system indices as given, environment indices ascending) with the checks of the product's subsystem_partition."""
    s = np.asarray(system)
    idx = np.nonzero(s)[0] if s.dtype == np.bool_ else s.astype(np.int64)
    assert len(idx) and len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < n and len(idx) < n
    env = np.setdiff1d(np.arange(n), idx)
    return idx, env


def dof(atoms, dim):
    return (dim * np.asarray(atoms)[:, None] + np.arange(dim)[None, :]).reshape(-1)


def cholesky(a):
    """Unblocked lower Cholesky factor in a's dtype (column by column, as the device's diagonal-block kernel); None at a pivot <= 0."""
    a = np.array(a)
    n = len(a)
    l = np.zeros_like(a)
    for j in range(n):
        p = a[j, j] - l[j, :j] @ l[j, :j]
        if not p > 0:
            return None
        l[j, j] = np.sqrt(p)
        l[j + 1:, j] = (a[j + 1:, j] - l[j + 1:, :j] @ l[j, :j]) / l[j, j]
    return l


def forward(l, b):
    """Y with L Y = B by forward substitution, in l's dtype."""
    y = np.array(b, dtype=l.dtype)
    for i in range(len(l)):
        y[i] = (y[i] - l[i, :i] @ y[:i]) / l[i, i]
    return y


def backward(l, y):
    """X with L^T X = Y by backward substitution."""
    x = np.array(y, dtype=l.dtype)
    for i in range(len(l) - 1, -1, -1):
        x[i] = (x[i] - l[i + 1:, i] @ x[i + 1:]) / l[i, i]
    return x


def blocks(h, system, env, dim, inv_sqrt_mass=None):
    """(H_ss, H_es, H_ee) of the full matrix; inv_sqrt_mass (n_s,) scales the system's rows and columns."""
    s, e = dof(system, dim), dof(env, dim)
    hss, hes, hee = h[np.ix_(s, s)], h[np.ix_(e, s)], h[np.ix_(e, e)]
    if inv_sqrt_mass is not None:
        t = np.repeat(np.asarray(inv_sqrt_mass, dtype=h.dtype), dim)
        hss, hes = hss * t[:, None] * t[None, :], hes * t[None, :]
    return hss, hes, hee


def effective_hessian(h, system, env, dim, inv_sqrt_mass=None):
    """(H_eff, L, Y) in h's dtype."""
    hss, hes, hee = blocks(h, system, env, dim, inv_sqrt_mass)
    l = cholesky(hee)
    y = forward(l, hes)
    return hss - y.T @ y, l, y


def follow(l, y, xs):
    """x_e (q, m_env) = -L^-T (Y x_s) for the rows xs (q, m)."""
    return -backward(l, y @ np.asarray(xs, dtype=l.dtype).T).T


# ---- LAPACK's test ratios ------------------------------------------------------------------------------------------------------------
def norm1(a):
    return np.abs(a).sum(axis=0).max()


def factor_ratio(a, l):
    """dpot01: |A - L L^T|_1 / (n eps |A|_1)."""
    l = np.tril(l)
    return norm1(a - l @ l.T) / (len(a) * EPS * norm1(a))


def solve_ratio(a, x, b):
    """dpot02: |A X - B|_1 / (|A|_1 |X|_1 n eps); a, x, b with x and b of shape (n, q)."""
    return norm1(a @ x - b) / (norm1(a) * norm1(x) * len(a) * EPS)


def triangular_ratio(t, x, b):
    """|T X - B|_1 / (|T|_1 |X|_1 n eps) for a triangular solve with the factor (dtrt02)."""
    return norm1(t @ x - b) / (norm1(t) * norm1(x) * len(t) * EPS)
