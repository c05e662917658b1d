"""
What tests/test_subsystem_batch_host.py and tests/test_subsystem_batch_gpu.py share: the members of the test family, the
padded NumPy specification of the batched subsystem reduction, and the pinned error of that specification.

Members.  Five structures ``subsystem_model.synthetic_coord(N, seed)`` with a common core of ``N_S`` = 12 atoms and
environments of 0 / 1 / 21 / 22 / 44 atoms, i.e. H_ee of order 0 / 3 / 63 / 66 / 132: no environment, the smallest one, one
column below and two above the 64-column diagonal block of the Cholesky solver, and a third diagonal block with a panel
solve.  The core atoms of a member are ``default_rng(seed).choice(N, N_S)`` UNSORTED: the order of the columns is the
alignment's.  Force fields alternate between ``InvariantForceField(13)`` and ``HinsenForceField()``.

Specification.  ``subsystem_model.effective_hessian`` per member on the oracle's matrix; :func:`padded_effective_hessian`
is the same on the slot the device works on, ``diag(H_ee, I)`` with zero pad rows of H_es.  The gate of a comparison is
``subsystem_model.gate``: 8 x the specification's own float64-against-longdouble error (pinned in :data:`SPEC_ERROR`, measured
by tests/test_subsystem_batch_host.py) with the floor ``n eps scale``.
"""
import functools

import numpy as np

from tests import subsystem_model as sm

N_S = 12
# (N atoms, force field, seed of coordinates and core choice)
MEMBERS = ((12, "invariant", 11), (13, "hinsen", 12), (33, "invariant", 13), (34, "hinsen", 14), (56, "invariant", 15))
N_ENV = tuple(n - N_S for n, _, _ in MEMBERS)
ENV_ORDER = max(N_ENV)

# max |H_eff(float64 specification) - H_eff(longdouble specification)| / (3 N_S eps max|H_eff|) per member, measured by
# tests/test_subsystem_batch_host.py::test_specification_error_is_pinned (which fails when a measurement exceeds its entry).
# Member 0 has no environment: its H_eff is H itself and the error is exactly 0.
SPEC_ERROR = (0.0, 0.0060, 0.017, 0.10, 0.015)


@functools.lru_cache(maxsize=None)
def member_inputs(index):
    """(coord (N, 3), core atom indices (N_S,) unsorted, force-field name) of MEMBERS[index]; read-only."""
    n, ff, seed = MEMBERS[index]
    coord = sm.synthetic_coord(n, seed)
    system = np.random.default_rng(seed).choice(n, N_S, replace=False).astype(np.int64)
    coord.setflags(write=False)
    system.setflags(write=False)
    return coord, system, ff


def oracle_hessian(coord, ff, dim=3):
    from oracle import enm_oracle as orc

    return (orc.compute_hessian if dim == 3 else orc.compute_kirchhoff)(np.asarray(coord), sm.oracle_ff(ff))[0]


@functools.lru_cache(maxsize=None)
def member_matrix(index, dim=3):
    h = oracle_hessian(member_inputs(index)[0], member_inputs(index)[2], dim)
    h.setflags(write=False)
    return h


def partition(n, system):
    """subsystem_model.partition, with an empty environment allowed."""
    idx = np.asarray(system).astype(np.int64)
    assert len(idx) and len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < n
    return idx, np.setdiff1d(np.arange(n), idx)


def effective_hessian(h, system, env, dim, inv_sqrt_mass=None):
    """(H_eff, L, Y) as subsystem_model.effective_hessian; without environment H_eff = H_ss and L, Y are empty."""
    if len(env) == 0:
        hss = sm.blocks(h, system, env, dim, inv_sqrt_mass)[0]
        return np.array(hss), np.zeros((0, 0), dtype=h.dtype), np.zeros((0, len(hss)), dtype=h.dtype)
    return sm.effective_hessian(h, system, env, dim, inv_sqrt_mass)


def padded_blocks(h, system, env, dim, env_order, inv_sqrt_mass=None):
    """(H_ss, H_es, H_ee) of the slot: H_ee -> diag(H_ee, I), H_es gets zero pad rows."""
    hss, hes, hee = sm.blocks(h, system, env, dim, inv_sqrt_mass)
    me, own = dim * env_order, dim * len(env)
    assert own <= me
    pes = np.zeros((me, hss.shape[0]), dtype=h.dtype)
    pee = np.eye(me, dtype=h.dtype)
    pes[:own] = hes
    pee[:own, :own] = hee
    return hss, pes, pee


def padded_effective_hessian(h, system, env, dim, env_order, inv_sqrt_mass=None):
    """(H_eff, L, Y) of the padded slot, by the same unblocked algorithms."""
    hss, hes, hee = padded_blocks(h, system, env, dim, env_order, inv_sqrt_mass)
    l = sm.cholesky(hee)
    y = sm.forward(l, hes)
    return hss - y.T @ y, l, y


def spec_of(h, system, dim=3, inv_sqrt_mass=None):
    """The specification record of one member on its full matrix h."""
    n = len(h) // dim
    s, e = partition(n, system)
    heff, l, y = effective_hessian(h, s, e, dim, inv_sqrt_mass)
    w = np.linalg.eigvalsh(0.5 * (heff + heff.T))
    return dict(h=h, s=s, e=e, heff=heff, l=l, y=y, w=w, n=dim * n)


@functools.lru_cache(maxsize=None)
def member_spec(index):
    rec = spec_of(member_matrix(index), member_inputs(index)[1])
    for a in rec.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return rec


def pinned(index, m, top):
    """The specification's pinned absolute error of member `index` for a quantity of magnitude `top`."""
    return SPEC_ERROR[index] * m * sm.EPS * top


# ---- the fit family: one structure in three poses, and a perturbed copy ------------------------------------------------------------
def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


POSES = (((0.0, 0.0, 1.0), 0.0, (0.0, 0.0, 0.0)), ((1.0, 2.0, -0.5), 1.1, (7.0, -3.0, 2.0)), ((-0.3, 0.4, 1.0), 2.5, (-11.0, 5.0, 9.0)))
PERTURBATION = 0.05


@functools.lru_cache(maxsize=None)
def fit_family():
    """(list of four coordinate arrays (34, 3), the core indices): member 3 in POSES, and a copy with noise of 0.05."""
    coord, system, _ = member_inputs(3)
    out = [coord @ rotation(ax, ang).T + np.asarray(t) for ax, ang, t in POSES]
    out.append(coord + PERTURBATION * np.random.RandomState(7).randn(*coord.shape))
    for c in out:
        c.setflags(write=False)
    return out, system
