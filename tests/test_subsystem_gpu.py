"""
GPU tests of the subsystem (VSA) modes: the partitioned assembly and the reduction of csrc/subsystem.hip on the Cholesky
solver of csrc/potrf.hip, through the public :class:`springcraft_amd.Subsystem`.

Cases (tests/subsystem_model.py): N = 24 / 40 / 66 / 110 / 150 atoms of ``synthetic_coord(N, seed)`` with n_s = 12 / 18 / 23 /
40 / 21 system atoms drawn by ``default_rng(seed).choice``, sorted, under ``InvariantForceField(13)`` or
``HinsenForceField()``.  NumPy on the oracle's Hessian gives H_ee of orders 36 / 66 / 129 / 210 / 387 with condition numbers 17
- 830 and smallest eigenvalue >= 0.76; H_eff keeps six eigenvalues <= 2e-13 with w_6 / w_max >= 3.7e-4; the float64
specification is within 0.0074 - 0.024 of 3 n_s eps max|H_eff| of its longdouble evaluation and the unblocked factor's
ratio is <= 0.019 (tests/test_subsystem_host.py asserts all of this without a GPU).  dim 1 runs on N = 24 with n_s = 23
(n_e = 1), N = 110 with n_s = 45 (n_e = 65: one inner block and one row) and N = 66 with n_s = 23.

The reference throughout is the float64 specification on the ORACLE's matrix (``oracle.enm_oracle``), and independently the
package's own :class:`PairOperator` on the full network.

Gates: ``subsystem_model.gate`` = max(8 x the specification's pinned error, n eps scale) with n = dim N and scale the largest
magnitude of the quantity compared; on these inputs the floor governs.  The assembled blocks are held to the assembly's
existing gate 1e-12 max|ref|; eigenvector residuals and orthogonality to the eigensolver's existing gates
(``tests.util.check_eigenvectors``: 1e-5 and 1e-8).  Every comparison prints measured / gate.
"""
import numpy as np
import pytest

from tests import subsystem_model as sm
from tests.util import check_eigenvectors

pytestmark = pytest.mark.gpu

CASE_IDS = range(len(sm.CASES))


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


_CACHE = {}


def solved_case(sc, index):
    """(Subsystem after solve() and finish(), specification record) of CASES[index]: built once, read-only."""
    if index not in _CACHE:
        coord, system, ff = sm.case_inputs(index)
        sub = sc.Subsystem(coord, sm.package_ff(sc, ff), system)
        sub.solve()
        sub.finish()
        _CACHE[index] = (sub, spec_of(index))
    return _CACHE[index]


def spec_of(index, dim=3, inv_sqrt_mass=None):
    coord, system, _ = sm.case_inputs(index) if dim == 3 else sm.dim1_inputs(index)
    h = sm.oracle_matrix(index, dim)
    s, e = sm.partition(len(coord), system)
    heff, l, y = sm.effective_hessian(h, s, e, dim, inv_sqrt_mass)
    w, v = np.linalg.eigh(heff)
    rec = dict(h=h, s=s, e=e, heff=heff, l=l, y=y, w=w, n=dim * len(coord))
    for a in rec.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return rec


def within(name, got, ref, n, scale, pinned=0.0):
    g = sm.gate(pinned, n, scale)
    err = float(np.abs(np.asarray(got) - np.asarray(ref)).max())
    print(f"{name}: measured / gate = {err / g:.3f}")
    assert err <= g, (name, err, g)


# ---- 1. assembly ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", CASE_IDS)
def test_blocks_match_the_oracle(sc, index):
    coord, system, ff = sm.case_inputs(index)
    sub = sc.Subsystem(coord, sm.package_ff(sc, ff), system)
    first = [t.cpu().numpy() for t in sub.blocks()]
    second = [t.cpu().numpy() for t in sub.blocks()]
    s, e = sm.partition(len(coord), system)
    ref = sm.blocks(sm.oracle_matrix(index), s, e, 3)
    for name, a, b, r in zip(("H_ss", "H_es", "H_ee"), first, second, ref):
        print(f"{name}: max |got - ref| / max|ref| = {np.abs(a - r).max() / np.abs(r).max():.3e}")
        assert a.shape == r.shape and np.allclose(a, r, rtol=0, atol=1e-12 * np.abs(r).max())
        assert np.array_equal(a, b), f"{name} differs between two calls"
    assert np.array_equal(first[0], first[0].T) and np.array_equal(first[2], first[2].T)


# ---- 2. reduction and modes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", CASE_IDS)
def test_effective_hessian_and_spectrum(sc, index):
    sub, spec = solved_case(sc, index)
    heff = sub.effective_hessian().cpu().numpy()
    again = sub.effective_hessian().cpu().numpy()
    top = np.abs(spec["heff"]).max()
    pinned = sm.SPEC_ERROR[index] * sub.m * sm.EPS * top
    assert np.array_equal(heff, heff.T) and np.array_equal(heff, again)
    within("H_eff", heff, spec["heff"], spec["n"], top, pinned)
    w, v = sub.w[0].cpu().numpy(), sub.v[0].cpu().numpy()
    assert w.shape == (sub.m,) and v.shape == (sub.m, sub.m)
    within("w", w, spec["w"], spec["n"], np.abs(spec["w"]).max(), pinned)
    within("trivial w", w[:6], 0.0, spec["n"], np.abs(spec["w"]).max(), pinned)
    assert spec["w"][6] >= 3e-4 * spec["w"][-1]
    check_eigenvectors(heff, w, v)


def test_index_subset_gives_the_same_rows(sc):
    sub, spec = solved_case(sc, 2)
    w_full, v_full = sub.w[0, 6:16].cpu().numpy(), sub.v[0, 6:16].cpu().numpy()
    coord, system, ff = sm.case_inputs(2)
    part = sc.Subsystem(coord, sm.package_ff(sc, ff), system)
    w, v = part.eigen(subset_by_index=(6, 15))
    assert w.shape == (10,) and v.shape == (10, part.m)
    scale = np.abs(spec["w"]).max()
    within("subset w", w, w_full, spec["n"], scale)
    v = v * np.sign((v * v_full).sum(axis=1))[:, None]
    # an eigenvector moves by the backward error over its gap: the rows are compared as the eigensolver's tests compare them
    gap = np.diff(spec["w"][5:17]).min()
    assert np.abs(v - v_full).max() <= 1e-8 * scale / gap


@pytest.mark.parametrize("index", CASE_IDS)
def test_full_modes_against_the_pair_operator(sc, torch, index):
    """Independent of the specification: H x of the full network vanishes at the environment and is w v at the system."""
    sub, spec = solved_case(sc, index)
    coord, system, ff = sm.case_inputs(index)
    x = sub.full_modes()[6:]
    w, v = sub.w[0, 6:], sub.v[0, 6:]
    assert tuple(x.shape) == (sub.m - 6, 3 * len(coord))
    op = sc.PairOperator(coord, sm.package_ff(sc, ff))
    hx = op.apply(x.contiguous()).view(len(x), len(coord), 3)
    scale = np.abs(spec["h"]).max() * float(x.abs().max())
    s = torch.from_numpy(np.asarray(spec["s"])).cuda()
    e = torch.from_numpy(np.asarray(spec["e"])).cuda()
    n = spec["n"]
    within("H x at the environment", hx[:, e].cpu().numpy(), 0.0, n, scale)
    within("H x at the system", hx[:, s].reshape(len(x), -1).cpu().numpy(), (w[:, None] * v).cpu().numpy(), n, scale)
    within("x^T H x", (x * hx.view(len(x), -1)).sum(dim=1).cpu().numpy(), w.cpu().numpy(), n, scale)
    # and the follow motion of given rows is the specification's
    xe = sub.environment_displacement(sub.v[0, 6:9].contiguous()).cpu().numpy()
    ref = sm.follow(spec["l"], spec["y"], sub.v[0, 6:9].cpu().numpy())
    within("follow motion", xe, ref, n, max(np.abs(ref).max(), 1.0))


def test_scrambled_system_order_permutes(sc):
    coord, system, ff = sm.case_inputs(1)
    perm = np.random.RandomState(0).permutation(len(system))
    base = solved_case(sc, 1)[0].effective_hessian().cpu().numpy()
    sub = sc.Subsystem(coord, sm.package_ff(sc, ff), np.asarray(system)[perm])
    got = sub.effective_hessian().cpu().numpy()
    d = sm.dof(perm, 3)
    spec = solved_case(sc, 1)[1]
    within("permuted H_eff", got, base[np.ix_(d, d)], spec["n"], np.abs(base).max())
    # the same with a mask
    mask = np.zeros(len(coord), dtype=bool)
    mask[system] = True
    assert np.array_equal(sc.Subsystem(coord, sm.package_ff(sc, ff), mask).effective_hessian().cpu().numpy(), base)


@pytest.mark.parametrize("index", [0, 3])
def test_masses(sc, index):
    coord, system, ff = sm.case_inputs(index)
    m = sm.masses_of(len(coord))
    spec = spec_of(index, inv_sqrt_mass=1.0 / np.sqrt(m[system]))
    sub = sc.Subsystem(coord, sm.package_ff(sc, ff), system, masses=m)
    top = np.abs(spec["heff"]).max()
    within("T H_eff T", sub.effective_hessian().cpu().numpy(), spec["heff"], spec["n"], top,
           sm.SPEC_ERROR[index] * sub.m * sm.EPS * top)
    w, _ = sub.eigen()
    within("w with masses", w, spec["w"], spec["n"], np.abs(spec["w"]).max())


@pytest.mark.parametrize("index", range(len(sm.CASES_DIM1)))
def test_dim_1(sc, index):
    coord, system, ff = sm.dim1_inputs(index)
    spec = spec_of(index, dim=1)
    sub = sc.Subsystem(coord, sm.package_ff(sc, ff), system, dim=1)
    assert sub.m == len(system) and sub.m_env == len(coord) - len(system)
    blocks = [t.cpu().numpy() for t in sub.blocks()]
    for a, r in zip(blocks, sm.blocks(spec["h"], spec["s"], spec["e"], 1)):
        assert np.allclose(a, r, rtol=0, atol=1e-12 * np.abs(r).max())
    heff = sub.effective_hessian().cpu().numpy()
    top = np.abs(spec["heff"]).max()
    assert np.array_equal(heff, heff.T)
    within("dim 1 H_eff", heff, spec["heff"], spec["n"], top, 0.03 * sub.m * sm.EPS * top)
    w, v = sub.eigen()
    within("dim 1 w", w, spec["w"], spec["n"], np.abs(spec["w"]).max())
    within("dim 1 trivial w", w[:1], 0.0, spec["n"], np.abs(spec["w"]).max())
    check_eigenvectors(heff, w, v)
    with pytest.raises(ValueError):
        sub.prs()


# ---- 3. the consumers run unchanged ---------------------------------------------------------------------------------------------
def test_consumers_equal_a_batch_solver_on_the_same_modes(sc, torch):
    from springcraft_amd.batch import DeviceBatchSolver

    sub, _ = solved_case(sc, 2)
    coord, system, ff = sm.case_inputs(2)
    other = DeviceBatchSolver(sub.n_atoms, 1, sm.package_ff(sc, ff))
    other.w, other.v = sub.w.clone(), sub.v.clone()
    force = torch.from_numpy(np.random.RandomState(1).randn(1, sub.n_atoms, 3)).cuda()
    for name, args in (("mean_square_fluctuation", ()), ("dcc", ()), ("prs", ()), ("linear_response", (force,))):
        a, b = getattr(sub, name)(*args), getattr(other, name)(*args)
        assert a.shape[:2] == (1, sub.n_atoms) and torch.equal(a, b), name
    assert tuple(sub.generalized_correlation().shape) == (1, sub.n_atoms, sub.n_atoms)
    assert abs(float(sub.rmsip(other=other)) - 1.0) <= 1e-12
    sub.finish()


def test_model_methods_build_the_same_solver(sc):
    coord, system, ff = sm.case_inputs(0)
    mask = np.zeros(len(coord), dtype=bool)
    mask[system] = True
    base = solved_case(sc, 0)[0].effective_hessian().cpu().numpy()
    via = sc.ANM(coord, sm.package_ff(sc, ff)).subsystem(mask)
    assert isinstance(via, sc.Subsystem) and via.dim == 3
    assert np.array_equal(via.effective_hessian().cpu().numpy(), base)
    m = sm.masses_of(len(coord))
    direct = sc.Subsystem(coord, sm.package_ff(sc, ff), system, masses=m).effective_hessian().cpu().numpy()

    class Atoms:   # (an ANM wants an atom container for a mass array)
        def __init__(self, c):
            self.coord = c

        def array_length(self):
            return len(self.coord)

    assert np.array_equal(sc.ANM(Atoms(coord), sm.package_ff(sc, ff), masses=m).subsystem(system).effective_hessian().cpu().numpy(),
                          direct)
    g = sc.GNM(coord, sm.package_ff(sc, ff)).subsystem(system)
    assert g.dim == 1 and g.m == len(system)


# ---- 4. the single-structure C entries, which the Python solver no longer calls -------------------------------------------------
@pytest.mark.parametrize("with_masses", [False, True])
@pytest.mark.parametrize("dim", [3, 1])
def test_single_entries_equal_the_solver_bit_for_bit(sc, torch, dim, with_masses):
    """
    sc_dev_subsystem_blocks_f64 / _reduce_f64 / _follow_f64 called directly on a solver's own device inputs: dim 3 on case 1
    (H_ee of order 66) and dim 1 on the second dim-1 case (order 65), so the factorisation crosses a diagonal-block boundary.
    """
    import ctypes as C

    from springcraft_amd import _hip

    coord, system, ff = sm.case_inputs(1) if dim == 3 else sm.dim1_inputs(1)
    masses = sm.masses_of(len(coord)) if with_masses else None
    sub = sc.Subsystem(coord, sm.package_ff(sc, ff), system, masses=masses, dim=dim)
    m, me = sub.m, sub.m_env
    assert me > 64 and (sub.inv_sqrt_mass is not None) == with_masses
    L, h = sub._L, sub.ctx.handle
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    hss, hes, hee = sub._empty((m, m)), sub._empty((me, m)), sub._empty((me, me))
    info = torch.ones(1, dtype=torch.int64, device="cuda")

    def blocks(n_atoms=sub.n_total, n_s=sub.n_atoms, n_e=sub.n_env):
        return L.sc_dev_subsystem_blocks_f64(h, p(sub._coord), n_atoms, dim, p(sub._pairs), sub.n_pairs, p(sub._gamma),
                                             p(sub._row_start), p(sub._group), p(sub._pos), n_s, n_e, p(sub.inv_sqrt_mass),
                                             p(hss), p(hes), p(hee))

    assert blocks() == _hip.SC_OK
    for got, ref in zip((hss, hes, hee), sub.blocks()):
        assert np.array_equal(got.cpu().numpy(), ref.cpu().numpy())
    assert torch.equal(hss, hss.t()) and torch.equal(hee, hee.t())
    assert L.sc_dev_subsystem_reduce_f64(h, p(hss), p(hes), p(hee), m, me, p(info)) == _hip.SC_OK
    assert np.array_equal(hss.cpu().numpy(), sub.effective_hessian().cpu().numpy())
    assert torch.equal(hss, hss.t()) and int(info.cpu()[0]) == 0
    rows = torch.from_numpy(np.random.RandomState(dim).randn(3, m)).cuda()
    xe = sub._empty((3, me))
    assert L.sc_dev_subsystem_follow_f64(h, p(hee), p(hes), m, me, p(rows), 3, p(xe)) == _hip.SC_OK
    assert np.array_equal(xe.cpu().numpy(), sub.environment_displacement(rows).cpu().numpy())
    # the single entries keep their own refusals: an empty environment, and groups that do not make up the atoms
    bad = _hip.SC_ERR_INVALID_ARG
    assert blocks(n_s=sub.n_total, n_e=0) == bad and blocks(n_s=sub.n_atoms - 1) == bad and blocks(n_atoms=sub.n_total + 1) == bad
    assert L.sc_dev_subsystem_reduce_f64(h, p(hss), p(hes), p(hee), m, 0, p(info)) == bad
    sub.finish()


# ---- 5. refusals and failures -------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(sc):
    coord, system, ff = sm.case_inputs(0)
    field = sm.package_ff(sc, ff)
    n = len(coord)
    for bad in ([0, 0, 1], [0, n], [-1, 2], [], np.zeros(n, dtype=bool), np.zeros(n - 1, dtype=bool), [0.5, 1.0]):
        with pytest.raises(ValueError):
            sc.Subsystem(coord, field, np.asarray(bad))
    with pytest.raises(ValueError, match="use ANM"):
        sc.Subsystem(coord, field, np.arange(n))
    with pytest.raises(ValueError, match="dim"):
        sc.Subsystem(coord, field, system, dim=2)
    # an environment atom without any contact, and a system that shares no spring with its environment
    far = np.array(coord)
    env = sm.partition(n, system)[1]
    far[env[0]] += 1000.0
    lonely = sc.Subsystem(far, field, system)
    with pytest.raises(ValueError, match="without any contact"):
        lonely.solve()
    with pytest.raises(ValueError, match="without any contact"):
        lonely.effective_hessian()
    apart = np.array(coord)
    apart[system] += 1000.0
    with pytest.raises(ValueError, match="shares no spring"):
        sc.Subsystem(apart, field, system).solve()
    assert lonely.w is None and lonely.matrix is None
    lonely.finish()   # nothing was enqueued, nothing is reported
    # asymmetric constants, as PairOperator refuses them
    class Lopsided(sc.InvariantForceField):
        def force_constant(self, atom_i, atom_j, sq_distance):
            return np.where(atom_i < atom_j, 1.0, 2.0)

    with pytest.raises(ValueError, match="asymmetric"):
        sc.Subsystem(coord, Lopsided(sm.CUTOFF), system)


def test_singular_environment_raises_in_finish(sc):
    """
    One environment atom keeps a single spring, along x exactly: its diagonal block of H_ee is gamma diag(1, 0, 0) and nothing
    else touches its y and z rows, so the pivot of its y column is exactly 0 whatever the order of the sums.
    """
    coord, system, ff = sm.case_inputs(0)
    coord = np.array(coord)
    n = len(coord)
    env = sm.partition(n, system)[1]
    atom, neighbour = env[3], system[0]
    coord[atom] = coord[neighbour] + np.array([3.0, 0.0, 0.0])
    d2 = ((coord[:, None, :] - coord[None, :, :]) ** 2).sum(axis=-1)
    off = np.array([[atom, j] for j in range(n) if j not in (atom, neighbour) and d2[atom, j] <= sm.CUTOFF ** 2])
    field = sc.PatchedForceField(sc.InvariantForceField(sm.CUTOFF), contact_pair_off=off)
    sub = sc.Subsystem(coord, field, system)
    sub.solve()
    with pytest.raises(np.linalg.LinAlgError, match="positive definite"):
        sub.finish()
    assert int(sub._info.cpu()[0]) == 3 * 3 + 2    # 1 + the y column of the environment's fourth atom
    assert bool(sub.w.isnan().all())
    sub.finish()                                   # reported once
    sub.solve()                                    # the solver still works: the same failure, reported again
    with pytest.raises(np.linalg.LinAlgError):
        sub.finish()
    healthy = sc.Subsystem(*[sm.case_inputs(0)[0], sm.package_ff(sc, "invariant"), system])
    w, _ = healthy.eigen()
    assert np.isfinite(w).all()
