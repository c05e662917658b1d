"""
GPU tests of ensemble NMA on a common core: the batched partitioned assembly and the batched reduction of
csrc/subsystem.hip on the batched Cholesky solver, through the public :class:`springcraft_amd.SubsystemBatch`.

Members (tests/subsystem_batch_model.py): N = 12 / 13 / 33 / 34 / 56 atoms with a common core of 12 atoms in an unsorted
order, i.e. H_ee of order 0 / 3 / 63 / 66 / 132 in slots of order 132; tests/test_subsystem_batch_host.py asserts without a
GPU that every environment is connected and coupled (H_ee positive definite, smallest eigenvalue >= 0.5) and that
w_6 >= 3e-4 w_max.

The reference throughout is the float64 NumPy specification of tests/subsystem_model.py evaluated per member on the
ORACLE's matrix; the gate is ``subsystem_model.gate`` = max(8 x the specification's pinned error, n eps scale) with n = dim N
of the member (the floor governs on these inputs).  Assembled blocks are held to the assembly's gate 1e-12 max|ref|,
eigenvectors to ``tests.util.check_eigenvectors``, the consumers and the subspace comparisons to the models and gates of
their own test files.  Every comparison prints measured / gate.
"""
import ctypes as C

import numpy as np
import pytest

from tests import subsystem_batch_model as bm
from tests import subsystem_model as sm
from tests.util import check_eigenvectors

pytestmark = pytest.mark.gpu

ALL = (0, 1, 2, 3, 4)


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def make(sc, ids, **kw):
    kw.setdefault("fit", False)
    return sc.SubsystemBatch([bm.member_inputs(i)[0] for i in ids], [sm.package_ff(sc, bm.member_inputs(i)[2]) for i in ids],
                             [bm.member_inputs(i)[1] for i in ids], **kw)


_CACHE = {}


def solved(sc, ids=ALL, **kw):
    """SubsystemBatch of the members `ids` after solve() and finish(), with its H_eff, w, v on the host: built once, read-only."""
    key = (tuple(ids), tuple(sorted(kw.items())))
    if key not in _CACHE:
        s = make(sc, ids, **kw)
        heff = s.effective_hessian().cpu().numpy()
        s.solve()
        s.finish()
        host = heff, s.w.cpu().numpy(), s.v.cpu().numpy()
        for a in host:
            a.setflags(write=False)
        _CACHE[key] = (s,) + host
    return _CACHE[key]


def within(name, got, ref, n, scale, pinned=0.0):
    g = sm.gate(pinned, n, scale)
    err = float(np.abs(np.asarray(got) - np.asarray(ref)).max()) if np.size(got) else 0.0
    print(f"{name}: measured / gate = {err / g:.3f}")
    assert err <= g, (name, err, g)


# ---- 1. assembly ------------------------------------------------------------------------------------------------------------
def test_blocks_bits_pads_and_oracle(sc):
    s = make(sc, ALL)
    first = [t.cpu().numpy() for t in s.blocks()]
    second = [t.cpu().numpy() for t in s.blocks()]
    me = 3 * bm.ENV_ORDER
    assert first[0].shape == (5, 36, 36) and first[1].shape == (5, me, 36) and first[2].shape == (5, me, me)
    for a, b in zip(first, second):
        assert np.array_equal(a, b), "two calls differ"
    for i in ALL:
        coord, system, ff = bm.member_inputs(i)
        rec = bm.member_spec(i)
        own = 3 * bm.N_ENV[i]
        hss, hes, hee = first[0][i], first[1][i], first[2][i]
        ref = sm.blocks(rec["h"], rec["s"], rec["e"], 3)
        for name, got, r in zip(("H_ss", "H_es", "H_ee"), (hss, hes[:own], hee[:own, :own]), ref):
            if r.size:
                print(f"member {i} {name}: max |got - ref| / max|ref| = {np.abs(got - r).max() / np.abs(r).max():.3e}")
                assert got.shape == r.shape and np.allclose(got, r, rtol=0, atol=1e-12 * np.abs(r).max())
        # the pads: the identity on H_ee's pad diagonal, exact zeros everywhere else
        assert np.array_equal(hee[own:, own:], np.eye(me - own)) and not hee[own:, :own].any() and not hee[:own, own:].any()
        assert not hes[own:].any()
        assert np.array_equal(hss, hss.T) and np.array_equal(hee, hee.T)
        if own:   # the bits of the single solver on this member alone
            single = [t.cpu().numpy() for t in sc.Subsystem(coord, sm.package_ff(sc, ff), system).blocks()]
            assert np.array_equal(hss, single[0]) and np.array_equal(hes[:own], single[1])
            assert np.array_equal(hee[:own, :own], single[2])


# ---- 2. reduction and modes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", ALL)
def test_effective_hessian_and_spectrum(sc, index):
    s, heff, w, v = solved(sc)
    spec = bm.member_spec(index)
    top, wtop = np.abs(spec["heff"]).max(), np.abs(spec["w"]).max()
    assert heff.shape == (5, 36, 36) and w.shape == (5, 36) and v.shape == (5, 36, 36)
    assert np.array_equal(heff[index], heff[index].T)
    within(f"member {index} H_eff", heff[index], spec["heff"], spec["n"], top, bm.pinned(index, s.m, top))
    within(f"member {index} w", w[index], spec["w"], spec["n"], wtop, bm.pinned(index, s.m, top))
    within(f"member {index} trivial w", w[index, :6], 0.0, spec["n"], wtop, bm.pinned(index, s.m, top))
    assert spec["w"][6] >= 3e-4 * spec["w"][-1]
    check_eigenvectors(heff[index], w[index], v[index])
    assert int(s._info.cpu()[index]) == 0


# ---- 3. no environment ---------------------------------------------------------------------------------------------------------
def test_member_without_environment(sc):
    s, heff, w, v = solved(sc)
    spec = bm.member_spec(0)
    hss = s.blocks()[0].cpu().numpy()
    assert np.array_equal(heff[0], hss[0])                       # the zero pad rows of Y subtract exactly nothing
    href = spec["h"][np.ix_(sm.dof(spec["s"], 3), sm.dof(spec["s"], 3))]
    wref = np.linalg.eigvalsh(0.5 * (href + href.T))
    within("no environment: w against eigh of the 12 atoms", w[0], wref, spec["n"], np.abs(wref).max())
    assert tuple(s.environment_displacement(0).shape) == (36, 0)
    assert tuple(s.full_modes(0).shape) == (36, 36)
    # a batch of two such members: nothing to reduce at all
    two, heff2, w2, v2 = solved(sc, (0, 0))
    assert two.env_order == 0 and two.m_env == 0 and two.workspace_bytes() == 0
    assert np.array_equal(heff2[0], heff[0]) and np.array_equal(heff2[1], heff[0])
    within("env_order 0: w", w2, np.stack([wref, wref]), spec["n"], np.abs(wref).max())
    check_eigenvectors(heff2[1], w2[1], v2[1])
    assert tuple(two.environment_displacement(1).shape) == (36, 0)


# ---- 4. a member's bits are its own ----------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_batch(sc):
    _, heff5, w5, v5 = solved(sc)
    _, heff2, w2, v2 = solved(sc, (4, 2), env_order=bm.ENV_ORDER)
    _, heff1, w1, v1 = solved(sc, (2,), env_order=bm.ENV_ORDER)
    assert np.array_equal(heff5[2], heff2[1]) and np.array_equal(heff5[2], heff1[0]), "H_eff"
    assert np.array_equal(heff5[4], heff2[0]), "H_eff of member 4"
    assert np.array_equal(w5[2], w2[1]) and np.array_equal(w5[2], w1[0]), "w"
    assert np.array_equal(v5[2], v2[1]) and np.array_equal(v5[2], v1[0]), "v"


# ---- 5. against the single solver ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", ALL[1:])
def test_consistent_with_a_single_subsystem(sc, index):
    s, heff, w, _ = solved(sc)
    coord, system, ff = bm.member_inputs(index)
    assert np.array_equal(s.fitted_coord[index], coord) and s.transforms is None
    single = sc.Subsystem(s.fitted_coord[index], sm.package_ff(sc, ff), system)
    ref_h = single.effective_hessian().cpu().numpy()
    ref_w, _ = single.eigen()
    spec = bm.member_spec(index)
    top = np.abs(spec["heff"]).max()
    within(f"member {index} H_eff against Subsystem", heff[index], ref_h, spec["n"], top, bm.pinned(index, s.m, top))
    within(f"member {index} w against Subsystem", w[index], ref_w, spec["n"], np.abs(spec["w"]).max(), bm.pinned(index, s.m, top))


# ---- 6. an index range -------------------------------------------------------------------------------------------------------------
def test_index_subset_gives_the_same_rows(sc):
    _, _, w_all, v_all = solved(sc)
    part = make(sc, ALL)
    w, v = part.eigen(subset_by_index=(6, 15))
    assert w.shape == (5, 10) and v.shape == (5, 10, 36) and part._first_row == 6
    for i in ALL:
        spec = bm.member_spec(i)
        scale = np.abs(spec["w"]).max()
        within(f"member {i} subset w", w[i], w_all[i, 6:16], spec["n"], scale)
        vi = v[i] * np.sign((v[i] * v_all[i, 6:16]).sum(axis=1))[:, None]
        # an eigenvector moves by the backward error over its gap: the rows are compared as the eigensolver's tests compare them
        gap = np.diff(spec["w"][5:17]).min()
        assert np.abs(vi - v_all[i, 6:16]).max() <= 1e-8 * scale / gap


# ---- 7. masses and dim 1 -------------------------------------------------------------------------------------------------------------
def test_masses(sc):
    ids = (2, 3)
    masses = [sm.masses_of(bm.MEMBERS[i][0], seed=20 + i) for i in ids]
    s = make(sc, ids, masses=masses)
    assert tuple(s.inv_sqrt_mass.shape) == (2, bm.N_S)
    heff = s.effective_hessian().cpu().numpy()
    w, _ = s.eigen()
    for k, i in enumerate(ids):
        system = bm.member_inputs(i)[1]
        spec = bm.spec_of(bm.member_matrix(i), system, inv_sqrt_mass=1.0 / np.sqrt(masses[k][system]))
        top = np.abs(spec["heff"]).max()
        within(f"member {i} T H_eff T", heff[k], spec["heff"], spec["n"], top, bm.pinned(i, s.m, top))
        within(f"member {i} w with masses", w[k], spec["w"], spec["n"], np.abs(spec["w"]).max(), bm.pinned(i, s.m, top))
    # masses for one member only: the other is not scaled
    mixed = make(sc, ids, masses=[masses[0], None]).effective_hessian().cpu().numpy()
    plain = solved(sc, ids)[1]
    assert np.array_equal(mixed[0], heff[0]) and np.array_equal(mixed[1], plain[1])


def test_dim_1(sc):
    ids = (1, 4)
    s = make(sc, ids, dim=1, fit=True)          # (dim 1 ignores fit)
    assert s.m == bm.N_S and s.m_env == max(bm.N_ENV[i] for i in ids) and s.transforms is None
    heff = s.effective_hessian().cpu().numpy()
    w, v = s.eigen()
    hss, hes, hee = [t.cpu().numpy() for t in s.blocks()]
    for k, i in enumerate(ids):
        spec = bm.spec_of(bm.member_matrix(i, 1), bm.member_inputs(i)[1], dim=1)
        own = bm.N_ENV[i]
        for got, r in zip((hss[k], hes[k, :own], hee[k, :own, :own]), sm.blocks(spec["h"], spec["s"], spec["e"], 1)):
            assert np.allclose(got, r, rtol=0, atol=1e-12 * np.abs(r).max())
        assert np.array_equal(hee[k, own:, own:], np.eye(s.m_env - own)) and not hes[k, own:].any()
        top = np.abs(spec["heff"]).max()
        assert np.array_equal(heff[k], heff[k].T)
        within(f"member {i} dim 1 H_eff", heff[k], spec["heff"], spec["n"], top)
        within(f"member {i} dim 1 w", w[k], spec["w"], spec["n"], np.abs(spec["w"]).max())
        within(f"member {i} dim 1 trivial w", w[k, :1], 0.0, spec["n"], np.abs(spec["w"]).max())
        check_eigenvectors(heff[k], w[k], v[k])
    with pytest.raises(ValueError):
        s.prs()


# ---- 8. the environments follow ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [3, 4])
def test_follow_motion_and_full_modes(sc, torch, index):
    s, _, w, v = solved(sc)
    spec = bm.member_spec(index)
    coord, system, ff = bm.member_inputs(index)
    n = spec["n"]
    rows = s.v[index, 6:9].contiguous()
    xe = s.environment_displacement(index, rows).cpu().numpy()
    ref = sm.follow(spec["l"], spec["y"], v[index, 6:9])
    assert xe.shape == (3, 3 * bm.N_ENV[index])
    within(f"member {index} follow motion", xe, ref, n, max(np.abs(ref).max(), 1.0))
    # independent of the specification: H x of the member's full network vanishes at its environment atoms
    x = s.full_modes(index)[6:]
    assert tuple(x.shape) == (30, n)
    op = sc.PairOperator(coord, sm.package_ff(sc, ff))
    hx = op.apply(x.contiguous()).view(len(x), len(coord), 3)
    scale = np.abs(spec["h"]).max() * float(x.abs().max())
    e = torch.from_numpy(np.asarray(spec["e"])).cuda()
    sidx = torch.from_numpy(np.asarray(spec["s"])).cuda()
    within(f"member {index} H x at the environment", hx[:, e].cpu().numpy(), 0.0, n, scale)
    within(f"member {index} H x at the system", hx[:, sidx].reshape(len(x), -1).cpu().numpy(), w[index, 6:, None] * v[index, 6:], n,
           scale)
    with pytest.raises(ValueError, match="outside"):
        s.environment_displacement(5)


# ---- 9. the consumers and the comparisons run unchanged ----------------------------------------------------------------------------------
def test_consumers_against_their_models(sc, torch):
    from tests.test_batch_consumers_gpu import check_dcc, check_msf, np_dcc, np_msf, pinv_rows
    from tests.test_mode_overlap_gpu import check, np_overlap

    s, _, w, v = solved(sc)
    rows = np.arange(6, 36)
    msf = s.mean_square_fluctuation().cpu().numpy()
    dcc = s.dcc(norm=False).cpu().numpy()
    assert msf.shape == (5, bm.N_S) and dcc.shape == (5, bm.N_S, bm.N_S)
    d = np.random.RandomState(3).randn(5, 2, bm.N_S, 3)
    o = s.overlap(torch.from_numpy(d).cuda()).cpu().numpy()
    assert o.shape == (5, 2, 36)
    for b in ALL:
        check_msf(msf[b], np_msf(w[b], v[b], rows, 3), rows, 3, f"member {b}")
        drows = pinv_rows(w[b])
        check_dcc(dcc[b], np_dcc(w[b], v[b], drows, 3), drows, 3, f"member {b}")
        check(o[b], np_overlap(v[b], d[b]), f"member {b} overlap")
    s.finish()


def test_subspace_comparisons_against_their_models(sc, torch):
    from springcraft_amd.batch import _listed_pick, _rmsip_pick
    from tests.subspace import EPS, np_gram
    from tests.test_subspace_gpu import check_matrix, raw

    s, _, w, v = solved(sc)
    k = 10
    rows = [np.arange(6, 6 + k)] * 5
    got = raw(s, 0, _rmsip_pick(k, None))
    check_matrix(0, got, w, v, rows, "core rmsip")
    pub = s.rmsip()
    assert tuple(pub.shape) == (5, 5) and torch.equal(pub, pub.t()) and np.array_equal(pub.cpu().numpy(), got[0])
    cov = raw(s, 1, _listed_pick(rows[0], True))
    check_matrix(1, cov, w, v, rows, "core covariance overlap")
    assert np.array_equal(s.covariance_overlap(rows[0]).cpu().numpy(), cov[0]) and np.array_equal(cov[0], cov[0].T)
    pairs = [(0, 4), (2, 3), (1, 1)]
    g = s.mode_overlap_matrix(pairs, rows[0]).cpu().numpy()
    err = max(np.abs(g[i] - np_gram(v[a], v[b], rows[0], rows[0])).max() for i, (a, b) in enumerate(pairs))
    print(f"core gram: max |G - model| / (2 m eps) = {err / (2 * 36 * EPS):.3e}")
    assert err <= 2 * 36 * EPS
    # against a plain uniform solver of the same order: the batch is one
    other = sc.batch.DeviceBatchSolver(bm.N_S, 1, sc.InvariantForceField(sm.CUTOFF))
    other.w, other.v = s.w[2:3].clone(), s.v[2:3].clone()
    assert abs(float(s.rmsip(other=other)[2, 0]) - 1.0) <= 1e-12
    s.finish()


# ---- 10. the fit ------------------------------------------------------------------------------------------------------------------------
def test_fit_on_the_common_core(sc):
    from tests import ensemble_model as em

    family, system = bm.fit_family()
    ff = bm.member_inputs(3)[2]
    s = sc.SubsystemBatch(family, sm.package_ff(sc, ff), [system] * 4)        # fit=True is the default
    rot, trans = s.transforms
    assert rot.shape == (4, 3, 3) and trans.shape == (4, 3) and s.fit_rmsd.shape == (4,)
    scale = max(np.abs(c).max() for c in family)
    for b in range(4):
        assert abs(np.linalg.det(rot[b]) - 1.0) <= 1e-12 and np.abs(rot[b] @ rot[b].T - np.eye(3)).max() <= 1e-12
        redo = family[b] @ rot[b].T + trans[b]
        assert np.abs(redo - s.fitted_coord[b]).max() <= 8 * sm.EPS * scale      # the same three products, one rounding each
    cores = s.core_coord.cpu().numpy()
    assert cores.shape == (4, bm.N_S, 3)
    assert all(np.array_equal(cores[b], s.fitted_coord[b][system]) for b in range(4))
    # the three poses are one structure: fitted on one target they coincide, each within a fitted frame's gate of the truth
    g = 2 * em.gate(em.SPEC_ERR_SUPERPOSE[63][0], bm.N_S, scale)
    err = max(np.abs(cores[b] - cores[0]).max() for b in (1, 2))
    print(f"fitted cores of the posed copies: measured / gate = {err / g:.3f}")
    assert err <= g
    assert s.fit_rmsd[:3].max() <= s.fit_rmsd[3] and 0.2 * bm.PERTURBATION <= s.fit_rmsd[3] <= 3 * bm.PERTURBATION
    # every member's H_eff is the specification's on ITS fitted coordinates
    heff = s.effective_hessian().cpu().numpy()
    s.finish()
    for b in range(4):
        spec = bm.spec_of(bm.oracle_hessian(s.fitted_coord[b], ff), system)
        top = np.abs(spec["heff"]).max()
        within(f"fitted member {b} H_eff", heff[b], spec["heff"], spec["n"], top, bm.pinned(3, s.m, top))


# ---- 11. one member fails, the others do not ------------------------------------------------------------------------------------------------
def singular_member(sc):
    """
    Member 2 with one environment atom that keeps a single spring, along x exactly (tests/test_subsystem_gpu.py): its
    diagonal block of H_ee is gamma diag(1, 0, 0) and nothing else touches its y and z rows, so the pivot of its y column is
    exactly 0 whatever the order of the sums.  It passes the host checks: the atom has a contact, the member is coupled.
    """
    coord, system, _ = bm.member_inputs(2)
    coord = np.array(coord)
    n = len(coord)
    env = bm.partition(n, system)[1]
    atom, neighbour = env[3], system[0]
    coord[atom] = coord[neighbour] + np.array([3.0, 0.0, 0.0])
    d2 = ((coord[:, None, :] - coord[None, :, :]) ** 2).sum(axis=-1)
    off = np.array([[atom, j] for j in range(n) if j not in (atom, neighbour) and d2[atom, j] <= sm.CUTOFF ** 2])
    return coord, sc.PatchedForceField(sc.InvariantForceField(sm.CUTOFF), contact_pair_off=off), system


def test_a_singular_member_fails_alone(sc):
    bad_coord, bad_ff, system = singular_member(sc)
    ids = (1, 2, 4)
    coords = [bm.member_inputs(i)[0] for i in ids]
    ffs = [sm.package_ff(sc, bm.member_inputs(i)[2]) for i in ids]
    systems = [bm.member_inputs(i)[1] for i in ids]
    s = sc.SubsystemBatch([coords[0], bad_coord, coords[2]], [ffs[0], bad_ff, ffs[2]], systems, fit=False)
    s.solve()
    with pytest.raises(np.linalg.LinAlgError, match=r"member\(s\) 1 \(info = 11\).*not positive definite"):
        s.finish()
    assert s._info.cpu().tolist() == [0, 3 * 3 + 2, 0]               # 1 + the y column of the environment's fourth atom
    assert bool(s.w[1].isnan().all())
    s.finish()                                                       # reported once
    # the others have the bits of the same batch with a healthy member in its place
    _, heff, w, v = solved(sc, ids)
    assert np.isfinite(s.w[[0, 2]].cpu().numpy()).all()
    for k in (0, 2):
        assert np.array_equal(s.w[k].cpu().numpy(), w[k]) and np.array_equal(s.v[k].cpu().numpy(), v[k]), k
    again = s.effective_hessian().cpu().numpy()
    assert np.array_equal(again[0], heff[0]) and np.array_equal(again[2], heff[2]) and np.isnan(again[1]).all()
    with pytest.raises(np.linalg.LinAlgError):
        s.finish()
    # and a solve on healthy input succeeds afterwards
    healthy = make(sc, ids)
    w2, _ = healthy.eigen()
    assert np.array_equal(w2, w)


# ---- 12. refusals before any launch -------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(sc):
    coords = [np.array(bm.member_inputs(i)[0]) for i in (1, 2)]
    systems = [bm.member_inputs(i)[1] for i in (1, 2)]
    ff = sc.InvariantForceField(sm.CUTOFF)
    with pytest.raises(ValueError, match="one length"):
        sc.SubsystemBatch(coords, ff, systems[:1])
    with pytest.raises(ValueError, match="member 1: its system has"):
        sc.SubsystemBatch(coords, ff, [systems[0], systems[1][:5]])
    with pytest.raises(ValueError, match="fit=True needs at least 3"):
        sc.SubsystemBatch(coords, ff, [systems[0][:2], systems[1][:2]])
    with pytest.raises(ValueError, match="env_order"):
        sc.SubsystemBatch(coords, ff, systems, env_order=3)
    env = bm.partition(33, systems[1])[1]
    far = np.array(coords[1])
    far[env[0]] += 1000.0
    lonely = sc.SubsystemBatch([coords[0], far], ff, systems, fit=False)
    for call in (lonely.solve, lonely.effective_hessian):
        with pytest.raises(ValueError, match="member 1: 1 environment atom.*without any contact"):
            call()
    apart = np.array(coords[1])
    apart[systems[1]] += 1000.0
    with pytest.raises(ValueError, match="member 1: the system shares no spring"):
        sc.SubsystemBatch([coords[0], apart], ff, systems, fit=False).solve()
    assert lonely.w is None and lonely.matrix is None
    lonely.finish()   # nothing was enqueued, nothing is reported

    class Lopsided(sc.InvariantForceField):
        def force_constant(self, atom_i, atom_j, sq_distance):
            return np.where(atom_i < atom_j, 1.0, 2.0)

    with pytest.raises(ValueError, match="member 1: asymmetric"):
        sc.SubsystemBatch(coords, [ff, Lopsided(sm.CUTOFF)], systems, fit=False)


def test_raw_entries_refuse_bad_shapes(sc, torch):
    from springcraft_amd import _hip

    s = make(sc, (1, 2))
    L, h, bad = s._L, s.ctx.handle, _hip.SC_ERR_INVALID_ARG
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    hss, hes, hee = s._empty((2, 36, 36)), s._empty((2, 63, 36)), s._empty((2, 63, 63))
    info = torch.zeros(2, dtype=torch.int64, device="cuda")

    def blocks(members=s._members, batch=2, dim=3, n_s=12, env_order=21, coord=p(s._coord), row_start=p(s._row_start), out=p(hss)):
        return L.sc_dev_vsa_batch_blocks_f64(h, _hip.ptr(np.ascontiguousarray(members)) if members is not None else None, batch,
                                             dim, n_s, env_order, coord, p(s._pairs), p(s._gamma), row_start, p(s._group),
                                             p(s._pos), None, out, p(hes), p(hee))

    assert blocks() == _hip.SC_OK
    for kw in (dict(dim=2), dict(n_s=0), dict(batch=0), dict(batch=65536), dict(env_order=-1), dict(env_order=20),
               dict(n_s=11), dict(members=None), dict(coord=None), dict(row_start=None), dict(out=None)):
        assert blocks(**kw) == bad, kw
    shifted = np.array(s._members)
    shifted[1, 0] += 1                                               # the offsets must follow the member before
    assert blocks(members=shifted) == bad
    short = np.array(s._members)
    short[1, 4] -= 1                                                 # n_s + n_e != n_atoms
    assert blocks(members=short) == bad

    def reduce(ms=36, me=63, batch=2, a=p(hss), b=p(hes), c=p(hee), i=p(info)):
        return L.sc_dev_vsa_batch_reduce_f64(h, a, b, c, ms, me, batch, i)

    for kw in (dict(ms=0), dict(me=-1), dict(batch=0), dict(batch=65536), dict(a=None), dict(b=None), dict(c=None), dict(i=None)):
        assert reduce(**kw) == bad, kw
    assert reduce() == _hip.SC_OK and reduce(me=0, b=None, c=None) == _hip.SC_OK
    s.finish()
    assert info.cpu().tolist() == [0, 0]
