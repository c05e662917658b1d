"""
GPU tests of batch perturbation-response scanning (``k_mode_prs`` of csrc/mode_prs.hip) through the three layers:
``DeviceBatchSolver.prs`` (``sc_dev_prs_f64``), ``RaggedBatchSolver.prs`` (``sc_batch_plan_prs_f64``), ``RTB.prs`` and
``nma.prs(anm, mode_subset=...)`` (``sc_modes_prs_subset``).

The model is ``np_prs`` of tests/batch_prs.py evaluated on the solver's OWN (w, v): what is under test is the consumer --
which rows it takes, which it never reads, where it puts the result -- and its arithmetic, gated entry by entry by the
derived bound ``np_prs_bound`` (the module docstring there; tests/test_batch_prs_host.py shows that the float64 model
itself stays inside it).  Every comparison prints its largest |difference| / bound; the largest over this file is recorded
in profiles/batch_prs.txt.

Networks: ``np.random.seed(s); rand(N, 3) * 5 * N**(1/3)`` under ``InvariantForceField(13)``.  Sizes: N = 20 (one tile
with idle lanes), 63 and 65 (one below and one above the tile of 64: 65 is an odd N whose rows are only 8-byte aligned, and
three tiles, one of them diagonal with one atom), 129 (six tiles).  The kernel's tile side is 64, a power of two, so no
further sizes around it are needed.  Batches of at most 5.
"""
import numpy as np
import pytest

from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver
from tests.batch_prs import CUTOFF, SIZES, SUBSETS, check_prs, network, np_prs, np_prs_bound, pinv_rows
from tests.test_batch_consumers_gpu import solved, window_case
from tests.util import load_csv, structures

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


_SOLVED = {}


def batch_of(sc, torch, n_atoms, batch=2):
    """A finished full-spectrum solver of seeds 0 .. batch - 1 at this size with host copies of (w, v): once per shape."""
    key = (n_atoms, batch)
    if key not in _SOLVED:
        coords = np.stack([network(n_atoms, seed) for seed in range(batch)])
        s, w, v = solved(sc, torch, coords, sc.InvariantForceField(CUTOFF))
        for a in (coords, w, v):
            a.setflags(write=False)
        for b in range(batch):
            assert np.abs(w[b, :6]).max() <= 1e-12 * w[b, -1] and w[b, 6] >= 0.005 * w[b, -1], "a nearly disconnected network"
        _SOLVED[key] = (s, coords, w, v)
    return _SOLVED[key]


def dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()     # (a copy: the cached inputs are read-only)


def symmetric_and_non_negative(torch, p):
    assert torch.equal(p, p.transpose(-1, -2)) and bool((p >= 0).all())


# ---- 1. parity inside the bound, the default rule and lists, bit-level symmetry ---------------------------------------------
@pytest.mark.parametrize("n_atoms", SIZES)
def test_uniform_batch_matches_the_model_inside_the_bound(sc, torch, n_atoms):
    s, _, w, v = batch_of(sc, torch, n_atoms)
    raw, nrm = s.prs(norm=False), s.prs()
    assert raw.is_cuda and raw.dtype == torch.float64 and tuple(raw.shape) == tuple(nrm.shape) == (2, n_atoms, n_atoms)
    symmetric_and_non_negative(torch, raw)
    lists = SUBSETS if n_atoms == 20 else {17: SUBSETS[17], 4: SUBSETS[4]}
    for b in range(2):
        rows = pinv_rows(w[b])
        assert np.array_equal(rows, np.arange(6, 3 * n_atoms))
        check_prs(raw[b].cpu().numpy(), w[b], v[b], rows, f"N = {n_atoms} [{b}] pinv rule")
        check_prs(nrm[b].cpu().numpy(), w[b], v[b], rows, f"N = {n_atoms} [{b}] pinv rule, norm", norm=True)
        assert bool((nrm[b].diagonal() == 1.0).all())
    for k, subset in lists.items():
        assert len(subset) == k
        got, gotn = s.prs(mode_subset=subset, norm=False), s.prs(subset)
        symmetric_and_non_negative(torch, got)
        for b in range(2):
            check_prs(got[b].cpu().numpy(), w[b], v[b], subset, f"N = {n_atoms} [{b}] {k} modes")
            check_prs(gotn[b].cpu().numpy(), w[b], v[b], subset, f"N = {n_atoms} [{b}] {k} modes, norm", norm=True)
    # a mode listed twice counts twice, an empty list gives zeros and 0 / 0 under norm
    twice = s.prs(mode_subset=[9, 7, 9], norm=False)
    check_prs(twice[1].cpu().numpy(), w[1], v[1], [9, 7, 9], f"N = {n_atoms} [1] modes [9, 7, 9]")
    assert not bool(s.prs(mode_subset=[], norm=False).any()) and bool(torch.isnan(s.prs(mode_subset=[])).all())
    # a repeated call gives the same bits
    assert torch.equal(s.prs(norm=False), raw) and torch.equal(s.prs(), nrm)


def test_effector_and_sensor_profiles_stay_on_the_device(sc, torch):
    from springcraft_amd import nma

    s, _, w, v = batch_of(sc, torch, 65)
    p, eff, sens = s.prs_effector_sensor()
    assert torch.equal(p, s.prs()) and eff.is_cuda and sens.is_cuda and tuple(eff.shape) == tuple(sens.shape) == (2, 65)
    for b in range(2):
        e, r = nma.effector_sensor(p[b].cpu().numpy())
        assert np.allclose(eff[b].cpu().numpy(), e, rtol=1e-13, atol=0) and np.allclose(sens[b].cpu().numpy(), r, rtol=1e-13, atol=0)
    p4, _, _ = s.prs_effector_sensor(mode_subset=SUBSETS[4], norm=False)
    assert torch.equal(p4, s.prs(SUBSETS[4], norm=False))


# ---- 2. behind an index range ----------------------------------------------------------------------------------------------------
def test_behind_an_index_range(sc, torch):
    n_atoms, batch = 65, 3
    coords = np.stack([network(n_atoms, seed) for seed in range(batch)])
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(CUTOFF), subset_by_index=(3, 25))
    assert w.shape == (batch, 23)
    raw, sub = s.prs(norm=False).cpu().numpy(), s.prs(mode_subset=[7, 20, 7]).cpu().numpy()
    for b in range(batch):
        check_prs(raw[b], w[b], v[b], np.arange(3, 23), f"subset_by_index (3, 25) [{b}] default: modes 6..25")
        check_prs(sub[b], w[b], v[b], [4, 17, 4], f"subset_by_index (3, 25) [{b}] modes [7, 20, 7], norm", norm=True)
    with pytest.raises(ValueError, match="was not solved"):
        s.prs(mode_subset=[26])


# ---- 3. behind a value window: counts that differ, an empty window, and rows that are never read ----------------------------------
def test_behind_a_value_window_the_padding_is_never_read(sc, torch):
    n_atoms, batch, K = 65, 5, 24
    coords, mats, lam, (vl, vu), expected = window_case(n_atoms, K, 3, batch=batch)
    assert expected.max() == K and expected.min() == 0 and len(set(expected)) >= 3
    s = DeviceBatchSolver(n_atoms, batch, sc.ParameterFreeForceField(), subset_by_value=(vl, vu), max_modes=K)
    s.matrix.copy_(torch.from_numpy(mats))
    s.eigh()
    raw, nrm = s.prs(norm=False), s.prs()                    # enqueued straight behind the solve
    s.finish()
    counts = s.counts.cpu().numpy()
    assert np.array_equal(counts, expected)
    for b in range(batch):
        s.v[b, counts[b]:] = float("nan")                    # what lies behind the count must not matter
    again, again_n = s.prs(norm=False), s.prs()
    assert torch.equal(again, raw)
    w, v = s.w.cpu().numpy(), s.v.cpu().numpy()
    symmetric_and_non_negative(torch, raw)
    for b in range(batch):
        k = counts[b]
        if k == 0:
            assert not bool(raw[b].any()) and bool(torch.isnan(nrm[b]).all()) and bool(torch.isnan(again_n[b]).all())
            continue
        assert bool(torch.isfinite(again[b]).all()) and bool(torch.isfinite(again_n[b]).all())
        assert torch.equal(again_n[b], nrm[b])
        # (K rows are listed; those behind the count are staged as zeros)
        check_prs(raw[b].cpu().numpy(), w[b], v[b], np.arange(k), f"window [{b}] count {k}", k=K)
        check_prs(nrm[b].cpu().numpy(), w[b], v[b], np.arange(k), f"window [{b}] count {k}, norm", norm=True, k=K)
    with pytest.raises(ValueError, match="subset_by_value"):
        s.prs(mode_subset=[7])


# ---- 4. bits ----------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_batch_size_or_position(sc, torch):
    n_atoms = 65
    ff = sc.InvariantForceField(CUTOFF)
    s1, _, _ = solved(sc, torch, network(n_atoms, 0)[None], ff)
    s3, _, _ = solved(sc, torch, np.stack([network(n_atoms, 0), network(n_atoms, 1), network(n_atoms, 2)]), ff)
    # the consumer's own property: the same eigenpairs alone, first of three and last of three
    for b in (0, 2):
        s3.w[b].copy_(s1.w[0])
        s3.v[b].copy_(s1.v[0])
    scale1 = dev(torch, np.random.RandomState(2).uniform(0.5, 2.0, (1, n_atoms)))
    scale3 = scale1.expand(3, -1).contiguous()
    for kw in (dict(norm=False), dict(), dict(mode_subset=SUBSETS[5], norm=False), dict(mode_subset=SUBSETS[17])):
        p1, p3 = s1.prs(**kw), s3.prs(**kw)
        assert bool(torch.isfinite(p3).all()) and float(p1.abs().max()) > 0
        assert torch.equal(p1[0], p3[0]) and torch.equal(p1[0], p3[2]) and not torch.equal(p1[0], p3[1])
        q1, q3 = s1.prs(atom_scale=scale1, **kw), s3.prs(atom_scale=scale3, **kw)
        assert torch.equal(q1[0], q3[0]) and torch.equal(q1[0], q3[2])
    # a weight-zero row is selected out, not multiplied by zero
    ref = s3.prs(norm=False)
    s3.v[1, 0:6] = float("nan")                              # the trivial rows: under the pinv threshold
    assert torch.equal(s3.prs(norm=False), ref)


# ---- 5. the reference's fixtures ------------------------------------------------------------------------------------------------------
def _check_fixtures(p, eff, sens):
    name = "prody_anm_13_ang_cutoff_prs"
    assert np.allclose(p.cpu().numpy(), load_csv(f"{name}_mat_1l2y.csv.gz"))
    assert np.allclose(eff.cpu().numpy(), load_csv(f"{name}_eff_1l2y.csv.gz"))
    assert np.allclose(sens.cpu().numpy(), load_csv(f"{name}_sens_1l2y.csv.gz"))


def test_1l2y_reproduces_the_prody_fixtures_uniform_and_ragged(sc, torch):
    ca = np.asarray(structures()["1l2y_coord"], dtype=np.float64)
    assert len(ca) == 20
    ff = sc.InvariantForceField(13)
    s, _, _ = solved(sc, torch, np.stack([ca, ca]), ff)
    p, eff, sens = s.prs_effector_sensor()
    for b in range(2):
        _check_fixtures(p[b], eff[b], sens[b])
    assert torch.equal(p[0], p[1])

    other = network(65, 4)
    r = RaggedBatchSolver((20, 65), ff)
    r.solve(dev(torch, np.concatenate([ca, other])))
    rp, reff, rsens = r.prs_effector_sensor()
    raw = r.prs(norm=False)
    r.finish()
    assert [tuple(t.shape) for t in rp] == [(20, 20), (65, 65)] and [tuple(t.shape) for t in reff] == [(20,), (65,)]
    assert rp[0].untyped_storage().data_ptr() == rp[1].untyped_storage().data_ptr() and rp[1].storage_offset() == 400
    _check_fixtures(rp[0], reff[0], rsens[0])
    # the neighbour against the model on its own rows and columns of the slot
    for b, n in enumerate((20, 65)):
        w, v = (t.cpu().numpy() for t in r.results()[b])
        assert w.shape == (3 * n,) and v.shape == (3 * n, 3 * n)
        # (the slot lists all 195 rows; a structure's pad rows carry no weight)
        check_prs(raw[b].cpu().numpy(), w, v, pinv_rows(w), f"ragged (20, 65) [{b}]", k=195)
        check_prs(rp[b].cpu().numpy(), w, v, pinv_rows(w), f"ragged (20, 65) [{b}], norm", norm=True, k=195)
        symmetric_and_non_negative(torch, raw[b])
    scale = dev(torch, np.random.RandomState(6).uniform(0.5, 2.0, 85))
    scaled = r.prs(norm=False, atom_scale=scale)
    w, v = (t.cpu().numpy() for t in r.results()[1])
    check_prs(scaled[1].cpu().numpy(), w, v, pinv_rows(w), "ragged (20, 65) [1] with a packed atom_scale",
              scale=scale[20:].cpu().numpy(), k=195)


# ---- 6. cross-checks with the one-model API, masses and RTB ------------------------------------------------------------------------------
def test_the_batch_agrees_with_the_one_model_path(sc, torch):
    n_atoms = 65
    s, coords, w, v = batch_of(sc, torch, n_atoms)
    anm = sc.ANM(coords[0], sc.InvariantForceField(CUTOFF))
    rows = pinv_rows(w[0])
    bound = np_prs_bound(w[0], v[0], rows, None, len(rows))
    for norm in (False, True):
        one = sc.nma.prs(anm, norm=norm)                     # today's path: covariance in scratch, then reduced
        got = s.prs(norm=norm)[0].cpu().numpy()
        b = bound / np.diag(np_prs(w[0], v[0], rows))[:, None] if norm else bound
        ratio = float((np.abs(got - one) / b).max())
        print(f"N = 65 batch against nma.prs, norm = {norm}: max |difference| / bound = {ratio:.3e}")
        assert ratio <= 2.0
    # nma.prs over a list of modes: the batch kernel on the model's own device-resident eigenpairs
    wa, va = anm.eigen()
    subset = [6, 7, 9, 20]
    for norm in (False, True):
        got = sc.nma.prs(anm, norm=norm, mode_subset=subset)
        assert isinstance(got, np.ndarray) and got.shape == (n_atoms, n_atoms)
        check_prs(got, wa, va, subset, f"nma.prs(mode_subset={subset}, norm={norm})", norm=norm)
    p, eff, sens = anm.prs_effector_sensor(mode_subset=subset)
    assert np.array_equal(p, sc.nma.prs(anm, mode_subset=subset))
    e, r = sc.nma.effector_sensor(p)
    assert np.array_equal(eff, e) and np.array_equal(sens, r)
    assert np.array_equal(sc.nma.prs(anm, norm=False, mode_subset=[]), np.zeros((n_atoms, n_atoms)))
    with pytest.raises(IndexError):
        sc.nma.prs(anm, mode_subset=[7, 3 * n_atoms])
    assert anm._covariance is None                           # no (3N, 3N) matrix was formed on the way


def test_masses_and_atom_scale(sc, torch):
    n_atoms, batch = 63, 2
    coords = np.stack([network(n_atoms, seed) for seed in range(batch)])
    masses = np.random.RandomState(3).uniform(10.0, 20.0, (batch, n_atoms))
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(CUTOFF), masses=masses)
    cart, raw = s.prs(norm=False, atom_scale=s.inv_sqrt_mass).cpu().numpy(), s.prs(norm=False).cpu().numpy()
    cart_n = s.prs(atom_scale=s.inv_sqrt_mass).cpu().numpy()
    for b in range(batch):
        rows = pinv_rows(w[b])
        assert np.array_equal(rows, np.arange(6, 3 * n_atoms))
        t = s.inv_sqrt_mass[b].cpu().numpy()
        check_prs(cart[b], w[b], v[b], rows, f"masses [{b}] atom_scale = 1 / sqrt(m)", scale=t)
        check_prs(cart_n[b], w[b], v[b], rows, f"masses [{b}] atom_scale = 1 / sqrt(m), norm", scale=t, norm=True)
        check_prs(raw[b], w[b], v[b], rows, f"masses [{b}] the modes as they are")
        assert not np.allclose(cart[b], raw[b])


def test_rtb_inherits_the_method(sc, torch):
    n_atoms = 60
    coord = network(n_atoms, 0)
    rtb = sc.RTB(coord, sc.InvariantForceField(CUTOFF), np.arange(n_atoms) // 5)
    rtb.solve()
    w, v = (t[0].cpu().numpy() for t in rtb.finish())
    assert v.shape == (rtb.nr, 3 * n_atoms) and rtb.nr == 72
    rows = pinv_rows(w)
    assert np.array_equal(rows, np.arange(6, rtb.nr))
    raw, nrm = rtb.prs(norm=False), rtb.prs()
    assert tuple(raw.shape) == (1, n_atoms, n_atoms)
    symmetric_and_non_negative(torch, raw)
    check_prs(raw[0].cpu().numpy(), w, v, rows, "RTB N = 60, blocks of 5: the expanded modes")
    check_prs(nrm[0].cpu().numpy(), w, v, rows, "RTB N = 60, blocks of 5: the expanded modes, norm", norm=True)
    check_prs(rtb.prs(mode_subset=[8, 30, 11], norm=False)[0].cpu().numpy(), w, v, [8, 30, 11], "RTB modes [8, 30, 11]")


# ---- 7. a structure that cannot be solved ----------------------------------------------------------------------------------------------
def test_a_non_finite_matrix_gives_nan_and_leaves_the_neighbours_alone(sc, torch):
    n_atoms, batch = 65, 3
    ff = sc.InvariantForceField(CUTOFF)
    mats = np.stack([sc.compute_hessian(network(n_atoms, seed), ff)[0] for seed in range(batch)])

    def run(matrices):
        s = DeviceBatchSolver(n_atoms, batch, ff)
        s.matrix.copy_(torch.from_numpy(matrices))
        s.eigh()
        return s, s.prs(norm=False), s.prs(), s.prs(mode_subset=SUBSETS[5])

    good, *ref = run(mats)
    good.finish()
    broken = mats.copy()
    broken[1, 5, 9] = broken[1, 9, 5] = np.nan
    bad, *got = run(broken)
    with pytest.raises(np.linalg.LinAlgError):
        bad.finish()
    for g, r in zip(got, ref):
        assert bool(torch.isnan(g[1]).all())
        for b in (0, 2):
            assert torch.equal(g[b], r[b]) and bool(torch.isfinite(g[b]).all())


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors(sc, torch):
    s, coords, _, _ = batch_of(sc, torch, 20)
    ff = sc.InvariantForceField(CUTOFF)
    gnm = DeviceBatchSolver(20, 2, sc.InvariantForceField(10.0), dim=1)
    gnm.solve(dev(torch, coords))
    gnm.finish()
    for call in (gnm.prs, gnm.prs_effector_sensor):
        with pytest.raises(ValueError, match="Instance of ANM class expected"):
            call()
    novec = DeviceBatchSolver(20, 2, ff, want_vectors=False)
    novec.solve(dev(torch, coords))
    novec.finish()
    with pytest.raises(ValueError, match="want_vectors"):
        novec.prs()
    good = torch.ones((2, 20), dtype=torch.float64, device=s.device)
    assert torch.equal(s.prs(atom_scale=good, norm=False), s.prs(norm=False))
    for bad in (good[:, :19].contiguous(), good[0].contiguous(), torch.ones((2, 20, 3), dtype=torch.float64, device=s.device)):
        with pytest.raises(ValueError, match="Expected atom_scale of shape"):
            s.prs(atom_scale=bad)
    for bad in (good.cpu(), good.float(), good.cpu().numpy()):
        with pytest.raises(ValueError, match="atom_scale must be a contiguous CUDA float64 tensor"):
            s.prs(atom_scale=bad)
    for subset in ([5, 7], [6, 6, 0]):
        with pytest.raises(ValueError, match="Trivial modes are included in the current selection"):
            s.prs(mode_subset=subset)
    with pytest.raises(ValueError, match="was not solved"):
        s.prs(mode_subset=[7, 60])
    with pytest.raises(ValueError, match="Instance of ANM class expected"):
        sc.nma.prs(sc.GNM(coords[0], sc.InvariantForceField(10.0)), mode_subset=[3])
