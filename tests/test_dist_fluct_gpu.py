"""
GPU tests of the distance fluctuations (``k_dist_fluct`` of csrc/dist_fluct.hip) through the three layers:
``nma.distance_fluctuation`` (one model, ``sc_modes_distfluct``), ``DeviceBatchSolver.distance_fluctuation``
(``sc_dev_modes_distfluct_f64``) and ``RaggedBatchSolver.distance_fluctuation`` (``sc_batch_plan_modes_distfluct_f64``).

The oracle is NumPy float64 on the solver's own ``w``, ``v``, coordinates and rows, the definition evaluated directly
(``np_distfluct`` of tests/test_dist_fluct_host.py):

    F[a, c] = sum_r (n_ac . (u_r[c] - u_r[a]))^2 / w_r,        n_ac = (x_c - x_a) / |x_c - x_a|

The bound follows tests/test_batch_consumers_gpu.py: a sum of rows x 3 products per pair, every term at most twice
``s (|u_a|^2 + |u_c|^2)`` in size, so

    |got - ref| <= 4 max(rows, 4) 3 EPS (msf_a + msf_c)

with ``msf`` from NumPy on the same rows (times ``atom_scale^2`` where one is given).  A float64 evaluation in another row
order sits at 0.002 of this bound against a long-double evaluation (N = 100, all 294 modes), the expanded covariance form
at 0.003.  Symmetry, the zero diagonal and the placement checks are bit for bit.  The figures are printed before they are
asserted (``pytest -s``).  Shapes: N = 5 (smaller than a tile), 20 (1l2y), 100 (two tiles per side, both partly filled),
301 (m odd: rows are only 8-byte aligned).
"""
import numpy as np
import pytest

from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver
from tests.test_batch_consumers_gpu import K_B, N_A, check_dcc, make_coords, np_dcc, np_msf, solved, window_case
from tests.test_dist_fluct_host import np_distfluct
from tests.util import ref_data, synthetic_coord

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def check(got, w, v, rows, coord, what, scale=None, exact=True):
    """``got`` (N, N) against the oracle on rows ``rows`` of (w, v) under the bound of the module docstring."""
    got = np.asarray(got)
    rows = np.asarray(rows, dtype=np.int64)
    n = len(coord)
    ref = np_distfluct(w, v, rows, coord, scale)
    msf = np_msf(w, v[:, :3 * n], rows, 3) * (1.0 if scale is None else scale ** 2)
    assert got.shape == ref.shape == (n, n), (what, got.shape)
    tol = 4 * max(len(rows), 4) * 3 * EPS
    size = msf[:, None] + msf[None, :]
    err = np.abs(got - ref)
    print(f"{what}: max err / (msf_a + msf_c) {(err / size).max():.3e}, bound {tol:.3e}, largest entry {ref.max():.3e}")
    assert np.all(err <= tol * size), what
    if exact:
        assert np.array_equal(got, got.T), what                 # both orientations from one sum
        assert np.all(np.diag(got) == 0.0), what
        assert np.all(got >= 0.0), what                          # only non-negative terms
    return ref


def no_timeouts(ctx):
    """Nothing the solves in front of the consumer ran into: chase time-outs, take-overs, unfinished chases."""
    for name in ("chase_timeouts", "chase_incomplete", "chase_resumed", "panel_coop_timeouts", "resident_takeovers"):
        assert ctx.counter(name) == 0, (name, ctx.counter(name))


def gpu(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


# ---- 1. uniform batches, the three kinds of selection --------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms,batch", [(5, 1), (100, 1), (100, 5), (301, 5)])
def test_uniform_batches_match_the_definition_on_the_solvers_own_eigenpairs(sc, torch, n_atoms, batch):
    m = 3 * n_atoms
    coords = make_coords(n_atoms, batch, seed=600 + n_atoms)
    ff = sc.HinsenForceField() if n_atoms == 5 else sc.InvariantForceField(13.0)
    s, w, v = solved(sc, torch, coords, ff)
    x = gpu(torch, coords)
    hi = min(36, m)
    lists = {"default": None, f"arange(6, {hi})": np.arange(6, hi),
             "unsorted with a repeat": np.array([9, 7, m - 1, 9, 12, 6])}
    for name, subset in lists.items():
        rows = np.arange(6, m) if subset is None else subset
        f = s.distance_fluctuation(x, mode_subset=subset)
        assert f.is_cuda and tuple(f.shape) == (batch, n_atoms, n_atoms) and f.dtype == torch.float64
        f = f.cpu().numpy()
        # (897 rows at N = 301 cost the NumPy oracle a second per structure: the first and the last of the batch there)
        for b in (range(batch) if len(rows) < 500 else (0, batch - 1)):
            check(f[b], w[b], v[b], rows, coords[b], f"N {n_atoms} batch {batch} [{b}] {name}")
    f = s.distance_fluctuation(x).cpu().numpy()
    scaled = s.distance_fluctuation(x, tem=300, tem_factors=K_B * N_A).cpu().numpy()
    assert np.allclose(scaled, f * (300 * K_B * N_A), rtol=1e-14, atol=0)
    assert not np.any(s.distance_fluctuation(x, mode_subset=[]).cpu().numpy())
    k = sc.nma.effective_stiffness(s.distance_fluctuation(x))
    assert k.is_cuda and np.array_equal(k.cpu().numpy(), sc.nma.effective_stiffness(f))
    no_timeouts(s.ctx)


# ---- 2. masses -------------------------------------------------------------------------------------------------------------
def test_masses_with_and_without_the_atom_scale(sc, torch):
    n_atoms, batch = 100, 3
    coords = make_coords(n_atoms, batch, seed=620)
    masses = np.random.RandomState(2).uniform(1.0, 20.0, (batch, n_atoms))
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(13.0), masses=masses)
    x = gpu(torch, coords)
    rows = np.arange(6, 3 * n_atoms)
    ism = s.inv_sqrt_mass.cpu().numpy()
    assert np.array_equal(ism, 1.0 / np.sqrt(masses))
    cart = s.distance_fluctuation(x, atom_scale=s.inv_sqrt_mass).cpu().numpy()
    raw = s.distance_fluctuation(x).cpu().numpy()
    for b in range(batch):
        check(cart[b], w[b], v[b], rows, coords[b], f"masses, atom_scale=inv_sqrt_mass [{b}]", scale=ism[b])
        check(raw[b], w[b], v[b], rows, coords[b], f"masses, no atom_scale [{b}]")
    assert not np.allclose(cart, raw)
    sub = np.array([9, 7, 30, 9])
    f = s.distance_fluctuation(x, mode_subset=sub, atom_scale=s.inv_sqrt_mass).cpu().numpy()
    check(f[1], w[1], v[1], sub, coords[1], "masses, atom_scale, a list [1]", scale=ism[1])
    with pytest.raises(ValueError, match="atom_scale"):
        s.distance_fluctuation(x, atom_scale=s.inv_sqrt_mass[:, :-1].contiguous())
    with pytest.raises(ValueError, match="atom_scale"):
        s.distance_fluctuation(x, atom_scale=ism)
    with pytest.raises(ValueError, match="coord"):
        s.distance_fluctuation(x[:, :-1].contiguous())
    with pytest.raises(ValueError, match="coord"):
        s.distance_fluctuation(x.float())


# ---- 3. the unprojected form, ANM and GNM ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 1])
def test_unprojected_form_is_the_dcc_expression_bit_for_bit(sc, torch, dim):
    n_atoms, batch = 100, 3
    ntriv = 6 if dim == 3 else 1
    coords = make_coords(n_atoms, batch, seed=630)
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(13.0 if dim == 3 else 10.0), dim=dim)
    x = gpu(torch, coords)
    for subset in (np.arange(ntriv, ntriv + 30), np.array([9, 7, 30, 9])):
        c = s.dcc(mode_subset=subset, norm=False).cpu().numpy()
        f = s.distance_fluctuation(x, mode_subset=subset, projected=False).cpu().numpy()
        for b in range(batch):
            d = np.diag(c[b])
            assert np.array_equal(f[b], (d[:, None] + d[None, :]) - 2 * c[b])
            assert np.all(np.diag(f[b]) == 0.0)
            check_dcc(c[b], np_dcc(w[b], v[b], subset, dim), subset, dim, f"dim {dim} [{b}] the dcc behind it")
    # the default selection is every non-trivial mode (not the dcc default's covariance rule)
    rows = np.arange(ntriv, dim * n_atoms)
    f = s.distance_fluctuation(x, projected=False).cpu().numpy()
    c = s.dcc(mode_subset=rows, norm=False).cpu().numpy()
    d = np.diag(c[0])
    assert np.array_equal(f[0], (d[:, None] + d[None, :]) - 2 * c[0])
    if dim == 3:
        # the projection on one direction never exceeds the whole relative displacement
        p = s.distance_fluctuation(x).cpu().numpy()
        assert np.all(p <= f * (1 + 1e-9) + 1e-12 * f.max())


def test_dim_1_solvers_raise_on_the_host_before_anything_is_enqueued(sc, torch):
    ff = sc.InvariantForceField(10.0)
    x = gpu(torch, make_coords(30, 2, seed=640))
    packed = gpu(torch, np.concatenate([synthetic_coord(20, 1), synthetic_coord(30, 2)]))
    # nothing was solved and nothing may be enqueued: a call that reached the device would read uninitialised modes
    for s, c in ((DeviceBatchSolver(30, 2, ff, dim=1), x), (RaggedBatchSolver((20, 30), ff, dim=1), packed)):
        with pytest.raises(ValueError, match="dim=3"):
            s.distance_fluctuation(c)
        with pytest.raises(ValueError, match="dim=3"):
            s.distance_fluctuation(c, mode_subset=[3, 4])
    gnm = sc.GNM(synthetic_coord(30, 560), ff)
    with pytest.raises(ValueError, match="ANM"):
        gnm._modes_device().distfluct(np.arange(1, 10), synthetic_coord(10, 1))   # the C entry's own argument error
    from springcraft_amd import _hip

    bad = DeviceBatchSolver(10, 1, sc.InvariantForceField(13.0))
    sel = _hip.ModeSelection()
    import ctypes as C

    rc = _hip.lib().sc_dev_modes_distfluct_f64(bad.ctx.handle, C.c_void_p(bad.w.data_ptr()), C.c_void_p(bad.v.data_ptr()),
                                               32, 30, 1, C.byref(sel), None, C.c_void_p(x.data_ptr()), None,
                                               C.c_void_p(bad.matrix.data_ptr()))
    assert rc == _hip.SC_ERR_INVALID_ARG                  # m % 3 != 0


# ---- 4. one model --------------------------------------------------------------------------------------------------------------
def test_single_model_1l2y_against_a_batch_of_one_and_the_oracle(sc, torch):
    ca = sc.read_pdb_ca(ref_data("1l2y.pdb"))
    n = ca.array_length()
    ff = sc.InvariantForceField(13.0)
    anm = sc.ANM(ca, ff)
    coord = np.asarray(ca.coord, dtype=np.float64)
    w1, v1 = anm.eigen()
    f = anm.distance_fluctuation()
    assert isinstance(f, np.ndarray) and f.shape == (n, n) and f.dtype == np.float64
    assert np.array_equal(f, sc.nma.distance_fluctuation(anm))
    check(f, w1, v1, np.arange(6, 3 * n), coord, "1l2y single model, default")
    sub = np.array([40, 7, 59, 40, 12, 6])
    check(anm.distance_fluctuation(mode_subset=sub), w1, v1, sub, coord, "1l2y single model, a list")
    # row 0 of a one-structure batch (another eigensolver path: each against the oracle on its own eigenpairs, and against
    # each other within the bound)
    s, w, v = solved(sc, torch, coord[None], ff)
    fb = s.distance_fluctuation(gpu(torch, coord[None])).cpu().numpy()[0]
    check(fb, w[0], v[0], np.arange(6, 3 * n), coord, "1l2y batch of one")
    msf = np_msf(w1, v1, np.arange(6, 3 * n), 3)
    tol = 4 * (3 * n - 6) * 3 * EPS
    gap = np.abs(f - fb) / (msf[:, None] + msf[None, :])
    print(f"1l2y single model against the batch of one: {gap.max():.3e}, bound {tol:.3e}")
    assert np.all(gap <= tol)
    un = anm.distance_fluctuation(projected=False)
    c = anm.dcc(mode_subset=np.arange(6, 3 * n), norm=False)
    assert np.array_equal(un, (np.diag(c)[:, None] + np.diag(c)[None, :]) - 2 * c)
    assert np.all(f <= un * (1 + 1e-9))
    g = sc.GNM(ca, sc.InvariantForceField(7.0)).distance_fluctuation(projected=False)
    assert g.shape == (n, n) and np.all(np.diag(g) == 0.0) and np.all(g[~np.eye(n, dtype=bool)] > 0)
    scaled = anm.distance_fluctuation(tem=300, tem_factors=K_B * N_A)
    assert np.allclose(scaled, f * (300 * K_B * N_A), rtol=1e-14, atol=0)
    kappa = sc.nma.effective_stiffness(f, tem=300, tem_factors=K_B * N_A)
    off = ~np.eye(n, dtype=bool)
    assert np.all(np.diag(kappa) == 0.0) and np.allclose(kappa[off] * f[off], 300 * K_B * N_A)
    assert not np.any(anm.distance_fluctuation(mode_subset=[]))
    with pytest.raises(IndexError):
        anm.distance_fluctuation(mode_subset=[7, 3 * n])


# ---- 5. partial spectra ----------------------------------------------------------------------------------------------------
def test_behind_a_value_window_the_counts_are_read_on_the_device(sc, torch):
    n_atoms, K, batch = 101, 24, 3
    coords, mats, lam, (vl, vu), expected = window_case(n_atoms, K, 3, batch=batch)
    assert expected.max() == K and expected.min() == 0
    s = DeviceBatchSolver(n_atoms, batch, sc.ParameterFreeForceField(), subset_by_value=(vl, vu), max_modes=K)
    x = gpu(torch, coords)
    s.matrix.copy_(torch.from_numpy(mats))
    s.eigh()
    f = s.distance_fluctuation(x)                              # enqueued straight behind the solve
    s.finish()
    counts = s.counts.cpu().numpy()
    print("window counts", counts, "expected", expected)
    assert np.array_equal(counts, expected)
    w, v, f = s.w.cpu().numpy(), s.v.cpu().numpy(), f.cpu().numpy()
    for b in range(batch):
        if counts[b] == 0:
            assert not np.any(f[b]) and not np.any(np.signbit(f[b]))
            continue
        check(f[b], w[b], v[b], np.arange(min(counts[b], K)), coords[b], f"window [{b}] count {counts[b]}")
    with pytest.raises(ValueError, match="subset_by_value"):
        s.distance_fluctuation(x, mode_subset=[7, 8])
    no_timeouts(s.ctx)


def test_behind_an_index_range(sc, torch):
    lo, hi = 6, 25
    n_atoms, batch = 100, 3
    coords = make_coords(n_atoms, batch, seed=650)
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(13.0), subset_by_index=(lo, hi))
    x = gpu(torch, coords)
    explicit = np.array([9, 7, 25, 9, 12])
    for subset, rows in ((None, np.arange(0, hi - lo + 1)), (explicit, explicit - lo)):
        f = s.distance_fluctuation(x, mode_subset=subset).cpu().numpy()
        for b in range(batch):
            check(f[b], w[b], v[b], rows, coords[b], f"subset_by_index [{b}] {None if subset is None else list(subset)}")
    with pytest.raises(ValueError, match=f"{lo}\\.\\.{hi}"):
        s.distance_fluctuation(x, mode_subset=[7, 26])
    with pytest.raises(ValueError, match="Trivial modes"):
        s.distance_fluctuation(x, mode_subset=[5, 7])
    no_timeouts(s.ctx)


# ---- 6. placement, repetition, a failed structure, coincident atoms -----------------------------------------------------------
def test_bits_do_not_depend_on_batch_size_or_position_and_repeat(sc, torch):
    n_atoms = 100
    ff = sc.InvariantForceField(13.0)
    x = synthetic_coord(n_atoms, 660)
    others = make_coords(n_atoms, 4, seed=661)
    five = np.stack([others[0], others[1], others[2], x, others[3]])
    s1, _, _ = solved(sc, torch, x[None], ff)
    s5, _, _ = solved(sc, torch, five, ff)
    # the consumer's own property: the same eigenpairs at position 0 of a batch of 1 and at position 3 of a batch of 5 (the
    # solver itself may pick another GEMM tile for another batch size)
    s5.w[3].copy_(s1.w[0]); s5.v[3].copy_(s1.v[0])
    x1, x5 = gpu(torch, x[None]), gpu(torch, five)
    for subset in (None, np.arange(6, 36), np.array([9, 7, 9])):
        f1 = s1.distance_fluctuation(x1, mode_subset=subset).cpu().numpy()
        f5 = s5.distance_fluctuation(x5, mode_subset=subset).cpu().numpy()
        assert np.array_equal(f1[0], f5[3])
        assert np.array_equal(f5, s5.distance_fluctuation(x5, mode_subset=subset).cpu().numpy())
        assert np.array_equal(f1, s1.distance_fluctuation(x1, mode_subset=subset).cpu().numpy())


def test_a_nan_structure_gives_nan_and_leaves_its_neighbours_their_bits(sc, torch):
    n_atoms, batch = 100, 5
    coords = make_coords(n_atoms, batch, seed=670)
    ff = sc.InvariantForceField(13.0)
    x = gpu(torch, coords)
    good, _, _ = solved(sc, torch, coords, ff)
    ref = [good.distance_fluctuation(x).cpu().numpy(), good.distance_fluctuation(x, np.arange(6, 36)).cpu().numpy()]
    without = np.delete(coords, 2, axis=0)
    four, _, _ = solved(sc, torch, without, ff)
    bad = DeviceBatchSolver(n_atoms, batch, ff)
    bad.assemble(x)
    bad.matrix[2, 5, 7] = float("nan")
    bad.matrix[2, 7, 5] = float("nan")
    bad.eigh()
    got = [bad.distance_fluctuation(x), bad.distance_fluctuation(x, np.arange(6, 36))]
    with pytest.raises(np.linalg.LinAlgError):
        bad.finish()
    assert np.all(np.isnan(bad.w.cpu().numpy()[2]))
    off = ~np.eye(n_atoms, dtype=bool)
    for g, r in zip(got, ref):
        g = g.cpu().numpy()
        assert np.all(np.isnan(g[2][off]))                      # every pair; a distance to oneself stays exactly 0
        assert np.all(np.diag(g[2]) == 0.0)
        for b in (0, 1, 3, 4):
            assert np.array_equal(g[b], r[b])
    # and these are the bits the neighbours have in a batch without the failed structure (the consumer's own property: the
    # same eigenpairs, copied; the solver itself may pick another GEMM tile for another batch size)
    for i, b in enumerate((0, 1, 3, 4)):
        four.w[i].copy_(bad.w[b]); four.v[i].copy_(bad.v[b])
    f4 = four.distance_fluctuation(gpu(torch, without)).cpu().numpy()
    assert np.array_equal(got[0].cpu().numpy()[[0, 1, 3, 4]], f4)


def test_two_atoms_at_one_position_give_nan_for_that_pair_only(sc, torch):
    n_atoms = 100
    coords = make_coords(n_atoms, 2, seed=680)
    coords[1, 70] = coords[1, 3]                                # atoms 3 and 70 of structure 1: different tiles
    s = DeviceBatchSolver(n_atoms, 2, sc.InvariantForceField(13.0))
    x = gpu(torch, coords)
    # the modes come from the structure a hair away, which is connected and whose Hessian is finite (a spring of length 0
    # has no direction either); the consumer then gets the coordinates with the two atoms at one position
    clean = coords.copy()
    clean[1, 70] += 1e-3
    s.solve(gpu(torch, clean))
    s.finish()
    w, v = s.w.cpu().numpy(), s.v.cpu().numpy()
    assert np.all(np.isfinite(w)) and np.all(w[:, 6] > 1e-8 * w[:, -1])
    f = s.distance_fluctuation(x).cpu().numpy()
    nan = np.isnan(f[1])
    assert nan[3, 70] and nan[70, 3] and nan.sum() == 2
    assert not np.any(np.isnan(f[0]))
    ref = np_distfluct(w[1], v[1], np.arange(6, 3 * n_atoms), coords[1])
    assert np.array_equal(np.isnan(ref), nan)
    f[1][nan] = 0.0
    ok = ~nan
    msf = np_msf(w[1], v[1], np.arange(6, 3 * n_atoms), 3)
    tol = 4 * (3 * n_atoms - 6) * 3 * EPS
    assert np.all(np.abs(f[1] - np.where(ok, ref, 0.0)) <= tol * (msf[:, None] + msf[None, :]))
    check(f[0], w[0], v[0], np.arange(6, 3 * n_atoms), coords[0], "the neighbour of the structure with coincident atoms")


# ---- 7. RaggedBatchSolver ----------------------------------------------------------------------------------------------------------
RAGGED = (20, 33, 64, 100)


def _ragged(sc, torch, sizes, seeds, **kw):
    coords = [synthetic_coord(n, k) for n, k in zip(sizes, seeds)]
    s = RaggedBatchSolver(sizes, sc.InvariantForceField(13.0), **kw)
    packed = gpu(torch, np.concatenate(coords))
    s.solve(packed)
    s.finish()
    return s, coords, packed


def test_ragged_views_match_their_own_oracle_and_do_not_depend_on_the_neighbours(sc, torch):
    seeds = (700, 701, 702, 703)
    s, coords, packed = _ragged(sc, torch, RAGGED, seeds)
    assert s.order == 300
    per = s.results()
    # the same structures among other neighbours, in another order, in slots of the same order
    other_sizes, other_seeds = (100, 50, 20, 64, 33), (703, 710, 700, 702, 701)
    t, _, tpacked = _ragged(sc, torch, other_sizes, other_seeds, order=s.order)
    where = {0: 2, 1: 4, 2: 3, 3: 0}
    for b, tb in where.items():                                 # the consumer's own property: the same eigenpairs
        t.w[tb].copy_(s.w[b]); t.v[tb].copy_(s.v[b])
    for subset in (None, np.array([9, 7, 25, 9, 12])):
        views = s.distance_fluctuation(packed, mode_subset=subset)
        tviews = t.distance_fluctuation(tpacked, mode_subset=subset)
        assert len(views) == len(RAGGED)
        for b, n in enumerate(RAGGED):
            wb, vb = (z.cpu().numpy() for z in per[b])
            assert vb.shape == (3 * n, 3 * n)
            rows = np.arange(6, 3 * n) if subset is None else subset
            f = views[b].cpu().numpy()
            assert f.shape == (n, n)
            check(f, wb, vb, rows, coords[b], f"ragged [{b}] N = {n} {None if subset is None else list(subset)}")
            assert np.array_equal(f, tviews[where[b]].cpu().numpy())
        again = s.distance_fluctuation(packed, mode_subset=subset)
        assert all(np.array_equal(a.cpu().numpy(), g.cpu().numpy()) for a, g in zip(again, views))
    # the unprojected form, per structure, is the dcc expression bit for bit
    un = s.distance_fluctuation(packed, mode_subset=np.arange(6, 36), projected=False)
    cc = s.dcc(mode_subset=np.arange(6, 36), norm=False)
    for f, c in zip(un, cc):
        c = c.cpu().numpy()
        d = np.diag(c)
        assert np.array_equal(f.cpu().numpy(), (d[:, None] + d[None, :]) - 2 * c)
    no_timeouts(s.ctx)


def test_ragged_masses_and_the_packed_atom_scale(sc, torch):
    sizes = (20, 33)
    coords = [synthetic_coord(n, 720 + k) for k, n in enumerate(sizes)]
    masses = [np.random.RandomState(6).uniform(1.0, 20.0, 20), None]
    s = RaggedBatchSolver(sizes, sc.InvariantForceField(13.0), masses=masses)
    packed = gpu(torch, np.concatenate(coords))
    s.solve(packed)
    s.finish()
    per = s.results()
    ism = s.inv_sqrt_mass.cpu().numpy()
    views = s.distance_fluctuation(packed, atom_scale=s.inv_sqrt_mass)
    for b, n in enumerate(sizes):
        wb, vb = (z.cpu().numpy() for z in per[b])
        sc_b = ism[int(s.offsets[b]): int(s.offsets[b + 1])]
        check(views[b].cpu().numpy(), wb, vb, np.arange(6, 3 * n), coords[b], f"ragged masses [{b}]", scale=sc_b)
