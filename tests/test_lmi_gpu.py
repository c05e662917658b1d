"""
GPU tests of the generalized correlation (``k_lmi_whiten`` / ``k_mode_lmi`` of csrc/mode_lmi.hip) through the three layers:
``DeviceBatchSolver.generalized_correlation`` (``sc_dev_lmi_f64``), ``RaggedBatchSolver`` (``sc_batch_plan_lmi_f64``), ``RTB``
and ``EssentialDynamics`` (inherited), ``nma.generalized_correlation`` / ``ANM.generalized_correlation`` (``sc_modes_lmi``).

The specification is ``np_lmi`` of tests/lmi_model.py evaluated in float64 on the solver's OWN (w, v); the gate of a comparison
is 8 times the specification's float64-against-longdouble error on that very input, floor N eps (the module docstring
there).  The mutual information is checked on every off-diagonal entry against [I(r - gate), I(r + gate)], the gate scaled by
dI/dr without linearising it (``check_lmi``).  Every comparison prints measured / gate; the largest is in profiles/lmi.txt.

Sizes: N = 5 (one partial tile), 63 / 64 / 65 (around the 64-atom tile; 65: a one-atom second tile; 63, 65: odd N, rows only
8-byte aligned), 130 (a full off-diagonal tile plus partial ones).  Selections of 3, 4, 8, 9 (one staged group of rows and its
one-row tail), 20 and all modes.  Batches of at most 5.
"""
import numpy as np
import pytest

from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver
from tests import lmi_model as lm
from tests.test_batch_consumers_gpu import solved, window_case

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
    """A finished full-spectrum solver of lattice(n_atoms, seed 0 .. batch - 1) with host copies of (w, v): once per shape."""
    key = (n_atoms, batch)
    if key not in _SOLVED:
        coords = np.stack([lm.lattice(n_atoms, seed) for seed in range(batch)])
        s, w, v = solved(sc, torch, coords, sc.InvariantForceField(lm.CUTOFF))
        for a in (w, v):
            a.setflags(write=False)
        for b in range(batch):
            assert np.abs(w[b, :6]).max() <= 1e-12 * w[b, -1] and w[b, 6] >= 1e-3 * w[b, -1], "a disconnected network"
        _SOLVED[key] = (s, coords, w, v)
    return _SOLVED[key]


def exact_properties(torch, r, info):
    """Bit-level symmetry, the diagonal by definition, the range."""
    assert torch.equal(r, r.transpose(-1, -2)) and torch.equal(info, info.transpose(-1, -2))
    assert bool((r.diagonal(dim1=-2, dim2=-1) == 1.0).all()) and bool(torch.isposinf(info.diagonal(dim1=-2, dim2=-1)).all())
    assert bool(((r >= 0) & (r <= 1)).all()) and bool((info >= 0).all())


# ---- 1. against the specification: sizes x selections ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms", lm.SIZES)
def test_uniform_batch_matches_the_specification(sc, torch, n_atoms):
    s, _, w, v = batch_of(sc, torch, n_atoms)
    selections = dict(lm.subsets(n_atoms))
    selections["all"] = None
    worst = 0.0
    for name, subset in selections.items():
        r, info = s.generalized_correlation(subset), s.generalized_correlation(subset, information=True)
        assert r.is_cuda and r.dtype == torch.float64 and tuple(r.shape) == tuple(info.shape) == (2, n_atoms, n_atoms)
        exact_properties(torch, r, info)
        for b in range(2):
            rows = lm.pinv_rows(w[b]) if subset is None else subset
            if subset is None:
                assert np.array_equal(rows, np.arange(6, 3 * n_atoms))
            worst = max(worst, lm.check_lmi(r[b].cpu().numpy(), w[b], v[b], rows, f"N = {n_atoms} [{b}] {name} modes: r"))
            worst = max(worst, lm.check_lmi(info[b].cpu().numpy(), w[b], v[b], rows, f"N = {n_atoms} [{b}] {name} modes: I",
                                            information=True))
        # a repeated call gives the same bits
        assert torch.equal(s.generalized_correlation(subset), r)
    print(f"N = {n_atoms}: largest measured / gate = {worst:.3e}")
    # one mode, none: nothing can be whitened
    for subset in ([9], []):
        for information in (False, True):
            assert bool(torch.isnan(s.generalized_correlation(subset, information)).all())


@pytest.mark.parametrize("n_atoms", lm.SIZES)
def test_two_modes_give_nan_everywhere(sc, torch, n_atoms):
    """
    Two modes span a plane: every diagonal block has rank two and its last pivot is rounding noise, eps times the block's
    entry times the growth of the elimination.  The factorisation pivots on the diagonal, which bounds the growth: on LAPACK's
    eigenpairs of lattice(N) the last pivot is at most 3.3e-14 times its diagonal entry over modes (6, 7), (6, 8), (7, 11) and
    the sizes here, against the rule's 2^-40 = 9.1e-13.  (In the natural order it reached 1.2e-12 where the two modes move an
    atom along nearly one line in the xy plane, and such atoms came out whitened.)
    """
    s, _, w, v = batch_of(sc, torch, n_atoms)
    for information in (False, True):
        for subset in ([6, 7], [6, 8], [7, 11]):
            assert bool(torch.isnan(s.generalized_correlation(subset, information)).all()), (subset, information)
        got = s.generalized_correlation([6, 7], information)
        for b in range(2):
            spec = lm.np_lmi(w[b], v[b], [6, 7], information=information)
            print(f"N = {n_atoms} [{b}] two modes, information = {information}: {int((~torch.isnan(got[b])).sum())} entries of "
                  f"the device and {int((~np.isnan(spec)).sum())} of the specification are not NaN")
        assert bool(torch.isnan(got).all())


# ---- 2. behind an index range and behind a value window ----------------------------------------------------------------------------
def test_behind_an_index_range(sc, torch):
    n_atoms, batch = 65, 3
    coords = np.stack([lm.lattice(n_atoms, seed) for seed in range(batch)])
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(lm.CUTOFF), subset_by_index=(3, 25))
    assert w.shape == (batch, 23)
    r, info = s.generalized_correlation(), s.generalized_correlation(information=True)
    sub = s.generalized_correlation(mode_subset=[7, 20, 9, 11, 13, 8, 25, 6, 22])
    exact_properties(torch, r, info)
    for b in range(batch):
        lm.check_lmi(r[b].cpu().numpy(), w[b], v[b], np.arange(3, 23), f"subset_by_index (3, 25) [{b}] default: modes 6..25")
        lm.check_lmi(info[b].cpu().numpy(), w[b], v[b], np.arange(3, 23), f"subset_by_index (3, 25) [{b}] default: I",
                     information=True)
        lm.check_lmi(sub[b].cpu().numpy(), w[b], v[b], [4, 17, 6, 8, 10, 5, 22, 3, 19], f"subset_by_index (3, 25) [{b}] 9 modes")
    with pytest.raises(ValueError, match="was not solved"):
        s.generalized_correlation(mode_subset=[26])


def test_behind_a_value_window_the_padding_is_never_read(sc, torch):
    n_atoms, batch, K = 65, 5, 24
    coords, mats, lam, (vl, vu), expected = window_case(n_atoms, K, 3, batch=batch)
    assert expected.max() == K and expected.min() == 0 and len(set(expected)) >= 3
    s = DeviceBatchSolver(n_atoms, batch, sc.ParameterFreeForceField(), subset_by_value=(vl, vu), max_modes=K)
    s.matrix.copy_(torch.from_numpy(mats))
    s.eigh()
    r, info = s.generalized_correlation(), s.generalized_correlation(information=True)   # straight behind the solve
    s.finish()
    counts = s.counts.cpu().numpy()
    assert np.array_equal(counts, expected)
    for b in range(batch):
        s.v[b, counts[b]:] = float("nan")                    # what lies behind the count must not matter
    assert torch.equal(s.generalized_correlation().nan_to_num(nan=-1.0), r.nan_to_num(nan=-1.0))
    w, v = s.w.cpu().numpy(), s.v.cpu().numpy()
    for b in range(batch):
        k = counts[b]
        if k == 0:                                           # an empty window
            assert bool(torch.isnan(r[b]).all()) and bool(torch.isnan(info[b]).all())
            continue
        lm.check_lmi(r[b].cpu().numpy(), w[b], v[b], np.arange(k), f"window [{b}] count {k}: r")
        lm.check_lmi(info[b].cpu().numpy(), w[b], v[b], np.arange(k), f"window [{b}] count {k}: I", information=True)
        assert torch.equal(r[b].nan_to_num(nan=-1.0), r[b].T.nan_to_num(nan=-1.0))
    with pytest.raises(ValueError, match="subset_by_value"):
        s.generalized_correlation(mode_subset=[7])


# ---- 3. bits ---------------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_batch_size_position_or_layout(sc, torch):
    ff = sc.InvariantForceField(lm.CUTOFF)
    n_atoms = 130
    s1, _, _ = solved(sc, torch, np.array(lm.lattice(n_atoms, 0))[None], ff)
    s3, _, _ = solved(sc, torch, np.stack([lm.lattice(n_atoms, seed) for seed in range(3)]), ff)
    # the consumer's own property: the same eigenpairs alone, first of three and last of three
    for b in (0, 2):
        s3.w[b].copy_(s1.w[0])
        s3.v[b].copy_(s1.v[0])
    selections = (None, lm.subsets(n_atoms)["9"], lm.subsets(n_atoms)["20"])
    for subset in selections:
        for information in (False, True):
            p1, p3 = s1.generalized_correlation(subset, information), s3.generalized_correlation(subset, information)
            assert bool(torch.isfinite(p1[0][~torch.eye(n_atoms, dtype=torch.bool, device=p1.device)]).all())
            assert torch.equal(p1[0], p3[0]) and torch.equal(p1[0], p3[2]) and not torch.equal(p1[0], p3[1])
    # a weight-zero row is selected out, not multiplied by zero
    ref = s3.generalized_correlation()
    s3.v[1, 0:6] = float("nan")                              # the trivial rows: under the pinv threshold
    assert torch.equal(s3.generalized_correlation(), ref)

    # a ragged batch against the uniform solves of its members: the slots' eigenpairs replaced by the uniform solvers' own
    sizes = lm.RAGGED_SIZES
    rag = RaggedBatchSolver(sizes, ff)
    rag.solve(torch.from_numpy(np.concatenate([lm.lattice(n) for n in sizes])).cuda())
    rag.finish()
    m = 3 * max(sizes)
    uniform = []
    for b, n in enumerate(sizes):
        u = s1 if n == n_atoms else solved(sc, torch, np.array(lm.lattice(n))[None], ff)[0]
        uniform.append(u)
        rag.w[b, : 3 * n].copy_(u.w[0])
        rag.v[b, : 3 * n, : 3 * n].copy_(u.v[0])
    assert tuple(rag.v.shape) == (3, m, m)
    for subset in selections:
        for information in (False, True):
            got = rag.generalized_correlation(subset, information)
            assert [tuple(t.shape) for t in got] == [(n, n) for n in sizes]
            assert got[0].untyped_storage().data_ptr() == got[2].untyped_storage().data_ptr()
            for b, n in enumerate(sizes):
                # (under the covariance rule the slot lists all its 390 rows, the uniform solve of a smaller member 3 n: the
                # rows behind the member's own carry no weight and add nothing, in the pair kernel and in the tensors alike)
                assert torch.equal(got[b], uniform[b].generalized_correlation(subset, information)[0]), (n, information)
    # the same member in another plan, at another position and beside other neighbours
    other = RaggedBatchSolver((70, 30), ff)
    other.solve(torch.from_numpy(np.concatenate([lm.lattice(70), lm.lattice(30, 1)])).cuda())
    other.finish()
    other.w[0, :210].copy_(uniform[1].w[0])
    other.v[0, :210, :210].copy_(uniform[1].v[0])
    for subset in selections:
        assert torch.equal(other.generalized_correlation(subset)[0], rag.generalized_correlation(subset)[1])
    for information in (False, True):
        got = rag.generalized_correlation(information=information)
        for b, n in enumerate(sizes):
            w, v = (t.cpu().numpy() for t in rag.results()[b])
            assert w.shape == (3 * n,) and v.shape == (3 * n, 3 * n)
            lm.check_lmi(got[b].cpu().numpy(), w, v, lm.pinv_rows(w), f"ragged (30, 70, 130) [{b}] I = {information}",
                         information=information)


# ---- 4. a structure that cannot be solved ------------------------------------------------------------------------------------------------
def test_a_non_finite_matrix_gives_nan_and_leaves_the_neighbours_alone(sc, torch):
    n_atoms, batch = 65, 3
    ff = sc.InvariantForceField(lm.CUTOFF)
    mats = np.stack([sc.compute_hessian(np.array(lm.lattice(n_atoms, seed)), ff)[0] for seed in range(batch)])

    def run(matrices):
        s = DeviceBatchSolver(n_atoms, batch, ff)
        s.matrix.copy_(torch.from_numpy(matrices))
        s.eigh()
        return s, s.generalized_correlation(), s.generalized_correlation(information=True), \
            s.generalized_correlation(lm.subsets(n_atoms)["9"])

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
            assert torch.equal(g[b], r[b]) and not bool(torch.isnan(g[b]).any())


# ---- 5. the invariance on the device: masses ---------------------------------------------------------------------------------------------
def test_a_mass_weighted_solver_gives_the_cartesian_result(sc, torch):
    n_atoms, batch = 63, 2
    coords = np.stack([lm.lattice(n_atoms, seed) for seed in range(batch)])
    masses = np.random.RandomState(3).uniform(10.0, 20.0, (batch, n_atoms))
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(lm.CUTOFF), masses=masses)
    r, info = s.generalized_correlation(), s.generalized_correlation(information=True)
    exact_properties(torch, r, info)
    for b in range(batch):
        rows = lm.pinv_rows(w[b])
        assert np.array_equal(rows, np.arange(6, 3 * n_atoms))
        t = s.inv_sqrt_mass[b].cpu().numpy()
        # the specification on M^-1/2 C M^-1/2; the kernel never saw the masses
        lm.check_lmi(r[b].cpu().numpy(), w[b], v[b], rows, f"masses [{b}] against the Cartesian covariance: r", scale=t)
        lm.check_lmi(info[b].cpu().numpy(), w[b], v[b], rows, f"masses [{b}] against the Cartesian covariance: I", scale=t,
                     information=True)


# ---- 6. the one-model path, RTB, EssentialDynamics ---------------------------------------------------------------------------------------
def test_the_one_model_path_is_the_batch_of_one(sc, torch):
    n_atoms = 65
    coord = np.array(lm.lattice(n_atoms))
    ff = sc.InvariantForceField(lm.CUTOFF)
    anm = sc.ANM(coord, ff)
    wa, va = anm.eigen()
    one = DeviceBatchSolver(n_atoms, 1, ff)
    one.w[0].copy_(torch.from_numpy(wa))
    one.v[0].copy_(torch.from_numpy(va))
    for subset in (None, lm.subsets(n_atoms)["9"], lm.subsets(n_atoms)["3"]):
        for information in (False, True):
            got = sc.nma.generalized_correlation(anm, subset, information)
            assert isinstance(got, np.ndarray) and got.shape == (n_atoms, n_atoms)
            assert np.array_equal(got, anm.generalized_correlation(subset, information))
            assert np.array_equal(got, one.generalized_correlation(subset, information)[0].cpu().numpy())
    lm.check_lmi(sc.nma.generalized_correlation(anm), wa, va, lm.pinv_rows(wa), "nma.generalized_correlation(anm)")
    assert np.isnan(sc.nma.generalized_correlation(anm, mode_subset=[])).all()
    with pytest.raises(IndexError):
        sc.nma.generalized_correlation(anm, mode_subset=[7, 3 * n_atoms])
    assert anm._covariance is None                           # no (3N, 3N) matrix was formed on the way
    with pytest.raises(ValueError, match="Instance of ANM class expected"):
        sc.nma.generalized_correlation(sc.GNM(coord, ff))
    gnm = DeviceBatchSolver(n_atoms, 1, ff, dim=1)
    with pytest.raises(ValueError, match=r"abs\(dcc\(norm=True\)\)"):
        gnm.generalized_correlation()


def test_rtb_and_essential_dynamics_inherit_the_method(sc, torch):
    from tests import ensemble_model as em

    n_atoms = 60
    rtb = sc.RTB(np.array(lm.lattice(n_atoms)), sc.InvariantForceField(lm.CUTOFF), np.arange(n_atoms) // 5)
    rtb.solve()
    w, v = (t[0].cpu().numpy() for t in rtb.finish())
    assert v.shape == (rtb.nr, 3 * n_atoms) and rtb.nr == 72
    rows = lm.pinv_rows(w)
    assert np.array_equal(rows, np.arange(6, rtb.nr))
    r = rtb.generalized_correlation()
    assert tuple(r.shape) == (1, n_atoms, n_atoms) and torch.equal(r[0], r[0].T)
    lm.check_lmi(r[0].cpu().numpy(), w, v, rows, "RTB N = 60, blocks of 5: the expanded modes")

    ens = sc.Ensemble(em.perturbed_ensemble(7, 40))
    assert ens.superpose()[1]
    ed = ens.pca(15)
    w, v = (t[0].cpu().numpy() for t in ed.finish())
    r, info = ed.generalized_correlation(), ed.generalized_correlation(information=True)
    assert tuple(r.shape) == (1, 7, 7)
    exact_properties(torch, r, info)
    # (every solved row is a component: subset_by_index, none of them trivial)
    lm.check_lmi(r[0].cpu().numpy(), w, v, np.arange(15), "EssentialDynamics M = 40, N = 7, 15 components: r")
    lm.check_lmi(info[0].cpu().numpy(), w, v, np.arange(15), "EssentialDynamics M = 40, N = 7, 15 components: I",
                 information=True)
