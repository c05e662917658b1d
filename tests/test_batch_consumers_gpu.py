"""
GPU tests for the batch consumers of ``DeviceBatchSolver`` (``csrc/batch_consumers.hip`` through ``sc_dev_modes_*``):
mean-square fluctuations, B-factors, dynamic cross-correlations and frequencies of every structure of a batch, from the
solver's own ``w`` / ``v`` / ``counts`` tensors.

Two references throughout.

(a) The arithmetic alone: the solver's own eigenpairs copied to the host and the two formulas

        msf[b, a]    = sum_r s[b, r] sum_d V[b, r, dim a + d]^2
        dcc[b, a, c] = sum_r s[b, r] sum_d V[b, r, dim a + d] V[b, r, dim c + d]

    evaluated in NumPy float64, s = 1 / lambda on the selected rows.  The bounds are derived, not fitted: MSF is a sum of
    rows x dim non-negative terms, so |msf - ref| <= 4 rows dim 2^-53 ref; DCC terms change sign, by Cauchy-Schwarz
    |dcc[a, c] - ref| <= 4 rows dim 2^-53 sqrt(C_aa C_cc) on the unnormalised result, and the normalised one (entries at
    most 1) within 3 x 4 rows dim 2^-53 absolute.  The factor 4 is slack for the fused multiply-adds and the division.

(b) The meaning: the reference's own ProDy fixtures for 1l2y (the files tests/test_consumers_gpu.py reads, under the same
    ``np.allclose``) and the single-model API, ``ANM(coord, ff).mean_square_fluctuation()`` etc., per structure.

The figures are printed before they are asserted (``pytest -s``).
"""
import numpy as np
import pytest

from springcraft_amd.batch import DeviceBatchSolver
from tests.util import load_csv, structures, synthetic_coord

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
K_B = 1.380649e-23
N_A = 6.02214076e23


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def ca():
    return structures()["1l2y_coord"]


# ---- reference (a): the formulas on the solver's own eigenpairs ------------------------------------------------------
def np_msf(w, v, rows, dim):
    s = 1.0 / w[rows]
    return ((v[rows] ** 2) * s[:, None]).sum(axis=0).reshape(-1, dim).sum(axis=1)


def np_dcc(w, v, rows, dim):
    s = 1.0 / w[rows]
    n = v.shape[1] // dim
    c = np.zeros((n, n))
    vr = v[rows]
    for d in range(dim):
        vd = np.ascontiguousarray(vr[:, d::dim])      # (a strided operand would take matmul off BLAS)
        c += np.ascontiguousarray(vd.T * s) @ vd
    return c


def pinv_rows(w):
    return np.nonzero(np.abs(w) > 1e-6 * np.abs(w).max())[0]


def check_msf(got, ref, rows, dim, what):
    tol = 4 * max(len(rows), 1) * dim * EPS
    err = np.abs(got - ref)
    rel = (err / np.where(ref > 0, ref, 1.0)).max() if len(ref) else 0.0
    print(f"{what}: msf max rel err {rel:.3e}, bound {tol:.3e}")
    assert np.all(err <= tol * np.abs(ref)), what


def check_dcc(got, ref, rows, dim, what):
    """got, ref unnormalised; then the normalised pair derived from each."""
    tol = 4 * max(len(rows), 1) * dim * EPS
    d = np.sqrt(np.diag(ref))
    scale = np.outer(d, d)
    err = np.abs(got - ref)
    print(f"{what}: dcc max err / sqrt(C_aa C_cc) {(err / np.where(scale > 0, scale, 1.0)).max():.3e}, bound {tol:.3e}")
    assert np.all(err <= tol * scale), what


def check_dcc_norm(got, ref, rows, dim, what):
    tol = 3 * 4 * max(len(rows), 1) * dim * EPS
    d = np.sqrt(np.diag(ref))
    refn = ref / np.outer(d, d)
    err = np.abs(got - refn).max()
    print(f"{what}: normalised dcc max abs err {err:.3e}, bound {tol:.3e}")
    assert err <= tol, what


def make_coords(n_atoms, batch, seed=0):
    return np.stack([synthetic_coord(n_atoms, seed + b) for b in range(batch)])


def solved(sc, torch, coords, ff, dim=3, masses=None, **kw):
    """A solver with ``coords`` solved and finished, and host copies of its w, v."""
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    s = DeviceBatchSolver(coords.shape[1], coords.shape[0], ff, dim=dim, masses=masses, **kw)
    s.solve(torch.from_numpy(coords).cuda())
    s.finish()
    return s, s.w.cpu().numpy(), s.v.cpu().numpy()


# ---- (a) across dims, sizes (odd and even m), batch sizes, masses, lists ------------------------------------------------
@pytest.mark.parametrize("dim,n_atoms,batch,with_masses", [
    (3, 100, 5, False), (3, 301, 1, True), (3, 301, 5, False), (3, 512, 16, False), (3, 100, 16, True),
    (1, 100, 1, False), (1, 301, 16, True), (1, 512, 5, False)])
def test_msf_and_dcc_match_the_formulas_on_the_solvers_own_eigenpairs(sc, torch, dim, n_atoms, batch, with_masses):
    ntriv = 6 if dim == 3 else 1
    m = dim * n_atoms
    coords = make_coords(n_atoms, batch, seed=3)
    masses = np.random.RandomState(1).uniform(1.0, 20.0, (batch, n_atoms)) if with_masses else None
    ff = sc.InvariantForceField(13.0 if dim == 3 else 10.0)
    s, w, v = solved(sc, torch, coords, ff, dim=dim, masses=masses)
    rs = np.random.RandomState(7)
    shuffled = rs.permutation(np.arange(ntriv, ntriv + 40))
    lists = {
        "default": None,
        "arange(6, 36)": np.arange(6, 36),
        "unsorted with a repeat": np.concatenate([shuffled, [ntriv + 3, ntriv + 3, m - 1]]),
    }
    for name, subset in lists.items():
        rows = np.arange(ntriv, m) if subset is None else np.asarray(subset)
        msf = s.mean_square_fluctuation(mode_subset=subset).cpu().numpy()
        raw = s.dcc(mode_subset=subset, norm=False).cpu().numpy()
        nrm = s.dcc(mode_subset=subset, norm=True).cpu().numpy()
        assert msf.shape == (batch, n_atoms) and raw.shape == (batch, n_atoms, n_atoms)
        for b in range(batch):
            tag = f"dim {dim} n {n_atoms} batch {batch} [{b}] {name}"
            check_msf(msf[b], np_msf(w[b], v[b], rows, dim), rows, dim, tag)
            drows = pinv_rows(w[b]) if subset is None else rows      # the covariance rule of dcc()'s default
            ref = np_dcc(w[b], v[b], drows, dim)
            check_dcc(raw[b], ref, drows, dim, tag)
            check_dcc_norm(nrm[b], ref, drows, dim, tag)
    assert np.array_equal(s.bfactor().cpu().numpy(),
                          (s.mean_square_fluctuation() * ((8 * np.pi**2) / 3)).cpu().numpy())


# ---- (b) the reference's fixtures and the single-model API ----------------------------------------------------------------
def _1l2y_batch(ca):
    pert = ca + np.random.RandomState(4).randn(*ca.shape) * 0.05
    return np.stack([synthetic_coord(len(ca), 9), ca, pert, synthetic_coord(len(ca), 10), ca])


def test_anm_batch_reproduces_the_prody_fixtures_and_the_single_model_api(sc, torch, ca):
    """tests/test_anm.py:160-209 of the reference (ProDy, ANM 13 A on 1l2y), 1l2y at positions 1 and 4 of a batch of 5."""
    coords = _1l2y_batch(ca)
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(13))
    name = "prody_anm_13_ang_cutoff"
    evals = load_csv(f"{name}_evals_1l2y.csv.gz")
    freq = s.frequencies().cpu().numpy()
    msf = s.mean_square_fluctuation().cpu().numpy()
    bfac = s.bfactor().cpu().numpy()
    dcc = s.dcc().cpu().numpy()
    dabs = s.dcc(norm=False).cpu().numpy()
    dsub = s.dcc(mode_subset=np.arange(6, 36)).cpu().numpy()
    tem = s.dcc(tem=300, tem_factors=K_B * N_A).cpu().numpy()
    mtem = s.mean_square_fluctuation(tem=300, tem_factors=K_B * N_A).cpu().numpy()
    msub = s.mean_square_fluctuation(mode_subset=np.arange(11, 33)).cpu().numpy()
    for b in (1, 4):
        assert np.allclose(freq[b, 6:], np.sqrt(evals[6:]) / (2 * np.pi))
        assert np.allclose(msf[b], load_csv(f"{name}_fluctuations_1l2y.csv.gz"))
        assert np.allclose(dcc[b], load_csv(f"{name}_dcc_norm_1l2y.csv.gz"))
        assert np.allclose(dabs[b], load_csv(f"{name}_dcc_absolute_1l2y.csv.gz"))
        assert np.allclose(dsub[b], load_csv(f"{name}_dcc_norm_subset_1l2y.csv.gz"))
    for b in range(len(coords)):
        anm = sc.ANM(coords[b], sc.InvariantForceField(13))
        assert np.allclose(freq[b, 6:], anm.frequencies()[6:])
        assert np.allclose(msf[b], anm.mean_square_fluctuation())
        assert np.allclose(bfac[b], anm.bfactor())
        assert np.allclose(dcc[b], anm.dcc())
        assert np.allclose(dabs[b], anm.dcc(norm=False))
        assert np.allclose(dsub[b], anm.dcc(mode_subset=np.arange(6, 36)))
        assert np.allclose(tem[b], anm.dcc(tem=300, tem_factors=K_B * N_A))
        assert np.allclose(mtem[b], anm.mean_square_fluctuation(tem=300, tem_factors=K_B * N_A))
        assert np.allclose(msub[b], anm.mean_square_fluctuation(mode_subset=np.arange(11, 33)))


@pytest.mark.parametrize("cutoff", [4, 7, 13])
def test_gnm_batch_reproduces_the_prody_fixtures_and_the_single_model_api(sc, torch, ca, cutoff):
    """tests/test_gnm.py:107-152 of the reference; the 13 A subset file is left out as in tests/test_consumers_gpu.py."""
    coords = _1l2y_batch(ca)
    # (cutoff 4 leaves the random neighbours of the batch disconnected: their own results are not looked at)
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(cutoff), dim=1)
    name = f"prody_gnm_{cutoff}_ang_cutoff"
    msf = s.mean_square_fluctuation().cpu().numpy()
    dcc = s.dcc().cpu().numpy()
    dabs = s.dcc(norm=False).cpu().numpy()
    dsub = s.dcc(mode_subset=np.arange(1, 17)).cpu().numpy()
    freq = s.frequencies().cpu().numpy()
    for b in (1, 4):
        assert np.allclose(msf[b], load_csv(f"{name}_fluctuations_1l2y.csv.gz"))
        assert np.allclose(dcc[b], load_csv(f"{name}_dcc_norm_1l2y.csv.gz"))
        if cutoff != 13:
            assert np.allclose(dsub[b], load_csv(f"{name}_dcc_norm_subset_1l2y.csv.gz"))
        assert np.allclose(dabs[b], load_csv(f"{name}_dcc_absolute_1l2y.csv.gz"))
    for b in (1, 2, 4):
        gnm = sc.GNM(coords[b], sc.InvariantForceField(cutoff))
        assert np.allclose(msf[b], gnm.mean_square_fluctuation())
        assert np.allclose(dcc[b], gnm.dcc())
        assert np.allclose(dabs[b], gnm.dcc(norm=False))
        assert np.allclose(freq[b, 1:], gnm.frequencies()[1:])
        assert np.allclose(s.bfactor().cpu().numpy()[b], gnm.bfactor())


# ---- partial spectrum ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0, 25), (6, 25)])
def test_subset_by_index_solver_defaults_explicit_lists_and_errors(sc, torch, lo, hi):
    n_atoms, batch, dim = 100, 5, 3
    coords = make_coords(n_atoms, batch, seed=20)
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(13.0), subset_by_index=(lo, hi))
    assert w.shape == (batch, hi - lo + 1)
    default_rows = np.arange(max(6, lo) - lo, hi - lo + 1)
    explicit = np.array([9, 7, 25, 9, 12])
    for subset, rows in ((None, default_rows), (explicit, explicit - lo), (np.arange(6, 26), default_rows)):
        msf = s.mean_square_fluctuation(mode_subset=subset).cpu().numpy()
        raw = s.dcc(mode_subset=subset, norm=False).cpu().numpy()
        nrm = s.dcc(mode_subset=subset).cpu().numpy()
        for b in range(batch):
            tag = f"subset_by_index ({lo}, {hi}) [{b}] {None if subset is None else list(subset)}"
            check_msf(msf[b], np_msf(w[b], v[b], rows, dim), rows, dim, tag)
            ref = np_dcc(w[b], v[b], rows, dim)
            check_dcc(raw[b], ref, rows, dim, tag)
            check_dcc_norm(nrm[b], ref, rows, dim, tag)
    # against the single-model API on the same modes (another eigensolver path: not a rounding-level check)
    anm = sc.ANM(coords[2], sc.InvariantForceField(13.0))
    assert np.allclose(s.mean_square_fluctuation().cpu().numpy()[2], anm.mean_square_fluctuation(mode_subset=np.arange(6, 26)))
    assert np.allclose(s.dcc().cpu().numpy()[2], anm.dcc(mode_subset=np.arange(6, 26)))
    f = s.frequencies().cpu().numpy()
    assert np.allclose(f[2, 6 - lo:], anm.frequencies()[6:26]) and np.all(np.isfinite(f))
    with pytest.raises(ValueError, match=f"{lo}\\.\\.{hi}"):
        s.mean_square_fluctuation(mode_subset=[7, 26])
    with pytest.raises(ValueError, match=f"{lo}\\.\\.{hi}"):
        s.dcc(mode_subset=[7, 299])
    with pytest.raises(ValueError, match="Trivial modes"):
        s.mean_square_fluctuation(mode_subset=[5, 7])
    with pytest.raises(ValueError, match="Trivial modes"):
        s.dcc(mode_subset=np.arange(0, 10))


def test_consumers_need_the_eigenvectors(sc, torch):
    coords = make_coords(50, 2)
    s = DeviceBatchSolver(50, 2, sc.InvariantForceField(13.0), want_vectors=False)
    s.solve(torch.from_numpy(coords).cuda())
    for call in (s.mean_square_fluctuation, s.bfactor, s.dcc):
        with pytest.raises(ValueError, match="want_vectors"):
            call()
    s.finish()
    assert s.frequencies().shape == (2, 150)


# ---- eigenvalue window --------------------------------------------------------------------------------------------------
def window_case(n_atoms, max_modes, dim, batch=6):
    """
    Matrices (oracle, ParameterFree force field) and a window (vl, vu] chosen from their LAPACK eigenvalues: vl leaves the
    trivial modes out, vu sits in the gap above the max_modes-th non-trivial eigenvalue of the structure whose spectrum is
    lowest there, so that this structure fills its slot exactly and no structure exceeds it; one matrix is scaled by 1e3,
    which lifts its whole non-trivial spectrum above vu (count 0) and leaves its trivial eigenvalues far below vl.
    """
    from oracle import enm_oracle as orc

    coords = np.stack([synthetic_coord(n_atoms, 31 + b) for b in range(batch)])
    build = orc.compute_hessian if dim == 3 else orc.compute_kirchhoff
    mats = np.stack([build(c, orc.parameter_free_ff())[0] for c in coords])
    lam = np.stack([np.linalg.eigvalsh(a) for a in mats])
    ntriv = 6 if dim == 3 else 1
    k = ntriv + max_modes
    lowest = int(np.argmin(lam[:, k - 1]))
    empty = (lowest + 1) % batch
    mats[empty] *= 1e3
    lam[empty] *= 1e3
    scale = np.abs(lam[np.arange(batch) != empty]).max()
    vl = 1e-6 * scale
    top = lam[lowest, k - 1]
    above = lam[lam > top].min()
    vu = 0.5 * (top + above)
    assert above - top > 1e-9 * scale and lam[:, ntriv:].min() > 10 * vl and np.abs(lam[:, :ntriv]).max() < 0.1 * vl
    expected = np.array([np.sum((l > vl) & (l <= vu)) for l in lam])
    assert expected.max() == max_modes and expected[lowest] == max_modes and expected[empty] == 0
    assert len(set(expected)) >= 3
    return coords, mats, lam, (vl, vu), expected


@pytest.mark.parametrize("dim", [3, 1])
def test_value_window_solver_reads_the_counts_on_the_device(sc, torch, dim):
    """
    Structures with different counts, one empty window and one that fills max_modes exactly.  The window is chosen on the
    CPU from LAPACK eigenvalues of the same matrices: scaled copies of the coordinates shift the spectra against each other.
    """
    n_atoms, max_modes = 101, 24
    coords, mats, lam, (vl, vu), expected = window_case(n_atoms, max_modes, dim)
    ff = sc.ParameterFreeForceField()
    s = DeviceBatchSolver(n_atoms, len(coords), ff, dim=dim, subset_by_value=(vl, vu), max_modes=max_modes)
    # (the matrices the window was chosen for, the scaled one included; the assembly has its own tests)
    s.matrix.copy_(torch.from_numpy(mats))
    s.eigh()
    # the consumers are enqueued straight behind the solve, before anything is known on the host
    msf = s.mean_square_fluctuation()
    raw = s.dcc(norm=False)
    nrm = s.dcc()
    s.finish()
    counts = s.counts.cpu().numpy()
    print("window counts", counts, "expected", expected)
    assert np.array_equal(counts, expected)
    w, v = s.w.cpu().numpy(), s.v.cpu().numpy()
    assert torch.isfinite(msf).all() and torch.isfinite(raw).all()
    msf, raw, nrm = msf.cpu().numpy(), raw.cpu().numpy(), nrm.cpu().numpy()
    for b in range(len(coords)):
        rows = np.arange(counts[b])
        assert np.all(np.isnan(w[b, counts[b]:]))
        tag = f"window dim {dim} [{b}] count {counts[b]}"
        if counts[b] == 0:
            assert np.all(msf[b] == 0.0) and np.all(raw[b] == 0.0)
            assert np.all(np.isnan(nrm[b]))                 # 0 / 0, as in NumPy
            continue
        check_msf(msf[b], np_msf(w[b], v[b], rows, dim), rows, dim, tag)
        ref = np_dcc(w[b], v[b], rows, dim)
        check_dcc(raw[b], ref, rows, dim, tag)
        check_dcc_norm(nrm[b], ref, rows, dim, tag)
        assert np.all(np.isfinite(nrm[b]))
    with pytest.raises(ValueError, match="subset_by_value"):
        s.mean_square_fluctuation(mode_subset=[7, 8])
    with pytest.raises(ValueError, match="subset_by_value"):
        s.dcc(mode_subset=np.arange(6, 12))


# ---- the covariance rule per structure ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 3])
def test_dcc_default_follows_the_pinv_rule_per_structure(sc, torch, dim):
    """
    tests/test_consumers_gpu.py::test_dcc_all_modes_follows_the_pinv_rule_on_a_nearly_disconnected_network in a batch: two
    clusters joined by one very weak spring next to a well-connected network whose matrix is scaled by 1e8.  The weak
    structure drops a NON-trivial mode and nothing else: the threshold is 1e-6 of its own max|lambda|; 1e-6 of the batch's
    would drop every one of its modes.
    """
    rs = np.random.RandomState(11)
    a = rs.rand(12, 3) * 6.0
    b = rs.rand(12, 3) * 6.0 + np.array([40.0, 0.0, 0.0])
    coord = np.concatenate([a, b])
    weak = sc.PatchedForceField(sc.InvariantForceField(9.0), contact_pair_on=np.array([[0, 12]]),
                                force_constants=np.array([1e-9]))
    dense = synthetic_coord(24, 5, box=8.0)
    if dim == 1:
        m_weak = sc.GNM(coord, weak).kirchhoff.copy()
        m_dense = 1e8 * sc.GNM(dense, sc.InvariantForceField(9.0)).kirchhoff.copy()
    else:
        m_weak = sc.ANM(coord, weak).hessian.copy()
        m_dense = 1e8 * sc.ANM(dense, sc.InvariantForceField(9.0)).hessian.copy()
    mats = np.stack([m_dense, m_weak, m_dense])
    ntriv = 6 if dim == 3 else 1
    lw = np.linalg.eigvalsh(m_weak)
    assert np.sum(np.abs(lw) <= 1e-6 * np.abs(lw).max()) > ntriv           # a non-trivial mode is dropped ...
    ld = np.linalg.eigvalsh(m_dense)
    assert np.all(np.abs(lw) <= 1e-6 * np.abs(ld).max())                   # ... by ITS OWN maximum, not the batch's
    s = DeviceBatchSolver(24, 3, sc.InvariantForceField(9.0), dim=dim)
    s.matrix.copy_(torch.from_numpy(mats))
    s.eigh()
    raw = s.dcc(norm=False)
    nrm = s.dcc()
    s.finish()
    raw, nrm = raw.cpu().numpy(), nrm.cpu().numpy()
    w, v = s.w.cpu().numpy(), s.v.cpu().numpy()
    for i, mat in enumerate(mats):
        cov = np.linalg.pinv(mat, hermitian=True, rcond=1e-6)
        n = 24
        tr = cov.reshape(n, dim, n, dim).swapaxes(1, 2).trace(axis1=2, axis2=3)
        d = np.sqrt(np.diag(tr))
        assert np.allclose(raw[i], tr, rtol=1e-8, atol=1e-9 * np.abs(tr).max())
        assert np.allclose(nrm[i], tr / np.outer(d, d), rtol=1e-8, atol=1e-9)
        rows = pinv_rows(w[i])
        ref = np_dcc(w[i], v[i], rows, dim)
        check_dcc(raw[i], ref, rows, dim, f"pinv rule dim {dim} [{i}]")
        check_dcc_norm(nrm[i], ref, rows, dim, f"pinv rule dim {dim} [{i}]")
    assert len(pinv_rows(w[1])) < dim * 24 - ntriv


# ---- a failed structure ---------------------------------------------------------------------------------------------------
def test_a_nan_structure_gives_nan_and_leaves_its_neighbours_their_bits(sc, torch):
    n_atoms, batch = 100, 5
    coords = make_coords(n_atoms, batch, seed=40)
    ff = sc.InvariantForceField(13.0)
    good, _, _ = solved(sc, torch, coords, ff)
    ref = [good.mean_square_fluctuation().cpu().numpy(), good.dcc().cpu().numpy(),
           good.dcc(mode_subset=np.arange(6, 36), norm=False).cpu().numpy()]
    bad = DeviceBatchSolver(n_atoms, batch, ff)
    bad.assemble(torch.from_numpy(coords).cuda())
    bad.matrix[2, 5, 7] = float("nan")
    bad.matrix[2, 7, 5] = float("nan")
    bad.eigh()
    got = [bad.mean_square_fluctuation(), bad.dcc(), bad.dcc(mode_subset=np.arange(6, 36), norm=False)]
    with pytest.raises(np.linalg.LinAlgError):
        bad.finish()
    assert np.all(np.isnan(bad.w.cpu().numpy()[2]))
    for g, r in zip(got, ref):
        g = g.cpu().numpy()
        assert np.all(np.isnan(g[2]))
        for b in (0, 1, 3, 4):
            assert np.array_equal(g[b], r[b])


# ---- reproducibility --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n_atoms", [(3, 301), (1, 512)])
def test_results_do_not_depend_on_the_position_and_repeat_bit_for_bit(sc, torch, dim, n_atoms):
    ff = sc.InvariantForceField(13.0 if dim == 3 else 10.0)
    x = synthetic_coord(n_atoms, 50)
    others = make_coords(n_atoms, 3, seed=51)
    five = np.stack([x, others[0], others[1], x, others[2]])
    s5, w5, v5 = solved(sc, torch, five, ff, dim=dim)
    s1, w1, v1 = solved(sc, torch, x[None], ff, dim=dim)
    # the consumers' own reproducibility: the same eigenpairs in a batch of 1 and at two positions of a batch of 5
    # (the solver itself may pick another GEMM tile for another batch size)
    s5.w[0].copy_(s1.w[0]); s5.v[0].copy_(s1.v[0])
    s5.w[3].copy_(s1.w[0]); s5.v[3].copy_(s1.v[0])
    w, v = s1.w.cpu().numpy()[0], s1.v.cpu().numpy()[0]
    ntriv = 6 if dim == 3 else 1
    for subset in (None, np.arange(ntriv, ntriv + 30)):
        m1 = s1.mean_square_fluctuation(mode_subset=subset).cpu().numpy()
        m5 = s5.mean_square_fluctuation(mode_subset=subset).cpu().numpy()
        assert np.array_equal(m1[0], m5[3]) and np.array_equal(m1[0], m5[0])
        assert np.array_equal(m5, s5.mean_square_fluctuation(mode_subset=subset).cpu().numpy())
        for norm in (False, True):
            d1 = s1.dcc(mode_subset=subset, norm=norm).cpu().numpy()
            d5 = s5.dcc(mode_subset=subset, norm=norm).cpu().numpy()
            assert np.array_equal(d5[0], d5[3])
            assert np.array_equal(d5, s5.dcc(mode_subset=subset, norm=norm).cpu().numpy())
            assert np.array_equal(d1, s1.dcc(mode_subset=subset, norm=norm).cpu().numpy())
            rows = pinv_rows(w) if subset is None else np.asarray(subset)
            ref = np_dcc(w, v, rows, dim)
            for got, tag in ((d1[0], "batch of 1"), (d5[3], "position 3 of 5")):
                (check_dcc_norm if norm else check_dcc)(got, ref, rows, dim, f"dim {dim} n {n_atoms} {tag}")


def test_a_small_budget_forces_slabs_and_chunks_without_changing_the_placement_independence(sc, torch):
    """n_atoms = 301 (m = 903, odd): 64 KiB of pack budget hold 4 rows, so every structure is a slab and takes 225 chunks."""
    n_atoms, dim = 301, 3
    ff = sc.InvariantForceField(13.0)
    x = synthetic_coord(n_atoms, 60)
    others = make_coords(n_atoms, 2, seed=61)
    coords = np.stack([x, others[0], others[1], x])
    s, w, v = solved(sc, torch, coords, ff)
    s.w[3].copy_(s.w[0]); s.v[3].copy_(s.v[0])
    w, v = s.w.cpu().numpy(), s.v.cpu().numpy()
    from springcraft_amd import _hip

    L = _hip.lib()
    m = dim * n_atoms
    for budget, subset in ((64 << 10, None), (1 << 20, np.arange(6, 106))):
        # (1 MiB: 100 listed rows take 1.4 MB per structure -> chunks of 72 and 28 rows; 64 KiB: chunks of 4 rows)
        s.consumer_budget_bytes = budget
        nsel = m if subset is None else len(subset)
        assert L.sc_dev_modes_workspace_bytes(m, m, 4, dim, nsel, 1, budget) < \
            L.sc_dev_modes_workspace_bytes(m, m, 4, dim, nsel, 1, 0)
        raw = s.dcc(mode_subset=subset, norm=False).cpu().numpy()
        nrm = s.dcc(mode_subset=subset).cpu().numpy()
        assert np.array_equal(raw[0], raw[3]) and np.array_equal(nrm[0], nrm[3])      # two different slabs
        for b in range(4):
            rows = pinv_rows(w[b]) if subset is None else subset
            ref = np_dcc(w[b], v[b], rows, dim)
            check_dcc(raw[b], ref, rows, dim, f"budget {budget} [{b}]")
            check_dcc_norm(nrm[b], ref, rows, dim, f"budget {budget} [{b}]")
    # a budget that holds two structures of a 100-row list at a time: slabs of 2 without chunks
    s.consumer_budget_bytes = 3 << 20
    raw = s.dcc(mode_subset=np.arange(6, 106), norm=False).cpu().numpy()
    assert np.array_equal(raw[0], raw[3])
    s.consumer_budget_bytes = None
    full = s.dcc(mode_subset=np.arange(6, 106), norm=False).cpu().numpy()
    for b in range(4):
        rows = np.arange(6, 106)
        check_dcc(full[b], np_dcc(w[b], v[b], rows, dim), rows, dim, f"default budget [{b}]")


# ---- the benchmarked shape ----------------------------------------------------------------------------------------------
def test_config3_shape_two_structures_full_spectrum(sc, torch):
    n_atoms, dim = 2000, 3
    coords = make_coords(n_atoms, 2, seed=70)
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(13.0))
    msf = s.mean_square_fluctuation().cpu().numpy()
    raw = s.dcc(norm=False).cpu().numpy()
    for b in range(2):
        rows = np.arange(6, dim * n_atoms)
        check_msf(msf[b], np_msf(w[b], v[b], rows, dim), rows, dim, f"N = 2000 [{b}]")
        drows = pinv_rows(w[b])
        check_dcc(raw[b], np_dcc(w[b], v[b], drows, dim), drows, dim, f"N = 2000 [{b}]")


# ---- nothing synchronises ---------------------------------------------------------------------------------------------------
def test_consumers_enqueued_straight_behind_solve_give_the_same_bits(sc, torch):
    n_atoms, batch = 301, 5
    coords = torch.from_numpy(make_coords(n_atoms, batch, seed=80)).cuda()
    ff = sc.InvariantForceField(13.0)
    a = DeviceBatchSolver(n_atoms, batch, ff)
    a.solve(coords)
    a.finish()
    torch.cuda.synchronize()
    ref = [a.mean_square_fluctuation(), a.dcc(), a.dcc(mode_subset=[9, 7, 9], norm=False), a.bfactor(), a.frequencies()]
    torch.cuda.synchronize()
    b = DeviceBatchSolver(n_atoms, batch, ff)
    b.mean_square_fluctuation(), b.dcc(), b.dcc(mode_subset=[9, 7, 9])   # (workspaces allocated: the calls below only enqueue)
    torch.cuda.synchronize()
    b.solve(coords)
    got = [b.mean_square_fluctuation(), b.dcc(), b.dcc(mode_subset=[9, 7, 9], norm=False), b.bfactor(), b.frequencies()]
    torch.cuda.synchronize()
    b.finish()
    for g, r in zip(got, ref):
        assert np.array_equal(g.cpu().numpy(), r.cpu().numpy())
