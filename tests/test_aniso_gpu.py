"""
GPU tests of the anisotropic fluctuation tensors (``k_baniso_partial`` / ``k_baniso_reduce`` of csrc/batch_consumers.hip)
through the three layers: ``nma.anisotropic_fluctuation`` (one model, ``sc_modes_aniso``), ``DeviceBatchSolver`` (
``sc_dev_modes_aniso_f64``) and ``RaggedBatchSolver`` (``sc_batch_plan_modes_aniso_f64``).

Ground truth is NumPy on eigenpairs,

    U[a, d, e] = sum_{k in S} v_k[3a + d] v_k[3a + e] / lambda_k
               = np.einsum('k,kad,kae->ade', 1 / w[S], V[S].reshape(-1, N, 3), V[S].reshape(-1, N, 3)),

under ``np.allclose`` with its defaults, the tolerance tests/test_batch_consumers_gpu.py uses for MSF / DCC against the
formulas' meaning.  Placement checks are bit for bit.  Shapes are the smallest that reach each branch: N = 20 (one partly
filled wavefront), 37, 171 (odd column counts), 257 (one atom past a 256-thread block).
"""
import numpy as np
import pytest

from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver
from tests.test_batch_consumers_gpu import K_B, N_A, make_coords, solved, window_case
from tests.util import ref_data, synthetic_coord

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def np_aniso(w, v, rows):
    """The formula on rows ``rows`` of (w (k,), v (k, 3N) rows = modes)."""
    rows = np.asarray(rows, dtype=np.int64)
    vs = v[rows].reshape(len(rows), -1, 3)
    return np.einsum("k,kad,kae->ade", 1.0 / w[rows], vs, vs)


def check(got, ref, what):
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = np.abs(ref).max() if ref.size else 0.0
    err = np.abs(got - ref).max() if ref.size else 0.0
    print(f"{what}: max abs err {err:.3e} (largest entry {scale:.3e})")
    assert np.array_equal(got, np.swapaxes(got, -1, -2)), what       # symmetric by construction, bit for bit
    assert np.allclose(got, ref), what


# ---- 1. one model: 1l2y against LAPACK on the oracle Hessian, the MSF and the covariance ---------------------------------
def test_1l2y_against_lapack_the_msf_and_the_covariance_blocks(sc):
    from oracle import enm_oracle as orc

    ca = sc.read_pdb_ca(ref_data("1l2y.pdb"))
    n = ca.array_length()
    assert n == 20
    ff = sc.InvariantForceField(13.0)
    anm = sc.ANM(ca, ff)
    h, _ = orc.compute_hessian(np.asarray(ca.coord, dtype=np.float64), orc.invariant_ff(13.0))
    w, vc = np.linalg.eigh(h)
    v = np.ascontiguousarray(vc.T)
    # (c) below relies on the covariance's rcond = 1e-6 dropping the six trivial modes and nothing else
    assert np.all(np.abs(w[:6]) <= 1e-6 * np.abs(w).max()) and np.all(w[6:] > 1e-6 * np.abs(w).max())
    for subset in (None, np.arange(6, 36)):
        rows = np.arange(6, 3 * n) if subset is None else subset
        u = anm.anisotropic_fluctuation(mode_subset=subset)
        assert u.shape == (n, 3, 3) and u.dtype == np.float64
        check(u, np_aniso(w, v, rows), f"1l2y {'all' if subset is None else 'arange(6, 36)'} (a) LAPACK")
        msf = anm.mean_square_fluctuation(mode_subset=subset)
        assert np.allclose(np.trace(u, axis1=1, axis2=2), msf)                                    # (b)
        assert np.array_equal(sc.nma.anisotropic_fluctuation(anm, subset), u)
    u = anm.anisotropic_fluctuation()
    scaled = anm.anisotropic_fluctuation(tem=300, tem_factors=K_B * N_A)
    assert np.allclose(scaled, u * (300 * K_B * N_A), rtol=1e-14, atol=0)
    ani = sc.nma.anisotropy(u)
    assert ani.shape == (n,) and np.all((ani > 0) & (ani <= 1))
    cov = sc.ANM(ca, ff).covariance                                                                # (c)
    blocks = np.stack([cov[3 * a: 3 * a + 3, 3 * a: 3 * a + 3] for a in range(n)])
    check(u, blocks, "1l2y all modes (c) diagonal blocks of the covariance")
    with pytest.raises(ValueError, match="Instance of ANM class expected"):
        sc.nma.anisotropic_fluctuation(sc.GNM(ca, ff))


# ---- 2. one model at the block edge ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms", [37, 257])
def test_single_model_on_its_own_eigenpairs(sc, n_atoms):
    anm = sc.ANM(synthetic_coord(n_atoms, 500 + n_atoms), sc.InvariantForceField(13.0))
    w, v = anm.eigen()
    m = 3 * n_atoms
    lists = {"default": None, "arange(6, 36)": np.arange(6, 36),
             "unsorted with a repeat": np.array([40, 7, m - 1, 40, 12, 6])}
    for name, subset in lists.items():
        rows = np.arange(6, m) if subset is None else subset
        u = anm.anisotropic_fluctuation(mode_subset=subset)
        check(u, np_aniso(w, v, rows), f"N = {n_atoms} {name}")
        assert np.allclose(np.trace(u, axis1=1, axis2=2), anm.mean_square_fluctuation(mode_subset=subset))
    assert not np.any(anm.anisotropic_fluctuation(mode_subset=[]))
    with pytest.raises(ValueError, match="Trivial modes"):
        anm.anisotropic_fluctuation(mode_subset=[5, 7])
    with pytest.raises(IndexError):
        anm.anisotropic_fluctuation(mode_subset=[7, m])


# ---- 3. DeviceBatchSolver --------------------------------------------------------------------------------------------------
N3, B3 = 171, 3


def test_batch_full_spectrum(sc, torch):
    coords = make_coords(N3, B3, seed=510)
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(13.0))
    m = 3 * N3
    for name, subset in (("default", None), ("unsorted with a repeat", np.array([40, 7, m - 1, 40, 12]))):
        rows = np.arange(6, m) if subset is None else subset
        u = s.anisotropic_fluctuation(mode_subset=subset)
        assert u.is_cuda and tuple(u.shape) == (B3, N3, 3, 3) and u.dtype == torch.float64
        msf = s.mean_square_fluctuation(mode_subset=subset).cpu().numpy()
        u = u.cpu().numpy()
        for b in range(B3):
            check(u[b], np_aniso(w[b], v[b], rows), f"batch [{b}] {name}")
            assert np.allclose(np.trace(u[b], axis1=1, axis2=2), msf[b])
    scaled = s.anisotropic_fluctuation(tem=300, tem_factors=K_B * N_A).cpu().numpy()
    assert np.allclose(scaled, s.anisotropic_fluctuation().cpu().numpy() * (300 * K_B * N_A), rtol=1e-14, atol=0)
    anm = sc.ANM(coords[1], sc.InvariantForceField(13.0))            # another eigensolver path: the same meaning
    assert np.allclose(s.anisotropic_fluctuation().cpu().numpy()[1], anm.anisotropic_fluctuation())


def test_batch_behind_an_index_range(sc, torch):
    lo, hi = 0, 25
    coords = make_coords(N3, B3, seed=520)
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(13.0), subset_by_index=(lo, hi))
    explicit = np.array([9, 7, 25, 9, 12])
    for subset, rows in ((None, np.arange(6, 26) - lo), (explicit, explicit - lo)):
        u = s.anisotropic_fluctuation(mode_subset=subset).cpu().numpy()
        msf = s.mean_square_fluctuation(mode_subset=subset).cpu().numpy()
        for b in range(B3):
            check(u[b], np_aniso(w[b], v[b], rows), f"subset_by_index [{b}] {None if subset is None else list(subset)}")
            assert np.allclose(np.trace(u[b], axis1=1, axis2=2), msf[b])
    with pytest.raises(ValueError, match=f"{lo}\\.\\.{hi}"):
        s.anisotropic_fluctuation(mode_subset=[7, 26])
    with pytest.raises(ValueError, match="Trivial modes"):
        s.anisotropic_fluctuation(mode_subset=[5, 7])


def test_batch_behind_a_value_window_reads_the_counts_on_the_device(sc, torch):
    """Counts that differ, one that fills max_modes, one below it and one empty window: chosen on the CPU from LAPACK."""
    K = 24
    coords, mats, lam, (vl, vu), expected = window_case(N3, K, 3, batch=B3)
    assert len(set(expected)) == 3 and expected.max() == K and expected.min() == 0 and np.sum(expected < K) == 2
    s = DeviceBatchSolver(N3, B3, sc.ParameterFreeForceField(), subset_by_value=(vl, vu), max_modes=K)
    s.matrix.copy_(torch.from_numpy(mats))
    s.eigh()
    u = s.anisotropic_fluctuation()                     # enqueued straight behind the solve
    msf = s.mean_square_fluctuation()
    s.finish()
    counts = s.counts.cpu().numpy()
    print("window counts", counts, "expected", expected)
    assert np.array_equal(counts, expected)
    w, v = s.w.cpu().numpy(), s.v.cpu().numpy()
    u, msf = u.cpu().numpy(), msf.cpu().numpy()
    for b in range(B3):
        if counts[b] == 0:
            assert not np.any(u[b])
            continue
        check(u[b], np_aniso(w[b], v[b], np.arange(counts[b])), f"window [{b}] count {counts[b]}")
        assert np.allclose(np.trace(u[b], axis1=1, axis2=2), msf[b])
    with pytest.raises(ValueError, match="subset_by_value"):
        s.anisotropic_fluctuation(mode_subset=[7, 8])


# ---- 4. placement, repetition, a failed structure --------------------------------------------------------------------------
def test_bits_do_not_depend_on_batch_size_position_or_neighbours(sc, torch):
    ff = sc.HinsenForceField()                          # no cutoff: a NaN coordinate reaches the matrix
    x = synthetic_coord(N3, 530)
    others = make_coords(N3, 2, seed=531)
    s1, _, _ = solved(sc, torch, x[None], ff)
    s3, _, _ = solved(sc, torch, np.stack([x, others[0], others[1]]), ff)
    # the consumer's own property: the same eigenpairs alone, first of three and last of three (the solver itself may pick
    # another GEMM tile for another batch size)
    s3.w[0].copy_(s1.w[0]); s3.v[0].copy_(s1.v[0])
    s3.w[2].copy_(s1.w[0]); s3.v[2].copy_(s1.v[0])
    for subset in (None, np.arange(6, 36), np.array([9, 7, 9])):
        u1 = s1.anisotropic_fluctuation(mode_subset=subset).cpu().numpy()
        u3 = s3.anisotropic_fluctuation(mode_subset=subset).cpu().numpy()
        assert np.array_equal(u1[0], u3[0]) and np.array_equal(u1[0], u3[2])
        assert np.array_equal(u3, s3.anisotropic_fluctuation(mode_subset=subset).cpu().numpy())
        assert np.array_equal(u1, s1.anisotropic_fluctuation(mode_subset=subset).cpu().numpy())
    # a NaN coordinate in the middle structure
    coords = make_coords(N3, 3, seed=540)
    good, _, _ = solved(sc, torch, coords, ff)
    ref = [good.anisotropic_fluctuation().cpu().numpy(), good.anisotropic_fluctuation(np.arange(6, 36)).cpu().numpy()]
    broken = coords.copy()
    broken[1, 7, 2] = np.nan
    bad = DeviceBatchSolver(N3, 3, ff)
    bad.solve(torch.from_numpy(broken).cuda())
    got = [bad.anisotropic_fluctuation(), bad.anisotropic_fluctuation(np.arange(6, 36))]
    with pytest.raises(np.linalg.LinAlgError):
        bad.finish()
    assert np.all(np.isnan(bad.w.cpu().numpy()[1]))
    for g, r in zip(got, ref):
        g = g.cpu().numpy()
        assert np.all(np.isnan(g[1]))
        assert np.array_equal(g[0], r[0]) and np.array_equal(g[2], r[2])
    assert np.all(np.isnan(sc.nma.anisotropy(got[0].cpu().numpy()[1])))


# ---- 5. RaggedBatchSolver ------------------------------------------------------------------------------------------------------
RAGGED = (20, 37, 171)


def _ragged(sc, torch, **kw):
    coords = [synthetic_coord(n, 550 + k) for k, n in enumerate(RAGGED)]
    s = RaggedBatchSolver(RAGGED, sc.InvariantForceField(13.0), **kw)
    s.solve(torch.from_numpy(np.concatenate(coords)).cuda().contiguous())
    s.finish()
    return s


def _own_plan_bits(sc, s, b, subset):
    """Structure b's eigenpairs in a plan of its own with the same slot order: its tensors from there."""
    kw = dict(order=s.order)
    if s.subset is not None:
        kw["subset_by_index"] = s.subset
    alone = RaggedBatchSolver((RAGGED[b],), sc.InvariantForceField(13.0), **kw)
    assert alone.order == s.order and alone.w.shape[1:] == s.w.shape[1:]
    alone.w[0].copy_(s.w[b]); alone.v[0].copy_(s.v[b])
    return alone.anisotropic_fluctuation(mode_subset=subset)[0].cpu().numpy()


@pytest.mark.parametrize("subset_by_index", [None, (0, 25)])
def test_ragged_views_sizes_and_placement(sc, torch, subset_by_index):
    kw = {} if subset_by_index is None else dict(subset_by_index=subset_by_index)
    s = _ragged(sc, torch, **kw)
    assert s.order == 3 * max(RAGGED)
    per = s.results()
    lists = [None, np.array([9, 7, 25, 9, 12])]
    for subset in lists:
        packed = s._aniso_packed(mode_subset=subset)
        assert packed.numel() == 6 * sum(RAGGED) and tuple(packed.shape) == (sum(RAGGED), 6)
        views = s.anisotropic_fluctuation(mode_subset=subset)
        msf = s.mean_square_fluctuation(mode_subset=subset)
        assert len(views) == len(RAGGED)
        for b, n in enumerate(RAGGED):
            w, v = (t.cpu().numpy() for t in per[b])
            assert v.shape[1] == 3 * n
            lo = 0 if subset_by_index is None else subset_by_index[0]
            rows = (np.arange(6, len(w) + lo) if subset is None else subset) - lo
            u = views[b].cpu().numpy()
            assert u.shape == (n, 3, 3)
            tag = f"ragged {subset_by_index} [{b}] N = {n} {None if subset is None else list(subset)}"
            check(u, np_aniso(w, v, rows), tag)
            assert np.allclose(np.trace(u, axis1=1, axis2=2), msf[b].cpu().numpy())
            # the six stored values sit at 6 x the structure's atom offset, in ANISOU order
            six = packed[int(s.offsets[b]): int(s.offsets[b + 1])].cpu().numpy()
            assert np.array_equal(six, np.stack([u[:, 0, 0], u[:, 1, 1], u[:, 2, 2], u[:, 0, 1], u[:, 0, 2], u[:, 1, 2]], axis=1))
            assert np.array_equal(u, _own_plan_bits(sc, s, b, subset)), tag
        again = s.anisotropic_fluctuation(mode_subset=subset)
        assert all(np.array_equal(a.cpu().numpy(), g.cpu().numpy()) for a, g in zip(again, views))


# ---- 6. GNM solvers ----------------------------------------------------------------------------------------------------------------
def test_dim_1_solvers_raise_on_the_host(sc, torch):
    ff = sc.InvariantForceField(10.0)
    for s in (DeviceBatchSolver(30, 2, ff, dim=1), RaggedBatchSolver((20, 30), ff, dim=1)):
        # nothing was solved and nothing may be enqueued: a call that reached the device would read uninitialised modes
        with pytest.raises(ValueError, match="dim=3"):
            s.anisotropic_fluctuation()
        with pytest.raises(ValueError, match="dim=3"):
            s.anisotropic_fluctuation(mode_subset=[3, 4])
    from springcraft_amd import _hip

    gnm = sc.GNM(synthetic_coord(30, 560), ff)
    with pytest.raises(ValueError, match="ANM"):
        gnm._modes_device().aniso(np.arange(1, 10))        # the C entry's own argument error for a dim-1 object
    assert _hip.lib().sc_dev_modes_workspace_bytes(90, 90, 2, 3, 84, 2, 0) > 0
