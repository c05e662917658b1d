"""
GPU tests of the linear response and the mode synthesis (``k_modes_project``, ``k_modes_combine_partial`` /
``_reduce`` of csrc/mode_response.hip) through the three layers: ``nma.linear_response`` / ``nma.mode_displacement`` (one
model, ``sc_modes_response`` / ``sc_modes_combine``), ``DeviceBatchSolver`` (``sc_dev_mode_*``) and ``RaggedBatchSolver``
(``sc_batch_plan_mode_*``).

Networks: ``np.random.seed(s); rand(N, 3) * 5 * N**(1/3)`` under ``InvariantForceField(13.0)``.  For N in {21, 64, 131,
200} and seeds 0 and 1 NumPy gives lambda_6 / lambda_max >= 0.012 and trivial |lambda| / lambda_max <= 3e-15: the 1e-6 pinv
threshold is far from any eigenvalue and the retained condition number is below 100.  Every numeric test asserts that on
its NumPy spectrum first (``spectrum``), so a changed input fails loudly instead of flaking.

Reference: ``np.linalg.pinv(H, hermitian=True, rcond=1e-6) @ f`` with H the package's own Hessian (``c @ V_sel`` for the
combine tests).  Tolerance: ``atol = 1e-10 * max|ref|, rtol = 0``.  The bound n eps kappa is about 600 * 2.2e-16 * 100 ~
1.3e-11 and NumPy's own mode-space formula agrees with ``pinv @ f`` to 2e-15 here: about a factor 10 over the bound.
Sums over a band of modes (6..25) are compared with NumPy's sum over the same band; the band's subspace is determined to
about eps lambda_max / gap, and the tests assert gap >= 1e-4 lambda_max at the band's edge (1e-12, far inside the gate).
Behind a value window and for the combine pass the reference is formed from the solver's own rows of v: what is under
test there is the consumer, which rows it takes and which it never reads.  Placement checks are bit for bit.

Shapes: N = 21 (lanes without atoms), 131 (odd: m = 393, 8-byte loads, a second trip of the atom loop), 200 (m = 600: two
column tiles, 16-byte loads, 594 selected rows in several chunks), q = 5 (crosses the group of four).
"""
import numpy as np
import pytest

from springcraft_amd.batch import DeviceBatchSolver, RaggedBatchSolver
from tests.test_batch_consumers_gpu import solved, window_case

pytestmark = pytest.mark.gpu

CUTOFF = 13.0


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def network(n_atoms, seed):
    np.random.seed(seed)
    return np.random.rand(n_atoms, 3) * 5 * n_atoms ** (1 / 3)


def spectrum(h, band_end=None):
    """NumPy eigenpairs (rows = modes) of the Hessian ``h``, with the preconditions of the module docstring asserted."""
    lam, vec = np.linalg.eigh(h)
    top = np.abs(lam).max()
    # (3e-15 measured; 1e-13 leaves room for another LAPACK and is still seven orders under the pinv threshold)
    assert np.abs(lam[:6]).max() <= 1e-13 * top, "trivial eigenvalues are not at rounding level"
    assert lam[6] >= 0.012 * top, f"lambda_6 / lambda_max = {lam[6] / top:.3e}: the network is nearly disconnected"
    if band_end is not None:
        assert lam[band_end + 1] - lam[band_end] >= 1e-4 * top, "the band's upper edge is nearly degenerate"
    return lam, vec.T


_CACHE = {}


def case(sc, n_atoms, seed):
    """(coord, Hessian of the package, pinv by NumPy, NumPy eigenvalues, eigenvectors as rows): computed once per shape."""
    key = (n_atoms, seed)
    if key not in _CACHE:
        coord = network(n_atoms, seed)
        h, _ = sc.compute_hessian(coord, sc.InvariantForceField(CUTOFF))
        lam, vec = spectrum(h, band_end=25)
        cov = np.linalg.pinv(h, hermitian=True, rcond=1e-6)
        for a in (coord, h, cov, lam, vec):
            a.setflags(write=False)
        _CACHE[key] = (coord, h, cov, lam, vec)
    return _CACHE[key]


def band_response(lam, vec, f, lo=6, hi=25):
    """sum over modes lo..hi of v <v, f> / lambda; f (q, 3N)."""
    vs = vec[lo: hi + 1]
    return ((f @ vs.T) / lam[lo: hi + 1]) @ vs


def check(got, ref, what):
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max() if ref.size else 0.0
    print(f"{what}: max abs err {err:.3e} = {err / scale if scale else 0.0:.3e} max|ref|")
    assert np.all(np.isfinite(got)), what
    assert np.allclose(got, ref, rtol=0, atol=1e-10 * scale), what


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


# ---- 1. one model: nma.linear_response --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms", [21, 131, 200])
def test_one_model_linear_response(sc, n_atoms):
    coord, h, cov, lam, vec = case(sc, n_atoms, 0)
    anm = sc.ANM(coord, sc.InvariantForceField(CUTOFF))
    rs = np.random.RandomState(n_atoms)
    f5 = rs.randn(5, n_atoms, 3)
    ref5 = (f5.reshape(5, -1) @ cov).reshape(5, n_atoms, 3)
    got5 = sc.nma.linear_response(anm, f5)
    check(got5, ref5, f"N = {n_atoms} (5, N, 3)")
    one = sc.nma.linear_response(anm, f5[4])
    check(one, ref5[4], f"N = {n_atoms} (N, 3)")
    flat = anm.linear_response(f5[4].ravel())
    assert flat.shape == (n_atoms, 3) and np.array_equal(flat, one)
    assert np.array_equal(one, got5[4])                      # alone or as the fifth of five: the same bits
    assert anm._covariance is None                           # no (3N, 3N) matrix was formed on the way
    # an explicit band of modes against NumPy's sum over the same band
    band = np.arange(6, 26)
    ref_band = band_response(lam, vec, f5.reshape(5, -1)).reshape(5, n_atoms, 3)
    check(anm.linear_response(f5, mode_subset=band), ref_band, f"N = {n_atoms} modes 6..25")
    check(sc.nma.linear_response(anm, f5[0], band), ref_band[0], f"N = {n_atoms} modes 6..25, one force")
    assert np.array_equal(anm.linear_response(f5, mode_subset=[]), np.zeros((5, n_atoms, 3)))
    with pytest.raises(IndexError):
        anm.linear_response(f5, mode_subset=[7, 3 * n_atoms])
    # a covariance assigned by the caller is applied as it is
    mine = sc.ANM(coord, sc.InvariantForceField(CUTOFF))
    a = rs.randn(3 * n_atoms, 3 * n_atoms)
    mine.covariance = a
    assert np.array_equal(mine.linear_response(f5[1]), (a @ f5[1].ravel()).reshape(-1, 3))
    assert np.allclose(mine.linear_response(f5), (f5.reshape(5, -1) @ a.T).reshape(5, -1, 3), rtol=1e-13, atol=0)


# ---- 2. one model: mode_displacement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n_atoms", [("anm", 131), ("gnm", 131), ("anm", 200), ("gnm", 21)])
def test_one_model_mode_displacement(sc, kind, n_atoms):
    coord = network(n_atoms, 1)
    dim, ntriv = (3, 6) if kind == "anm" else (1, 1)
    enm = sc.ANM(coord, sc.InvariantForceField(CUTOFF)) if kind == "anm" else sc.GNM(coord, sc.InvariantForceField(10.0))
    _, v = enm.eigen()
    m = dim * n_atoms
    tail = (n_atoms, 3) if kind == "anm" else (n_atoms,)
    rs = np.random.RandomState(n_atoms + dim)
    lists = {"default": None, "band": np.arange(ntriv, ntriv + 20), "unsorted with a repeat": np.array([m - 1, 7, 12, 7, ntriv])}
    for name, subset in lists.items():
        rows = np.arange(ntriv, m) if subset is None else subset
        c = rs.randn(5, len(rows))
        got = enm.mode_displacement(c, mode_subset=subset)
        check(got, (c @ v[rows]).reshape((5,) + tail), f"{kind} N = {n_atoms} {name}")
        one = sc.nma.mode_displacement(enm, c[4], subset)
        assert one.shape == tail and np.array_equal(one, got[4])
    assert np.array_equal(enm.mode_displacement(np.zeros((2, 0)), mode_subset=[]), np.zeros((2,) + tail))
    # the inverse of overlap: a displacement orthogonal to the trivial modes comes back from its projections
    d = rs.randn(2, m)
    d -= (d @ v[:ntriv].T) @ v[:ntriv]
    d = d.reshape((2,) + tail)
    ov = enm.overlap(d)
    back = enm.mode_displacement(np.linalg.norm(d.reshape(2, -1), axis=1)[:, None] * ov)
    check(back, d, f"{kind} N = {n_atoms} overlap -> mode_displacement")
    samples = sc.nma.sample_displacements(enm, 3, mode_subset=np.arange(ntriv, ntriv + 10), rng=5)
    assert samples.shape == (3,) + tail and np.all(np.isfinite(samples))


# ---- 3. DeviceBatchSolver, full spectrum -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms,batch", [(64, 3), (131, 2)])
def test_batch_full_spectrum(sc, torch, n_atoms, batch):
    cases = [case(sc, n_atoms, seed) for seed in range(batch)]    # (seed 2 at N = 64: lambda_6 / lambda_max = 0.028)
    coords = np.stack([c[0] for c in cases])
    ff = sc.InvariantForceField(CUTOFF)
    s, w, v = solved(sc, torch, coords, ff)
    m = 3 * n_atoms
    rs = np.random.RandomState(700 + n_atoms)
    for q in (1, 5):
        f = rs.randn(batch, q, n_atoms, 3)
        x = s.linear_response(dev(torch, f))
        assert x.is_cuda and tuple(x.shape) == (batch, q, n_atoms, 3) and x.dtype == torch.float64
        single = s.linear_response(dev(torch, f[:, q - 1]))
        assert tuple(single.shape) == (batch, n_atoms, 3) and torch.equal(single, x[:, q - 1])
        x = x.cpu().numpy()
        for b in range(batch):
            ref = (f[b].reshape(q, m) @ cases[b][2]).reshape(q, n_atoms, 3)
            check(x[b], ref, f"batch {batch} x {n_atoms} [{b}] q = {q} response")
    c = rs.randn(batch, 5, m)
    d = s.mode_displacement(dev(torch, c))
    assert d.is_cuda and tuple(d.shape) == (batch, 5, n_atoms, 3)
    one = s.mode_displacement(dev(torch, c[:, 4]))
    assert tuple(one.shape) == (batch, n_atoms, 3) and torch.equal(one, d[:, 4])
    d = d.cpu().numpy()
    for b in range(batch):
        check(d[b], (c[b] @ v[b]).reshape(5, n_atoms, 3), f"batch {batch} x {n_atoms} [{b}] mode_displacement")
    # overlap -> mode_displacement over all rows gives the displacement back, on the device
    disp = rs.randn(batch, 2, n_atoms, 3)
    ov = s.overlap(dev(torch, disp))
    norms = dev(torch, np.linalg.norm(disp.reshape(batch, 2, -1), axis=-1))
    back = s.mode_displacement((ov * norms[:, :, None]).contiguous()).cpu().numpy()
    for b in range(batch):
        check(back[b], disp[b], f"batch [{b}] overlap -> mode_displacement")


def test_batch_with_masses_gives_the_cartesian_response(sc, torch):
    n_atoms, batch = 64, 3
    cases = [case(sc, n_atoms, seed) for seed in range(batch)]
    coords = np.stack([c[0] for c in cases])
    masses = np.random.RandomState(3).uniform(10.0, 20.0, (batch, n_atoms))
    s, w, v = solved(sc, torch, coords, sc.InvariantForceField(CUTOFF), masses=masses)
    f = np.random.RandomState(4).randn(batch, 5, n_atoms, 3)
    x = s.linear_response(dev(torch, f), atom_scale=s.inv_sqrt_mass).cpu().numpy()
    raw = s.linear_response(dev(torch, f)).cpu().numpy()
    c = np.random.RandomState(5).randn(batch, 2, 3 * n_atoms)
    cart = s.mode_displacement(dev(torch, c), atom_scale=s.inv_sqrt_mass).cpu().numpy()
    for b in range(batch):
        ism = np.repeat(1 / np.sqrt(masses[b]), 3)
        h_mw = cases[b][1] * ism[:, None] * ism[None, :]
        lam = np.linalg.eigvalsh(h_mw)
        # (the mass ratio of 2 may double the condition number: 192 eps 200 ~ 8e-12 stays under the gate)
        assert lam[6] >= 0.005 * lam[-1] and np.abs(lam[:6]).max() <= 1e-13 * lam[-1]
        cov = np.linalg.pinv(h_mw, hermitian=True, rcond=1e-6)
        fb = f[b].reshape(5, -1)
        check(x[b], (((fb * ism) @ cov) * ism).reshape(5, n_atoms, 3), f"masses [{b}] M^-1/2 pinv(H_mw) M^-1/2 f")
        check(raw[b], (fb @ cov).reshape(5, n_atoms, 3), f"masses [{b}] pinv(H_mw) f")
        check(cart[b], ((c[b] @ v[b]) * ism).reshape(2, n_atoms, 3), f"masses [{b}] scaled mode_displacement")


# ---- 4. behind an index range ---------------------------------------------------------------------------------------------------
def test_batch_behind_an_index_range(sc, torch):
    n_atoms, batch = 64, 3
    cases = [case(sc, n_atoms, seed) for seed in range(batch)]
    s = DeviceBatchSolver(n_atoms, batch, sc.InvariantForceField(CUTOFF), subset_by_index=(0, 25))
    s.solve(dev(torch, np.stack([c[0] for c in cases])))
    f = np.random.RandomState(710).randn(batch, 5, n_atoms, 3)
    x = s.linear_response(dev(torch, f))                 # enqueued straight behind the solve
    sub = s.linear_response(dev(torch, f), mode_subset=[7, 20, 7])
    s.finish()
    x, sub = x.cpu().numpy(), sub.cpu().numpy()
    assert x.shape == (batch, 5, n_atoms, 3)
    for b in range(batch):
        _, _, _, lam, vec = cases[b]
        fb = f[b].reshape(5, -1)
        check(x[b], band_response(lam, vec, fb).reshape(5, n_atoms, 3), f"subset_by_index [{b}] modes 6..25")
        assert lam[8] - lam[7] >= 1e-4 * lam[-1] and lam[7] - lam[6] >= 1e-4 * lam[-1]
        assert lam[21] - lam[20] >= 1e-4 * lam[-1] and lam[20] - lam[19] >= 1e-4 * lam[-1]
        ref = 2 * band_response(lam, vec, fb, 7, 7) + band_response(lam, vec, fb, 20, 20)
        check(sub[b], ref.reshape(5, n_atoms, 3), f"subset_by_index [{b}] modes [7, 20, 7]")
    with pytest.raises(ValueError, match="was not solved"):
        s.linear_response(dev(torch, f), mode_subset=[26])


# ---- 5. behind a value window -----------------------------------------------------------------------------------------------------
def test_batch_behind_a_value_window(sc, torch):
    """Counts that differ, one that fills max_modes, one below it and one empty window (tests/test_batch_consumers_gpu.py)."""
    n_atoms, batch, K = 171, 3, 24
    coords, mats, lam, (vl, vu), expected = window_case(n_atoms, K, 3, batch=batch)
    assert expected.max() == K and expected.min() == 0
    s = DeviceBatchSolver(n_atoms, batch, sc.ParameterFreeForceField(), subset_by_value=(vl, vu), max_modes=K)
    s.matrix.copy_(torch.from_numpy(mats))
    s.eigh()
    rs = np.random.RandomState(720)
    f = rs.randn(batch, 5, n_atoms, 3)
    c = rs.randn(batch, 5, K)
    x = s.linear_response(dev(torch, f))                 # enqueued straight behind the solve
    d_clean = s.mode_displacement(dev(torch, c))
    s.finish()
    counts = s.counts.cpu().numpy()
    assert np.array_equal(counts, expected)
    poisoned = c.copy()
    for b in range(batch):
        poisoned[b, :, counts[b]:] = np.nan                # coefficients behind the count are never read
    d = s.mode_displacement(dev(torch, poisoned)).cpu().numpy()
    assert np.array_equal(d, d_clean.cpu().numpy())
    w, v = s.w.cpu().numpy(), s.v.cpu().numpy()
    x = x.cpu().numpy()
    for b in range(batch):
        k = counts[b]
        if k == 0:
            assert np.array_equal(x[b], np.zeros_like(x[b])) and np.array_equal(d[b], np.zeros_like(d[b]))
            continue
        fb = f[b].reshape(5, -1)
        check(x[b], (((fb @ v[b, :k].T) / w[b, :k]) @ v[b, :k]).reshape(5, n_atoms, 3), f"window [{b}] count {k} response")
        check(d[b], (c[b][:, :k] @ v[b, :k]).reshape(5, n_atoms, 3), f"window [{b}] count {k} mode_displacement")
    with pytest.raises(ValueError, match="subset_by_value"):
        s.linear_response(dev(torch, f), mode_subset=[7])


# ---- 6. bits --------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_batch_size_position_neighbours_or_q(sc, torch):
    n_atoms = 131
    ff = sc.InvariantForceField(CUTOFF)
    x0 = network(n_atoms, 0)
    others = np.stack([network(n_atoms, 1), network(n_atoms, 2)])
    s1, _, _ = solved(sc, torch, x0[None], ff)
    s3, _, _ = solved(sc, torch, np.stack([x0, others[0], others[1]]), ff)
    # the consumer's own property: the same eigenpairs alone, first of three and last of three
    for b in (0, 2):
        s3.w[b].copy_(s1.w[0])
        s3.v[b].copy_(s1.v[0])
    rs = np.random.RandomState(730)
    m = 3 * n_atoms
    f1, f3 = rs.randn(1, 6, n_atoms, 3), rs.randn(3, 6, n_atoms, 3)
    c1, c3 = rs.randn(1, 6, m), rs.randn(3, 6, m)
    for a1, a3 in ((f1, f3), (c1, c3)):
        a3[0] = a1[0]
        a3[2] = a1[0]
    r1, r3 = s1.linear_response(dev(torch, f1)).cpu().numpy(), s3.linear_response(dev(torch, f3)).cpu().numpy()
    d1, d3 = s1.mode_displacement(dev(torch, c1)).cpu().numpy(), s3.mode_displacement(dev(torch, c3)).cpu().numpy()
    assert np.all(np.isfinite(r3)) and np.all(np.isfinite(d3)) and np.abs(r1).max() > 0 and np.abs(d1).max() > 0
    assert np.array_equal(r1[0], r3[0]) and np.array_equal(r1[0], r3[2])
    assert np.array_equal(d1[0], d3[0]) and np.array_equal(d1[0], d3[2])
    # vector j alone against vector j as member of q = 6: first group, and second group of four
    for j in (2, 5):
        assert np.array_equal(s1.linear_response(dev(torch, f1[:, j])).cpu().numpy(), r1[:, j])
        assert np.array_equal(s3.linear_response(dev(torch, f3[:, j: j + 1])).cpu().numpy()[:, 0], r3[:, j])
        assert np.array_equal(s1.mode_displacement(dev(torch, c1[:, j])).cpu().numpy(), d1[:, j])
        assert np.array_equal(s3.mode_displacement(dev(torch, c3[:, j: j + 1])).cpu().numpy()[:, 0], d3[:, j])
    # a repeated call
    assert np.array_equal(s3.linear_response(dev(torch, f3)).cpu().numpy(), r3)
    assert np.array_equal(s3.mode_displacement(dev(torch, c3)).cpu().numpy(), d3)
    # a weight-zero row is selected out, not multiplied by zero: NaN in rows the selection leaves out changes nothing
    s3.v[1, 0:6] = float("nan")                            # the trivial rows: under the pinv threshold
    assert np.array_equal(s3.linear_response(dev(torch, f3)).cpu().numpy(), r3)
    band = s3.linear_response(dev(torch, f3), mode_subset=np.arange(6, 26)).cpu().numpy()
    s3.v[1, 30] = float("nan")                             # not in the list
    assert np.array_equal(s3.linear_response(dev(torch, f3), mode_subset=np.arange(6, 26)).cpu().numpy(), band)
    assert np.all(np.isfinite(band))


# ---- 7. RaggedBatchSolver -----------------------------------------------------------------------------------------------------------
RAGGED = (21, 64, 40)


@pytest.mark.parametrize("subset_by_index", [None, (0, 25)])
def test_ragged_views_placement_and_pads(sc, torch, subset_by_index):
    kw = {} if subset_by_index is None else dict(subset_by_index=subset_by_index)
    ff = sc.InvariantForceField(CUTOFF)
    coords = [network(n, 0) for n in RAGGED]
    for n, x in zip(RAGGED, coords):
        h, _ = sc.compute_hessian(x, ff)
        spectrum(h)
    s = RaggedBatchSolver(RAGGED, ff, **kw)
    s.solve(dev(torch, np.concatenate(coords)))
    s.finish()
    total = sum(RAGGED)
    off = np.concatenate([[0], np.cumsum(RAGGED)])
    rs = np.random.RandomState(740)
    f = rs.randn(5, total, 3)
    nvec = s.w.shape[1]
    c = rs.randn(len(RAGGED), 5, nvec)
    limits = [3 * n if subset_by_index is None else nvec for n in RAGGED]
    for b, lim in enumerate(limits):
        c[b, :, lim:] = np.nan                             # the pad tail of the coefficients is never read
    x5, x1 = s.linear_response(dev(torch, f)), s.linear_response(dev(torch, f[3]))
    d5, d1 = s.mode_displacement(dev(torch, c)), s.mode_displacement(dev(torch, c[:, 3]))
    assert len(x5) == len(x1) == len(d5) == len(d1) == len(RAGGED)
    for views, q in ((x5, 5), (d5, 5), (x1, None), (d1, None)):
        base = views[0].untyped_storage().data_ptr()
        for b, n in enumerate(RAGGED):
            assert tuple(views[b].shape) == ((n, 3) if q is None else (q, n, 3))
            assert views[b].untyped_storage().data_ptr() == base               # views into ONE packed buffer
            assert views[b].storage_offset() == 3 * off[b]
    for b, n in enumerate(RAGGED):
        alone, _, v = solved(sc, torch, coords[b][None], ff, **kw)
        fb = np.ascontiguousarray(f[:, off[b]: off[b + 1]])
        ref = alone.linear_response(dev(torch, fb[None]))[0].cpu().numpy()
        tag = f"ragged {subset_by_index} [{b}] N = {n}"
        check(x5[b].cpu().numpy(), ref, tag + " response against the structure alone")
        assert np.array_equal(x1[b].cpu().numpy(), x5[b][3].cpu().numpy())
        lim = limits[b]
        own = s.results()[b][1].cpu().numpy()                                   # (rows_b, 3 n): the slot's own rows and columns
        assert own.shape == (lim, 3 * n)
        check(d5[b].cpu().numpy(), (c[b][:, :lim] @ own).reshape(5, n, 3), tag + " mode_displacement")
        assert np.array_equal(d1[b].cpu().numpy(), d5[b][3].cpu().numpy())
        if subset_by_index is None:
            cov = np.linalg.pinv(sc.compute_hessian(coords[b], ff)[0], hermitian=True, rcond=1e-6)
            check(x5[b].cpu().numpy(), (fb.reshape(5, -1) @ cov).reshape(5, n, 3), tag + " response against pinv(H) f")


# ---- 8. a structure that cannot be solved ---------------------------------------------------------------------------------------------
def test_a_non_finite_matrix_gives_nan_and_leaves_the_neighbours_alone(sc, torch):
    n_atoms, batch = 64, 3
    cases = [case(sc, n_atoms, seed) for seed in range(batch)]
    mats = np.stack([c[1] for c in cases])
    ff = sc.InvariantForceField(CUTOFF)
    rs = np.random.RandomState(750)
    f, c = rs.randn(batch, 2, n_atoms, 3), rs.randn(batch, 2, 3 * n_atoms)

    def run(matrices):
        s = DeviceBatchSolver(n_atoms, batch, ff)
        s.matrix.copy_(torch.from_numpy(matrices))
        s.eigh()
        return s, s.linear_response(dev(torch, f)), s.mode_displacement(dev(torch, c))

    good, ref_x, ref_d = run(mats)
    good.finish()
    broken = mats.copy()
    broken[1, 5, 9] = broken[1, 9, 5] = np.nan
    bad, x, d = run(broken)
    with pytest.raises(np.linalg.LinAlgError):
        bad.finish()
    x, d, ref_x, ref_d = (t.cpu().numpy() for t in (x, d, ref_x, ref_d))
    assert np.all(np.isnan(x[1])) and np.all(np.isnan(d[1]))
    for b in (0, 2):
        assert np.array_equal(x[b], ref_x[b]) and np.array_equal(d[b], ref_d[b])
        assert np.all(np.isfinite(x[b])) and np.all(np.isfinite(d[b]))
