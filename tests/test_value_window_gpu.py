"""
The eigenvalue window (``subset_by_value=(vl, vu)``, scipy's half-open interval (vl, vu]) on the device.

The window is counted on the tridiagonal matrix that is then solved (k_window_count in stein.hip: Sturm counts at the
bounds, scaled by the matrix' power-of-two factor); a single matrix then runs the index path for exactly the m pairs it
found, a batch (sc_dev_eigh_window_f64, DeviceBatchSolver) fills slots of K pairs from a start index per member and moves
the window's rows to the front of every slot (k_window_compact).

Window bounds sit at the midpoints of gaps >= 1e-6 ||A|| of the reference spectrum, never near an eigenvalue (where the
device's count decides membership to about n eps ||A||, as in LAPACK's dsyevr).  Gates as tests/test_partial_spectrum_gpu.py:
eigenvalues within 1e-11 max|lambda| of the reference, residual <= 1e-10 lambda_max, ||V V^T - I||_max <= 1e-10, and the
Davis-Kahan subspace check of tests/util.py:subspace_error.  The figures are printed (``pytest -s``).
"""
import ctypes as C

import numpy as np
import pytest

from tests.util import (LATTICE_CUTOFF, anm_exact, clustered_spectrum, device_checks, gnm_exact, lattice,
                        random_orthogonal, subspace_error, synthetic_coord)

pytestmark = pytest.mark.gpu

TOL_W, TOL_RES, TOL_ORTH = 1e-11, 1e-10, 1e-10
MIN_GAP = 1e-6


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture
def two_stage_path():
    """Sets the tridiagonalisation path of the process-wide context and restores the automatic rule afterwards."""
    from springcraft_amd import _hip

    ctx = _hip.context()
    yield ctx.set_two_stage
    ctx.set_two_stage(None)


def _sym(seed, n, scale=1.0):
    a = np.random.RandomState(seed).randn(n, n)
    return (a + a.T) * scale


def _bound_below(w, i, scale):
    """A bound in the first gap >= MIN_GAP scale at or above position i (between w[j - 1] and w[j]); returns (bound, j)."""
    if i <= 0:
        return -np.inf, 0
    j = i
    while j < len(w) and w[j] - w[j - 1] < MIN_GAP * scale:
        j += 1
    if j == len(w):
        return np.inf, j
    return 0.5 * (w[j - 1] + w[j]), j


def _window(w, i0, i1, scale=None):
    """(vl, vu, il, m): bounds in gaps near positions i0 (first inside) and i1 (first outside) of the ascending w."""
    scale = np.abs(w).max() if scale is None else scale
    vl, il = _bound_below(w, i0, scale)
    vu, iu = _bound_below(w, i1, scale)
    return vl, vu, il, iu - il


def _gate(label, a, w, v, ref, il, m, scale=None):
    """All gates on the window's eigenpairs (w, v), the reference eigenpairs il .. il + m - 1 of `a` (LAPACK: ref)."""
    w = np.asarray(w)
    w_ref, v_ref = ref
    n = len(w_ref)
    scale = np.abs(w_ref).max() if scale is None else scale
    assert w.shape == (m,), (label, w.shape, m)
    if v is not None:
        assert np.asarray(v).shape == (m, n), (label, np.asarray(v).shape)
    out = {"m": m}
    if m == 0:
        print(f"{label}: empty")
        return out
    out["eig"] = float(np.abs(w - w_ref[il:il + m]).max() / scale)
    assert out["eig"] <= TOL_W, (label, out)
    assert np.all(np.diff(w) >= 0), f"{label}: eigenvalues not ascending"
    if v is not None:
        v = np.asarray(v)
        r = a @ v.T - v.T * w[None, :]
        out["res"] = float(np.linalg.norm(r, axis=0).max() / scale)
        out["orth"] = float(np.abs(v @ v.T - np.eye(m)).max())
        sub, bound, _ = subspace_error(a, w_ref, v_ref, il, il + m - 1, v, np.linalg.norm(r))
        out["sub"], out["sub_bound"] = float(sub), float(bound)
        assert out["res"] <= TOL_RES and out["orth"] <= TOL_ORTH, (label, out)
        assert out["sub"] <= out["sub_bound"], (label, out)
    print(f"{label}: " + ", ".join(f"{k} {x:.1e}" if isinstance(x, float) else f"{k} {x}" for k, x in out.items()))
    return out


# ---- random symmetric matrices against scipy -------------------------------------------------------------------------

@pytest.mark.parametrize("two_stage", [False, True], ids=["one_stage", "two_stage"])
@pytest.mark.parametrize("n", [300, 1000, 1500])
def test_random_against_scipy(sc, two_stage_path, n, two_stage):
    import scipy.linalg

    two_stage_path(two_stage)
    a = _sym(500 + n, n)
    ref = np.linalg.eigh(a)
    for i0, i1 in [(n // 5, n // 5 + n // 7), (0, 40), (n - 33, n)]:
        vl, vu, il, m = _window(ref[0], i0, i1)
        if i0 == 0:
            vl = -np.inf if n == 300 else ref[0][0] - 1.0          # both kinds of "below everything"
        if i1 == n:
            vu = np.inf if n != 1000 else ref[0][-1] + 1.0
        w_sp = scipy.linalg.eigh(a, eigvals_only=True, subset_by_value=(vl, vu))
        assert len(w_sp) == m, (n, vl, vu, len(w_sp), m)
        w, v = sc.nma.eigh(a, subset_by_value=(vl, vu))
        _gate(f"n={n} {two_stage} ({vl:.3g}, {vu:.3g}]", a, w, v, ref, il, m)
        assert np.abs(w - w_sp).max() <= TOL_W * np.abs(ref[0]).max()
        w2 = sc.nma.eigh(a, eigenvectors=False, subset_by_value=(vl, vu))
        assert w2.shape == (m,) and np.abs(w2 - w).max() <= 1e-12 * np.abs(ref[0]).max()


@pytest.mark.parametrize("vectors", [True, False])
def test_empty_single_and_everything(sc, vectors):
    n = 400
    a = _sym(17, n)
    ref = np.linalg.eigh(a)
    w_ref = ref[0]
    gaps = np.diff(w_ref)
    k = int(np.argmax(gaps[100:300])) + 100          # a wide gap: between w_ref[k] and w_ref[k + 1]
    cases = {
        "empty": (w_ref[k] + 0.25 * gaps[k], w_ref[k] + 0.75 * gaps[k], k + 1, 0),
        "single": (0.5 * (w_ref[k - 1] + w_ref[k]), w_ref[k] + 0.5 * gaps[k], k, 1),
        "everything": (-np.inf, np.inf, 0, n),
        "above all": (w_ref[-1] + 1.0, np.inf, n, 0),
        "below all": (-np.inf, w_ref[0] - 1.0, 0, 0),
    }
    for label, (vl, vu, il, m) in cases.items():
        out = sc.nma.eigh(a, eigenvectors=vectors, subset_by_value=(vl, vu))
        w, v = out if vectors else (out, None)
        assert w.shape == (m,) and w.dtype == np.float64, (label, w.shape)
        if vectors:
            assert v.shape == (m, n), (label, v.shape)
        _gate(f"{label} vectors={vectors}", a, w, v, ref, il, m)
    w_all, v_all = sc.nma.eigh(a)
    out = sc.nma.eigh(a, eigenvectors=vectors, subset_by_value=(-np.inf, np.inf))
    w, v = out if vectors else (out, None)
    assert np.abs(w - w_all).max() <= 1e-12 * np.abs(w_ref).max()


# ---- degenerate clusters -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rel_spacing", [0.0, 1e-13])
def test_clusters_inside_the_window(sc, rel_spacing):
    """Q diag(w) Q^T with clusters of 5, 12, 8, 20 (near-)equal eigenvalues wholly inside windows."""
    n = 500
    w0 = clustered_spectrum(rel_spacing, n=n, seed=3)
    q = random_orthogonal(11, n)
    a = (q * w0[None, :]) @ q.T
    a = 0.5 * (a + a.T)
    ref = np.linalg.eigh(a)
    centres = np.linspace(-3.0, 5.0, 10) + 0.01
    for c0, c1 in [(1, 2), (6, 7), (1, 7)]:      # clusters c0 .. c1 - 1 (of sizes 5 / 20 / everything between)
        vl, vu = centres[c0] - 0.02, centres[c1 - 1] + 0.02 + 1e-9
        exact = int(np.count_nonzero((w0 > vl) & (w0 <= vu)))
        assert np.all(np.abs(w0 - vl) > 1e-3) and np.all(np.abs(w0 - vu) > 1e-3)
        il = int(np.count_nonzero(w0 <= vl))
        w, v = sc.nma.eigh(a, subset_by_value=(vl, vu))
        assert len(w) == exact, (c0, c1, len(w), exact)
        _gate(f"clusters {c0}..{c1 - 1} spacing {rel_spacing:g}", a, w, v, ref, il, exact)


@pytest.mark.parametrize("dim", [1, 3], ids=["gnm", "anm"])
def test_lattice_closed_form_counts(sc, dim):
    """Lattice networks: exact spectra with high multiplicities; windows between distinct exact values."""
    a_, b_, c_ = (7, 8, 9) if dim == 1 else (5, 6, 7)
    coord = lattice(a_, b_, c_, 5)
    ff = sc.InvariantForceField(LATTICE_CUTOFF)
    exact = np.sort(np.asarray(anm_exact(a_, b_, c_) if dim == 3 else gnm_exact(a_, b_, c_), dtype=np.float64))
    scale = exact.max()
    model = sc.ANM(coord, ff) if dim == 3 else sc.GNM(coord, ff)
    h = (sc.ANM(coord, ff).hessian if dim == 3 else sc.GNM(coord, ff).kirchhoff)
    ref = np.linalg.eigh(h)
    assert np.abs(ref[0] - exact).max() <= 1e-12 * scale
    # the distinct values, merged where closer than the smallest gap a bound may sit in
    distinct = [exact[0]]
    for x in exact[1:]:
        if x - distinct[-1] > MIN_GAP * scale:
            distinct.append(x)
    for k0, k1 in [(1, 4), (3, 9), (0, 2)]:
        vl = -np.inf if k0 == 0 else 0.5 * (distinct[k0 - 1] + distinct[k0])
        vu = 0.5 * (distinct[k1 - 1] + distinct[k1])
        m = int(np.count_nonzero((exact > vl) & (exact <= vu)))
        il = int(np.count_nonzero(exact <= vl))
        w, v = model.eigen(subset_by_value=(vl, vu))
        assert len(w) == m, (dim, k0, k1, len(w), m)
        _gate(f"lattice dim={dim} ({vl:.3g}, {vu:.3g}] closed form m={m}", h, w, v, ref, il, m, scale=scale)
        assert np.abs(w - exact[il:il + m]).max() <= TOL_W * scale


# ---- scaling and agreement with the index path ---------------------------------------------------------------------

@pytest.mark.parametrize("factor", [1e120, 1e-120])
@pytest.mark.parametrize("two_stage", [False, True], ids=["one_stage", "two_stage"])
def test_badly_scaled_matrix(sc, two_stage_path, factor, two_stage):
    """Entries ~1e+-120: the solver scales the matrix by a power of two f != 1, and the bounds with it."""
    two_stage_path(two_stage)
    n = 600
    base = _sym(23, n)
    ref0 = np.linalg.eigh(base)
    vl, vu, il, m = _window(ref0[0], 150, 260)
    a = base * factor
    w, v = sc.nma.eigh(a, subset_by_value=(vl * factor, vu * factor))
    assert len(w) == m, (factor, len(w), m)
    _gate(f"scaled {factor:g} {two_stage}", base, w / factor, v, ref0, il, m)
    # a window entirely in the scaled matrix' range above its largest eigenvalue, and the whole of it
    assert len(sc.nma.eigh(a, eigenvectors=False, subset_by_value=(ref0[0][-1] * 2 * factor, np.inf))) == 0
    assert len(sc.nma.eigh(a, eigenvectors=False, subset_by_value=(-np.inf, 1e308))) == n


def test_agrees_with_the_index_path(sc):
    n = 1000
    a = _sym(91, n)
    ref = np.linalg.eigh(a)
    scale = np.abs(ref[0]).max()
    vl, vu, il, m = _window(ref[0], 300, 420)
    w, v = sc.nma.eigh(a, subset_by_value=(vl, vu))
    wi, vi = sc.nma.eigh(a, subset_by_index=(il, il + m - 1))
    assert len(w) == m
    assert np.abs(w - wi).max() <= 1e-13 * scale
    # the same subspace: || V V^T - Vi Vi^T ||_2 (both orthonormal)
    d = v.T @ v - vi.T @ vi
    assert np.linalg.norm(d, 2) <= 1e-10, np.linalg.norm(d, 2)


# ---- model entry points -------------------------------------------------------------------------------------------

def _atoms(sc, coord):
    atoms = sc.AtomArray(len(coord))
    atoms.coord = coord
    return atoms


@pytest.mark.parametrize("masses", [False, True], ids=["unit", "masses"])
@pytest.mark.parametrize("kind", ["anm", "gnm"])
def test_models(sc, kind, masses):
    """ANM on the fused coordinates-in path (sc_anm_eigen_window_f64), GNM through its host matrix."""
    from springcraft_amd import _hip

    n_atoms = 300
    coord = synthetic_coord(n_atoms, 7)
    ff = sc.InvariantForceField(13.0)
    ms = np.random.RandomState(2).uniform(50.0, 200.0, n_atoms) if masses else None
    cls = sc.ANM if kind == "anm" else sc.GNM
    make = (lambda: cls(_atoms(sc, coord), ff, masses=ms)) if masses else (lambda: cls(coord, ff))
    h = make().hessian if kind == "anm" else make().kirchhoff
    ref = np.linalg.eigh(h)
    w_ref = ref[0]
    scale = np.abs(w_ref).max()
    ntriv = 6 if kind == "anm" else 1
    assert np.abs(w_ref[:ntriv]).max() <= 1e-10 * scale and w_ref[ntriv] > 1e-5 * scale
    vu, i1 = _bound_below(w_ref, 60, scale)
    ctx = _hip.context()
    for vl, il in [(1e-6 * scale, ntriv), (-np.inf, 0)]:
        model = make()
        w, v = model.eigen(subset_by_value=(vl, vu))
        assert model._matrix is None or kind == "gnm"      # the ANM stayed on the fused path
        _gate(f"{kind} masses={masses} ({vl:.3g}, {vu:.3g}]", h, w, v, ref, il, i1 - il)
        w2, _ = sc.nma.eigen(make(), subset_by_value=(vl, vu))
        assert np.array_equal(w2, w)
    ctx.synchronize()


# ---- batches ----------------------------------------------------------------------------------------------------------

def _batch_setup(sc):
    n_atoms = 120
    coord = synthetic_coord(n_atoms, 13)
    ff = sc.InvariantForceField(13.0)
    h = sc.compute_hessian(coord, ff)[0]
    w0 = np.linalg.eigh(h)[0]
    scale = w0.max()
    vl, _ = _bound_below(w0, 30, scale)
    vu, _ = _bound_below(w0, 60, scale)
    # member 1: eigenvalues x 1.7 (fewer in the window); member 2: x c with c w0_max inside the window, so that its window
    # reaches the top of its spectrum (il > n - K); member 3: x 0.6
    top = 0.5 * (vl + vu) / scale
    factors = [1.0, 1.7, top, 0.6]
    for b, f in enumerate(factors):      # keep every member's spectrum away from the bounds
        wf = w0 * f
        while np.min(np.abs(wf - vl)) < 1e-4 * scale * f or np.min(np.abs(wf - vu)) < 1e-4 * scale * f:
            f *= 1.0 + 1e-3
            wf = w0 * f
        factors[b] = f
    return coord, ff, h, (vl, vu), factors


def _batch_refs(h, factors, window):
    vl, vu = window
    refs = []
    for f in factors:
        w, v = np.linalg.eigh(h * f)
        il = int(np.count_nonzero(w <= vl))
        m = int(np.count_nonzero(w <= vu)) - il
        refs.append((h * f, (w, v), il, m))
    return refs


def _solve_batch(sc, coord, ff, factors, window, K, want_vectors=True):
    import torch

    from springcraft_amd.batch import DeviceBatchSolver

    batch, n_atoms = len(factors), len(coord)
    masses = np.repeat(1.0 / np.asarray(factors)[:, None], n_atoms, axis=1)
    s = DeviceBatchSolver(n_atoms, batch, ff, masses=masses, want_vectors=want_vectors, subset_by_value=window,
                          max_modes=K)
    s.solve(torch.from_numpy(np.repeat(coord[None], batch, axis=0)).cuda())
    return s


def test_batch_solver_members_with_different_counts(sc):
    coord, ff, h, window, factors = _batch_setup(sc)
    refs = _batch_refs(h, factors, window)
    n = 3 * len(coord)
    counts = [m for *_, m in refs]
    K = max(counts) + 3
    assert len(set(counts)) >= 3, counts
    assert any(il > n - K for _, _, il, _ in refs), [(il, m) for *_, il, m in refs]      # compaction offset
    s = _solve_batch(sc, coord, ff, factors, window, K)
    w, v = s.finish()
    assert tuple(w.shape) == (len(factors), K) and tuple(v.shape) == (len(factors), K, n)
    assert s.counts.dtype == s.torch.int64 and s.counts.is_cuda
    got = s.counts.cpu().numpy()
    assert got.tolist() == counts, (got, counts)
    w, v = w.cpu().numpy(), v.cpu().numpy()
    for b, (hb, ref, il, m) in enumerate(refs):
        _gate(f"batch member {b} il={il} m={m} K={K}", hb, w[b, :m], v[b, :m], ref, il, m)
        assert np.all(np.isnan(w[b, m:])) and np.all(v[b, m:] == 0.0), b
    # values only: the same windows
    s2 = _solve_batch(sc, coord, ff, factors, window, K, want_vectors=False)
    w2, v2 = s2.finish()
    assert v2 is None and s2.counts.cpu().numpy().tolist() == counts
    w2 = w2.cpu().numpy()
    for b, (_, ref, il, m) in enumerate(refs):
        assert np.abs(w2[b, :m] - ref[0][il:il + m]).max() <= TOL_W * np.abs(ref[0]).max()
        assert np.all(np.isnan(w2[b, m:]))


def test_batch_solver_overflow(sc):
    coord, ff, h, window, factors = _batch_setup(sc)
    refs = _batch_refs(h, factors, window)
    counts = [m for *_, m in refs]
    K = sorted(counts)[1]                 # smaller than the two largest counts
    over = [b for b, c in enumerate(counts) if c > K]
    assert over
    s = _solve_batch(sc, coord, ff, factors, window, K)
    with pytest.raises(ValueError) as e:
        s.finish()
    for b in over:
        assert f"{b} ({counts[b]})" in str(e.value), (str(e.value), b)
    assert s.counts.cpu().numpy().tolist() == counts
    w, v = s.w.cpu().numpy(), s.v.cpu().numpy()
    for b, (hb, ref, il, m) in enumerate(refs):
        keep = min(m, K)
        _gate(f"overflow member {b} m={m} K={K}", hb, w[b, :keep], v[b, :keep], ref, il, keep)
        assert np.all(np.isnan(w[b, keep:])) and np.all(v[b, keep:] == 0.0)


@pytest.mark.parametrize("two_stage", [False, True], ids=["one_stage", "two_stage"])
def test_dev_entry_nan_member(sc, two_stage):
    """sc_dev_eigh_window_f64 on matrices: a NaN member raises LinAlgError once and gets count 0, the others are right."""
    import torch

    from springcraft_amd import _hip

    n, batch, K = 520, 4, 90
    mats = np.stack([_sym(61 + b, n) for b in range(batch)])
    refs = [np.linalg.eigh(m) for m in mats]
    spectra = np.sort(np.concatenate([refs[b][0] for b in (0, 1, 3)]))      # bounds in gaps of all members' spectra
    vl, vu, _, _ = _window(spectra, 600, 780)
    mats_in = mats.copy()
    mats_in[2, 300, 17] = np.nan
    ctx = _hip.Context(0)
    try:
        ctx.set_two_stage(two_stage)
        a = torch.from_numpy(mats_in).cuda()
        w = torch.full((batch, K), -7.0, dtype=torch.float64, device="cuda")
        v = torch.full((batch, K, n), -7.0, dtype=torch.float64, device="cuda")
        cnt = torch.full((batch,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.check(_hip.lib().sc_dev_eigh_window_f64(ctx.handle, C.c_void_p(a.data_ptr()), n, batch, vl, vu, K,
                                                    C.c_void_p(w.data_ptr()), C.c_void_p(v.data_ptr()),
                                                    C.c_void_p(cnt.data_ptr())))
        with pytest.raises(np.linalg.LinAlgError):
            ctx.synchronize()
        ctx.synchronize()              # reported once
    finally:
        ctx.close()
    w, v, cnt = w.cpu().numpy(), v.cpu().numpy(), cnt.cpu().numpy()
    assert cnt[2] == 0 and np.all(np.isnan(w[2])) and np.all(v[2] == 0.0)
    for b in (0, 1, 3):
        w_ref = refs[b][0]
        il = int(np.count_nonzero(w_ref <= vl))
        m = int(np.count_nonzero(w_ref <= vu)) - il
        assert cnt[b] == m and m <= K, (b, cnt[b], m)
        _gate(f"dev entry member {b} {two_stage}", mats[b], w[b, :m], v[b, :m], refs[b], il, m)
        assert np.all(np.isnan(w[b, m:])) and np.all(v[b, m:] == 0.0)


def test_device_checks_on_a_window(sc):
    """The window of an ANM at n = 3000 (one matrix, fused path) checked on the device against its assembled Hessian."""
    import torch

    from springcraft_amd.batch import DeviceBatchSolver

    coord = synthetic_coord(1000, 5)
    ff = sc.InvariantForceField(13.0)
    assembler = DeviceBatchSolver(1000, 1, ff, want_vectors=False)
    hd = assembler.assemble(torch.from_numpy(coord[None]).cuda())[0].clone()
    w_all = sc.nma.eigh(sc.compute_hessian(coord, ff)[0], eigenvectors=False)
    scale = w_all.max()
    vu, i1 = _bound_below(w_all, 112, scale)
    w, v = sc.ANM(coord, ff).eigen(subset_by_value=(1e-6 * scale, vu))
    assert len(w) == i1 - 6
    assert np.abs(w - w_all[6:i1]).max() <= TOL_W * scale
    res, orth = device_checks(torch, hd, torch.from_numpy(w).cuda(), torch.from_numpy(v).cuda(), scale=scale)
    print(f"ANM n=3000 window m={len(w)}: res {res:.1e}, orth {orth:.1e}")
    assert res <= TOL_RES and orth <= TOL_ORTH
