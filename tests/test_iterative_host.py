"""
Host tests (no GPU) of springcraft_amd.iterative: the spectral bound, the Chebyshev filter coefficients, the
subspace-iteration driver with NumPy stand-ins for the panel step and the small eigensolver, and the argument checks of
``PairOperator.lowest_modes``.

Structures (shared with tests/test_pair_panel_gpu.py and tests/test_iterative_gpu.py): :func:`lattice`, a cubic lattice of
spacing 3.8 A plus ``RandomState(seed).uniform(-0.3, 0.3)`` jitter; under ``InvariantForceField(7.0)`` (constant 1 within
7 A) every atom has 6 .. 26 contacts and the network is connected with exactly six zero modes, which
:func:`test_structures_are_connected` checks in NumPy.  A = ``lattice(4, 5, 6, 3)`` (N = 120), B = ``lattice(6, 6, 8, 4)``
(N = 288); masses ``RandomState(5).uniform(50, 200, N)``.  The matrices here are NumPy's own (:func:`np_network`), not the
package's, which needs the device.
"""
import numpy as np
import pytest

from springcraft_amd import iterative

CUTOFF = 7.0
MAX_ITER, DEGREE, TOL = 60, 20, 1e-10   # the solver tests' settings; the reference iteration needs at most 19 passes


def lattice(nx, ny, nz, seed):
    grid = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3) * 3.8
    return grid + np.random.RandomState(seed).uniform(-0.3, 0.3, grid.shape)


def masses_of(n):
    return np.random.RandomState(5).uniform(50, 200, n)


def np_network(coord, cutoff=CUTOFF):
    """(pairs (k, 2) sorted by first then second atom, gamma (k,) = 1) of the contacts within ``cutoff``."""
    d = coord[None] - coord[:, None]
    r2 = (d * d).sum(-1)
    pairs = np.argwhere((r2 <= cutoff * cutoff) & (r2 > 0)).astype(np.int64)
    return pairs, np.ones(len(pairs))


def np_matrix(coord, pairs, gamma, dim, scale=None):
    """The dense (dim N, dim N) matrix ``T H T`` of a directed pair list in NumPy."""
    n = len(coord)
    i, j = pairs[:, 0], pairs[:, 1]
    if dim == 3:
        d = coord[j] - coord[i]
        blk = -gamma[:, None, None] * d[:, :, None] * d[:, None, :] / (d * d).sum(axis=1)[:, None, None]
        h = np.zeros((n, n, 3, 3))
        h[i, j] = blk
        np.subtract.at(h, (i, i), blk)
        h = h.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n)
    else:
        h = np.zeros((n, n))
        h[i, j] = -gamma
        np.subtract.at(h, (i, i), -gamma)
    if scale is not None:
        s = np.repeat(scale, dim)
        h = h * np.outer(s, s)
    return h


@pytest.fixture(scope="module")
def a_case():
    coord = lattice(4, 5, 6, 3)
    pairs, gamma = np_network(coord)
    return coord, pairs, gamma


def test_structures_are_connected():
    for dims, seed, n in (((4, 5, 6), 3, 120), ((6, 6, 8), 4, 288)):
        coord = lattice(*dims, seed)
        pairs, gamma = np_network(coord)
        degree = np.bincount(pairs[:, 0], minlength=n)
        assert len(coord) == n and degree.min() >= 6 and degree.max() <= 26
        lam = np.linalg.eigvalsh(np_matrix(coord, pairs, gamma, 3))
        assert np.all(np.abs(lam[:6]) <= 1e-12 * lam[-1]) and lam[6] > 1e-4 * lam[-1]
        assert np.linalg.eigvalsh(np_matrix(coord, pairs, gamma, 1))[1] > 1e-4


def test_spectral_bound_bounds_the_spectrum(a_case):
    coord, pairs, gamma = a_case
    n = len(coord)
    scale = 1.0 / np.sqrt(masses_of(n))
    for dim, t in ((3, None), (3, scale), (1, None), (1, scale)):
        b = iterative.spectral_bound(pairs, gamma, n, t)
        lam_max = np.linalg.eigvalsh(np_matrix(coord, pairs, gamma, dim, t))[-1]
        print(f"dim {dim} {'mass' if t is not None else 'plain'}: b = {b:.6g}, lambda_max = {lam_max:.6g}")
        assert b >= lam_max
    assert iterative.spectral_bound(pairs, gamma, n) == 2.0 * np.bincount(pairs[:, 0]).max()
    # one spring negated, both directions: the bound sums |gamma| and holds for max |lambda|
    neg = gamma.copy()
    p = len(pairs) // 2
    back = np.nonzero((pairs[:, 0] == pairs[p, 1]) & (pairs[:, 1] == pairs[p, 0]))[0][0]
    neg[[p, back]] = -1.0
    lam = np.linalg.eigvalsh(np_matrix(coord, pairs, neg, 3))
    assert not np.array_equal(lam, np.linalg.eigvalsh(np_matrix(coord, pairs, gamma, 3)))
    assert iterative.spectral_bound(pairs, neg, n) >= np.abs(lam).max()
    assert iterative.spectral_bound(pairs, neg, n) == iterative.spectral_bound(pairs, gamma, n)
    assert iterative.spectral_bound(np.empty((0, 2), dtype=np.int64), np.empty(0), 1) == 0.0
    with pytest.raises(ValueError):
        iterative.spectral_bound(pairs, gamma[:-1], n)
    with pytest.raises(IndexError):
        iterative.spectral_bound(pairs, gamma, n, scale[:-1])


@pytest.mark.parametrize("degree", [1, 2, 7])
def test_filter_coefficients_are_the_scaled_chebyshev_polynomial(a_case, degree):
    coord, pairs, gamma = a_case
    h = np_matrix(coord, pairs, gamma, 3)
    lam, vec = np.linalg.eigh(h)
    b = iterative.spectral_bound(pairs, gamma, len(coord))
    a0, a = lam[6], lam[40]
    x = np.random.RandomState(1).standard_normal((len(h), 5))
    steps = iterative.filter_coefficients(a0, a, b, degree)
    assert len(steps) == degree and steps[0][2] == 0.0
    prev, cur = None, x
    for alpha, beta, gamma_c in steps:
        nxt = alpha * (h @ cur) + beta * cur + (gamma_c * prev if gamma_c != 0 else 0.0)
        prev, cur = cur, nxt
    e, c = (b - a) / 2, (b + a) / 2
    cheb = np.polynomial.chebyshev.Chebyshev.basis(degree)
    ref = vec @ ((cheb((lam - c) / e) / cheb((a0 - c) / e))[:, None] * (vec.T @ x))
    print(f"degree {degree}: max err {np.abs(cur - ref).max():.3e} at max |result| {np.abs(ref).max():.3e}")
    assert np.abs(cur - ref).max() <= 1e-12 * np.abs(ref).max()
    # 1 at a0, within 1 / |T_d| on [a, b]
    damp = np.abs(cheb((lam[lam >= a] - c) / e) / cheb((a0 - c) / e))
    assert damp.max() <= 1.0 / abs(cheb((a0 - c) / e)) * (1 + 1e-12)


def test_filter_coefficients_refuse_a_bad_interval():
    with pytest.raises(ValueError, match="a0 < a < b"):
        iterative.filter_coefficients(1.0, 1.0, 2.0, 3)
    with pytest.raises(ValueError, match="a0 < a < b"):
        iterative.filter_coefficients(0.0, 3.0, 2.0, 3)
    with pytest.raises(ValueError, match="degree"):
        iterative.filter_coefficients(0.0, 1.0, 2.0, 0)


def np_callables(h):
    """The driver's two callables on CPU tensors: a dense NumPy panel step and numpy.linalg.eigh."""
    import torch

    calls = []

    def panel_step(x, z, alpha, beta, gamma_c):
        assert x.data_ptr() != z.data_ptr() and x.is_contiguous() and z.is_contiguous()
        r = alpha * (h @ x.numpy()) + beta * x.numpy()
        if gamma_c != 0:
            r += gamma_c * z.numpy()
        z.copy_(torch.from_numpy(r))
        calls.append((alpha, beta, gamma_c))

    def small_eigh(a):
        w, u = np.linalg.eigh(a.numpy())
        return torch.from_numpy(w), torch.from_numpy(u)

    return panel_step, small_eigh, calls


@pytest.mark.parametrize("seed", [0, 1])
def test_driver_converges_on_the_host(a_case, seed):
    import torch

    coord, pairs, gamma = a_case
    h = np_matrix(coord, pairs, gamma, 3)
    lam = np.linalg.eigvalsh(h)
    b = iterative.spectral_bound(pairs, gamma, len(coord))
    k, guard, nb = iterative.checked_block(18, None, len(h))
    assert (guard, nb) == (8, 26) and iterative.default_guard(100) == 25
    panel_step, small_eigh, calls = np_callables(h)
    x0 = torch.from_numpy(iterative.start_block(None, len(h), nb, seed))
    w, x, info = iterative.chebyshev_subspace_iteration(panel_step, small_eigh, x0, k, b, tol=TOL, degree=DEGREE,
                                                        max_iter=MAX_ITER)
    w, x = w.numpy(), x.numpy()
    print(f"seed {seed}: {info['iterations']} passes, {info['panel_steps']} panel steps, max residual / b "
          f"{info['residuals'].max() / b:.2e}, max |w - lambda| / b {np.abs(w - lam[:k]).max() / b:.2e}, "
          f"|V^T V - I| {np.abs(x.T @ x - np.eye(k)).max():.2e}")
    assert info["converged"] and info["iterations"] <= MAX_ITER and info["b"] == b
    assert info["panel_steps"] == len(calls) == info["iterations"] * DEGREE + info["iterations"] + 1
    assert w.shape == (k,) and x.shape == (len(h), k) and np.all(np.diff(w) >= 0)
    assert np.all(np.abs(w - lam[:k]) <= TOL * b + 1e-12 * b)
    assert np.abs(x.T @ x - np.eye(k)).max() <= 1e-12
    res = np.linalg.norm(h @ x - x * w, axis=0)
    assert np.all(res <= TOL * b + 1e-12 * b) and np.allclose(res, info["residuals"], rtol=1e-3, atol=1e-13 * b)


def test_driver_returns_unconverged_pairs_without_raising(a_case):
    import torch

    coord, pairs, gamma = a_case
    h = np_matrix(coord, pairs, gamma, 3)
    b = iterative.spectral_bound(pairs, gamma, len(coord))
    panel_step, small_eigh, _ = np_callables(h)
    x0 = torch.from_numpy(iterative.start_block(None, len(h), 26, 0))
    w, x, info = iterative.chebyshev_subspace_iteration(panel_step, small_eigh, x0, 18, b, tol=TOL, degree=DEGREE, max_iter=1)
    assert not info["converged"] and info["iterations"] == 1 and info["panel_steps"] == DEGREE + 2
    assert np.all(np.isfinite(w.numpy())) and np.all(np.isfinite(x.numpy()))
    assert np.abs(x.numpy().T @ x.numpy() - np.eye(18)).max() <= 1e-12


def test_start_block_pads_and_truncates():
    m, nb = 30, 7
    rows = np.random.RandomState(2).standard_normal((3, m))
    x = iterative.start_block(rows, m, nb, 0)
    assert x.shape == (m, nb) and np.array_equal(x[:, :3], rows.T)
    assert np.array_equal(x, iterative.start_block(rows, m, nb, 0)) and not np.array_equal(x, iterative.start_block(rows, m, nb, 1))
    assert np.linalg.matrix_rank(x) == nb
    many = np.random.RandomState(3).standard_normal((9, m))
    assert np.array_equal(iterative.start_block(many, m, nb, 0), many[:nb].T)
    assert np.array_equal(iterative.start_block(None, m, nb, 4), np.random.RandomState(4).standard_normal((m, nb)))


def test_lowest_modes_refuses_bad_arguments_before_touching_the_device():
    from springcraft_amd import PairOperator

    op = PairOperator.__new__(PairOperator)   # (no device: the refusals come first)
    op.m = 360
    with pytest.raises(ValueError, match="k must be at least 1"):
        op.lowest_modes(0)
    with pytest.raises(ValueError, match="exceed the order"):
        op.lowest_modes(355)
    with pytest.raises(ValueError, match="exceed the order"):
        op.lowest_modes(18, guard=343)
    with pytest.raises(ValueError, match="guard"):
        op.lowest_modes(18, guard=-1)
    with pytest.raises(ValueError, match="degree"):
        op.lowest_modes(18, degree=0)
    for bad in (np.zeros((2, 359)), np.zeros(360), np.zeros((0, 360))):
        with pytest.raises(ValueError, match="start rows"):
            op.lowest_modes(18, start=bad)
