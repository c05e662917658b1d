"""
Host tests (no GPU) of the conjugate-gradient solve of springcraft_amd.iterative: the closed-form null space, the driver
:func:`iterative.conjugate_gradient` with NumPy stand-ins for the device entries, deflation, and the argument checks of
``PairOperator.solve``, ``linear_response``, ``covariance_columns``.

Structures (tests/test_iterative_host.py): A = ``lattice(4, 5, 6, 3)`` (N = 120), B = ``lattice(6, 6, 8, 4)`` (N = 288), and A19,
A without its last atom (N = 119, not a multiple of the four atoms of a workgroup), under a cutoff of 7 A with constant 1;
masses ``RandomState(5).uniform(50, 200, N)``.  The matrices are NumPy's own (:func:`np_matrix`).

Right-hand sides: five ``RandomState(11).standard_normal`` columns and the unit vectors of the first and the last atom.
Settings ``tol = 1e-10``, ``max_iter = 300``.  The cap is a condition, not a measurement: this NumPy iteration needs at most
70 (A plain), 89 (A mass-weighted), 36 (A as a GNM), 93 (B plain) iterations, and 46, 60, 22, 61 with the 18 lowest modes
deflated (10 for the GNM).

Gates per column, with ``f_p`` the projected right-hand side, ``lambda_nz`` the lowest non-zero eigenvalue, ``b`` the spectral
bound and ``H^+`` from ``numpy.linalg.eigh``: ``|f_p - H x| <= tol |f_p| + 1e-12 b |x|`` (the stopping rule plus the rounding
of one product), ``|x - H^+ f| <= tol |f_p| / lambda_nz + 1e-12 |H^+ f|`` (its error bound), ``|Z^T x| <= 1e-12 |x|``.
"""
import numpy as np
import pytest

from springcraft_amd import iterative
from tests.test_iterative_host import lattice, masses_of, np_matrix, np_network

TOL, MAX_ITER = 1e-10, 300
CASES = [("A", False, 3), ("A", True, 3), ("A", False, 1), ("B", False, 3)]
CASE_IDS = ["A-plain", "A-mass", "A-gnm", "B-plain"]


def coord_of(name):
    if name == "A19":
        return lattice(4, 5, 6, 3)[:-1]
    return lattice(4, 5, 6, 3) if name == "A" else lattice(6, 6, 8, 4)


def right_hand_sides(n, dim):
    """(7, dim n): five random rows, the unit vectors of the first and of the last atom's first coordinate."""
    m = dim * n
    f = np.zeros((7, m))
    f[:5] = np.random.RandomState(11).standard_normal((5, m))
    f[5, 0] = 1.0
    f[6, dim * (n - 1)] = 1.0
    return f


def dense_reference(h, z, b, f):
    """``(f_p, H^+ f, lambda_nz)`` of the rows ``f`` from ``numpy.linalg.eigh`` of ``h`` with ``z.shape[1]`` zero modes."""
    lam, vec = np.linalg.eigh(h)
    nz = z.shape[1]
    assert np.all(np.abs(lam[:nz]) <= 1e-9 * b) and lam[nz] > 1e-6 * b
    fp = f - (f @ z) @ z.T
    x = ((f @ vec[:, nz:]) / lam[nz:]) @ vec[:, nz:].T
    return fp, x, lam[nz]


def check_solution(x, info, h, z, b, f, tol=TOL, label=""):
    """The gates of the module docstring for the rows ``x`` of the right-hand sides ``f``; prints each figure first."""
    fp, ref, lam_nz = dense_reference(h, z, b, f)
    nrm = lambda a: np.linalg.norm(a, axis=1)   # noqa: E731
    res, err, nul = nrm(fp - x @ h), nrm(x - ref), nrm(x @ z)
    gate_res = tol * nrm(fp) + 1e-12 * b * nrm(x)
    gate_err = tol * nrm(fp) / lam_nz + 1e-12 * nrm(ref)
    print(f"{label}: iterations {info['iterations'].min()}..{info['iterations'].max()}, residual / gate "
          f"{(res / gate_res).max():.3f}, error / gate {(err / gate_err).max():.3f}, |Z^T x| / |x| {(nul / nrm(x)).max():.2e}")
    assert info["converged"] and np.all(info["status"] == 1)
    assert np.all(res <= gate_res) and np.all(err <= gate_err) and np.all(nul <= 1e-12 * nrm(x))
    assert np.all(info["residuals"] <= tol)


def np_cg_callables(h):
    """
    The driver's callables in NumPy on CPU tensors: the recurrence of csrc/pair_cg.hip, column by column, with a dense
    product.  Returns ``(init, step, panels)``; ``panels`` holds X, R, P, Q and the state arrays once ``init`` ran.
    """
    import torch

    st = {}

    def init(r, tol):
        rn = r.numpy()
        st.update(R=rn, X=np.zeros_like(rn), P=rn.copy(), Q=np.zeros_like(rn), rho=(rn * rn).sum(axis=0))
        st.update(stop=tol * tol * st["rho"], status=np.where(st["rho"] == 0, 1, 0), iters=np.zeros(rn.shape[1], dtype=np.int64))
        return torch.from_numpy(st["X"]), lambda: (st["status"].copy(), st["iters"].copy(), st["rho"].copy())

    def step(iterations):
        for _ in range(iterations):
            st["Q"][:] = h @ st["P"]
            pq = (st["P"] * st["Q"]).sum(axis=0)
            run = st["status"] == 0
            bad = run & ~((pq > 0) & np.isfinite(pq))
            st["status"][bad] = 2
            run &= ~bad
            alpha = np.where(run, st["rho"] / np.where(run, pq, 1.0), 0.0)
            st["X"][:, run] += (alpha * st["P"])[:, run]
            st["R"][:, run] -= (alpha * st["Q"])[:, run]
            new = (st["R"] * st["R"]).sum(axis=0)
            beta = np.where(run, new / np.where(run, st["rho"], 1.0), 0.0)
            st["rho"][run] = new[run]
            st["iters"][run] += 1
            st["status"][run & (new <= st["stop"])] = 1
            run = st["status"] == 0
            st["P"][:, run] = (st["R"] + beta * st["P"])[:, run]

    return init, step, st


def host_case(name, masses, dim):
    coord = coord_of(name)
    n = len(coord)
    pairs, gamma = np_network(coord)
    scale = 1.0 / np.sqrt(masses_of(n)) if masses else None
    h = np_matrix(coord, pairs, gamma, dim, scale)
    return coord, scale, h, iterative.spectral_bound(pairs, gamma, n, scale), iterative.null_space(coord, dim, scale)


def host_solve(h, z, b, f, **options):
    import torch

    init, step, _ = np_cg_callables(h)
    if options.get("deflate") is not None:
        options["deflate"] = tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in options["deflate"])
    x, info = iterative.conjugate_gradient(init, step, torch.from_numpy(f.T.copy()), torch.from_numpy(z), b,   # (overwritten)
                                           apply=lambda t: torch.from_numpy(h @ t.numpy()), **options)
    return x.numpy().T, info


def test_a_without_its_last_atom_is_connected():
    coord = coord_of("A19")
    pairs, gamma = np_network(coord)
    assert len(coord) == 119 and np.bincount(pairs[:, 0], minlength=119).min() >= 6
    lam = np.linalg.eigvalsh(np_matrix(coord, pairs, gamma, 3))
    assert np.all(np.abs(lam[:6]) <= 1e-12 * lam[-1]) and lam[6] > 1e-4 * lam[-1]


@pytest.mark.parametrize("name", ["A", "A19"])
@pytest.mark.parametrize("dim", [3, 1])
@pytest.mark.parametrize("masses", [False, True], ids=["plain", "mass"])
def test_null_space_is_orthonormal_and_annihilated(name, dim, masses):
    coord, scale, h, b, z = host_case(name, masses, dim)
    assert z.shape == (dim * len(coord), 6 if dim == 3 else 1)
    print(f"|Z^T Z - I| {np.abs(z.T @ z - np.eye(z.shape[1])).max():.2e}, |H Z| / b {np.abs(h @ z).max() / b:.2e}")
    assert np.abs(z.T @ z - np.eye(z.shape[1])).max() <= 1e-12
    assert np.abs(h @ z).max() <= 1e-12 * b and np.linalg.norm(h @ z, axis=0).max() <= 1e-12 * b


def test_null_space_of_degenerate_shapes():
    assert iterative.null_space(np.zeros((1, 3)), 3).shape == (3, 3)
    assert iterative.null_space(np.arange(12.0).reshape(4, 3), 3).shape == (12, 5)   # collinear atoms
    assert np.allclose(iterative.null_space(5, 1), 1 / np.sqrt(5))
    with pytest.raises(IndexError):
        iterative.null_space(np.zeros((4, 3)), 3, np.ones(3))
    with pytest.raises(ValueError, match="dim"):
        iterative.null_space(np.zeros((4, 3)), 2)


def test_column_dots_do_not_depend_on_the_other_columns():
    import torch

    rng = np.random.RandomState(2)
    z, f = torch.from_numpy(rng.standard_normal((357, 6))), torch.from_numpy(rng.standard_normal((357, 9)))
    full = iterative.column_dots(z, f)
    assert np.abs(full.numpy() - (z.T @ f).numpy()).max() <= 1e-13 * 357
    for c in (0, 4, 8):
        assert torch.equal(iterative.column_dots(z, f[:, c: c + 1].contiguous())[:, 0], full[:, c])


@pytest.mark.parametrize("key", CASES, ids=CASE_IDS)
def test_driver_solves_on_the_host(key):
    name, masses, dim = key
    coord, scale, h, b, z = host_case(name, masses, dim)
    f = right_hand_sides(len(coord), dim)
    x, info = host_solve(h, z, b, f, tol=TOL, max_iter=MAX_ITER)
    check_solution(x, info, h, z, b, f, label="undeflated")
    assert info["b"] == b and info["tol"] == TOL and info["iterations"].max() <= MAX_ITER
    # deflation with the dense matrix's own eigenvectors: the same gates, fewer iterations
    k = 18 if dim == 3 else 10
    lam, vec = np.linalg.eigh(h)
    xd, infod = host_solve(h, z, b, f, tol=TOL, max_iter=MAX_ITER, deflate=(lam[:k], vec[:, :k].T))
    check_solution(xd, infod, h, z, b, f, label=f"{k} modes deflated")
    assert infod["iterations"].max() < info["iterations"].max()
    # a column alone passes the same gates (the same bits only on the device: this stand-in's dense product promises none)
    one, info1 = host_solve(h, z, b, f[3:4], tol=TOL, max_iter=MAX_ITER)
    check_solution(one, info1, h, z, b, f[3:4], label="one column")

def test_a_zero_right_hand_side_is_solved_at_once():
    coord, scale, h, b, z = host_case("A", False, 3)
    f = right_hand_sides(len(coord), 3)[:3]
    f[1] = 0.0
    x, info = host_solve(h, z, b, f, tol=TOL, max_iter=MAX_ITER)
    assert np.all(x[1] == 0.0) and info["status"][1] == 1 and info["iterations"][1] == 0 and info["residuals"][1] == 0.0
    assert info["converged"] and info["iterations"][0] > 0
    # a right-hand side inside the null space is a zero one after the projection, up to rounding
    x, info = host_solve(h, z, b, z[:, :1].T.copy(), tol=TOL, max_iter=MAX_ITER)
    assert np.abs(x).max() <= 1e-12 / np.linalg.eigvalsh(h)[6]


def test_running_out_of_iterations_raises_nothing():
    coord, scale, h, b, z = host_case("A", False, 3)
    f = right_hand_sides(len(coord), 3)
    x, info = host_solve(h, z, b, f, tol=TOL, max_iter=5, check_every=2)
    assert info["converged"] is False and np.all(info["status"] == 0) and np.all(info["iterations"] == 5)
    assert np.all(np.isfinite(x)) and np.all(info["residuals"] > TOL)


def test_refusals_fire_before_the_device_is_touched():
    from springcraft_amd import PairOperator

    op = PairOperator.__new__(PairOperator)   # (no device: the refusals come first)
    op.m, op.n_atoms, op.dim = 360, 120, 3
    f = np.zeros((2, 360))
    for bad in (np.zeros(359), np.zeros((2, 361)), np.zeros((2, 120, 3))):
        with pytest.raises(ValueError, match="right-hand sides"):
            op.solve(bad)
    with pytest.raises(ValueError, match="tol"):
        op.solve(f, tol=0.0)
    with pytest.raises(ValueError, match="tol"):
        op.solve(f, tol=-1e-8)
    with pytest.raises(ValueError, match="check_every"):
        op.solve(f, check_every=0)
    with pytest.raises(ValueError, match="max_iter"):
        op.solve(f, max_iter=-1)
    for bad in ((np.zeros(3), np.zeros((3, 359))), (np.zeros(4), np.zeros((3, 360))), (np.zeros(3), np.zeros(360)), np.zeros(3)):
        with pytest.raises(ValueError, match="deflate"):
            op.solve(f, deflate=bad)
    with pytest.raises(ValueError, match="force"):
        op.linear_response(np.zeros((119, 3)))
    with pytest.raises(ValueError, match="force"):
        op.linear_response(np.zeros((2, 360)))
    with pytest.raises(IndexError, match="scale"):
        op.linear_response(np.zeros((120, 3)), atom_scale=np.ones(119))
    with pytest.raises(ValueError, match="tol"):
        op.linear_response(np.zeros((120, 3)), tol=0.0)
    for bad in ([120], [-1], [0, 57, 120]):
        with pytest.raises(IndexError, match="outside"):
            op.covariance_columns(bad)
    with pytest.raises(IndexError, match="integer"):
        op.covariance_columns([0.5])
    with pytest.raises(ValueError, match="tol"):
        iterative.checked_solve(360, float("nan"), 10, 1, None)


def test_deflation_with_inexact_modes_still_meets_the_stopping_rule():
    """Ritz pairs of a perturbed subspace (residuals of 1e-9 b, as an iterative eigensolver leaves them): the driver's second
    iteration on the true residual restores ``|f_p - H x| <= tol |f_p|``."""
    coord, scale, h, b, z = host_case("A", False, 3)
    f = right_hand_sides(len(coord), 3)
    lam, vec = np.linalg.eigh(h)
    basis, _ = np.linalg.qr(vec[:, :18] + 1e-9 * np.random.RandomState(4).standard_normal((len(h), 18)))
    w, u = np.linalg.eigh(basis.T @ h @ basis)
    v = (basis @ u).T
    assert 1e-11 * b < np.linalg.norm(v @ h - w[:, None] * v, axis=1).max() < 1e-7 * b
    plain = host_solve(h, z, b, f, tol=TOL, max_iter=MAX_ITER)[1]
    x, info = host_solve(h, z, b, f, tol=TOL, max_iter=MAX_ITER, deflate=(w, v))
    check_solution(x, info, h, z, b, f, label="inexact modes deflated")
    assert info["iterations"].max() < plain["iterations"].max()
    with pytest.raises(ValueError, match="apply"):
        import torch

        iterative.conjugate_gradient(None, None, torch.zeros((360, 1), dtype=torch.float64), torch.from_numpy(z), b,
                                     deflate=(torch.from_numpy(w), torch.from_numpy(v)))
