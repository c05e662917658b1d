"""
GPU tests of the exact pseudo-inverse by conjugate gradients on the device: :meth:`springcraft_amd.PairOperator.solve`,
``linear_response``, ``covariance_columns`` and :meth:`springcraft_amd.RTB.exact_response` (csrc/pair_cg.hip, the driver of
springcraft_amd/iterative.py).

Structures, right-hand sides, settings (``tol = 1e-10``, ``max_iter = 300``) and gates are those of tests/test_solve_host.py,
whose docstring derives them; the reference is ``numpy.linalg.eigh`` of the package's own dense matrix.  The iteration caps
are conditions, not measurements: the NumPy prototype needs at most 70, 89, 36, 93 iterations (A plain, A mass-weighted, A as
a GNM, B plain) and 46, 60, 22, 61 with the 18 lowest modes deflated (10 for the GNM).
"""
import numpy as np
import pytest

from tests.test_iterative_gpu import dense_of
from tests.test_iterative_host import masses_of
from tests.test_solve_host import CASE_IDS, CASES, MAX_ITER, TOL, check_solution, coord_of, right_hand_sides

pytestmark = pytest.mark.gpu
_cache = {}


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


def bits(t):
    import torch

    return t.contiguous().view(torch.int64)


def case_of(sc, key):
    """A case's operator, dense matrix, null space and its undeflated solve (run twice), built once."""
    if key not in _cache:
        name, masses, dim = key
        coord = coord_of(name)
        mass = masses_of(len(coord)) if masses else None
        op = sc.PairOperator(coord, sc.InvariantForceField(7.0), dim=dim, masses=mass)
        f = right_hand_sides(len(coord), dim)
        runs = [op.solve(f, tol=TOL, max_iter=MAX_ITER) for _ in range(2)]
        _cache[key] = {"op": op, "dim": dim, "f": f, "runs": runs, "h": dense_of(sc, coord, dim, mass),
                       "z": op.null_space().cpu().numpy(), "b": op.spectral_bound()}
    return _cache[key]


@pytest.fixture(params=CASES, ids=CASE_IDS)
def case(request, sc):
    return case_of(sc, request.param)


def test_solve_is_the_dense_pseudo_inverse(case):
    x, info = case["runs"][0]
    f = case["f"]
    assert x.is_cuda and tuple(x.shape) == f.shape and info["b"] == case["b"] and info["tol"] == TOL
    assert info["iterations"].shape == info["residuals"].shape == info["status"].shape == (len(f),)
    check_solution(x.cpu().numpy(), info, case["h"], case["z"], case["b"], f, label="device, undeflated")
    assert info["iterations"].max() <= MAX_ITER


def test_the_same_arguments_give_the_same_bits_and_a_column_alone_too(case):
    import torch

    (x0, i0), (x1, i1) = case["runs"]
    assert torch.equal(bits(x0), bits(x1)) and np.array_equal(i0["iterations"], i1["iterations"])
    assert np.array_equal(i0["residuals"], i1["residuals"])
    for c in (0, 3, 6):
        one, info = case["op"].solve(case["f"][c], tol=TOL, max_iter=MAX_ITER)
        assert tuple(one.shape) == (case["f"].shape[1],)
        assert torch.equal(bits(one), bits(x0[c])) and info["iterations"][0] == i0["iterations"][c]


def test_deflation_passes_the_same_gates_in_fewer_iterations(case):
    op, f = case["op"], case["f"]
    k = 18 if case["dim"] == 3 else 10
    w, v, modes = op.lowest_modes(k, tol=1e-10)
    assert modes["converged"]
    x, info = op.solve(f, tol=TOL, max_iter=MAX_ITER, deflate=(w, v))
    check_solution(x.cpu().numpy(), info, case["h"], case["z"], case["b"], f, label=f"device, {k} modes deflated")
    plain = case["runs"][0][1]["iterations"]
    print(f"iterations: {plain.max()} undeflated, {info['iterations'].max()} deflated")
    assert info["iterations"].max() < plain.max()
    # host arrays are taken as well as tensors
    x2, _ = op.solve(f, tol=TOL, max_iter=MAX_ITER, deflate=(w.cpu().numpy(), v.cpu().numpy()))
    assert np.array_equal(x2.cpu().numpy(), x.cpu().numpy())


def test_five_iterations_return_unconverged_columns_without_raising(sc):
    import torch

    coord = coord_of("A")
    op = sc.PairOperator(coord, sc.InvariantForceField(7.0))
    x, info = op.solve(right_hand_sides(len(coord), 3), tol=TOL, max_iter=5)
    assert info["converged"] is False and np.all(info["iterations"] == 5) and np.all(info["status"] == 0)
    assert bool(torch.isfinite(x).all()) and np.all(np.isfinite(info["residuals"])) and np.all(info["residuals"] > TOL)


def test_a_disconnected_network_does_not_converge_and_raises_nothing(sc):
    import torch

    a = coord_of("A")
    coord = np.concatenate([a, a + np.array([100.0 + np.ptp(a[:, 0]), 0.0, 0.0])])
    op = sc.PairOperator(coord, sc.InvariantForceField(7.0))
    lam = np.linalg.eigvalsh(dense_of(sc, coord, 3, None))
    assert np.all(np.abs(lam[:12]) <= 1e-9 * lam[-1]) and lam[12] > 1e-4 * lam[-1]   # twelve zero modes
    x, info = op.solve(np.random.RandomState(11).standard_normal((3, 3 * len(coord))), tol=TOL, max_iter=40)
    assert info["converged"] is False and tuple(x.shape) == (3, 3 * len(coord))
    assert set(info["status"]) <= {0, 2} and np.all(info["iterations"] <= 40)


@pytest.mark.parametrize("masses", [False, True], ids=["plain", "mass"])
def test_linear_response_is_the_reference_formula(sc, masses):
    from scipy.linalg import pinvh

    coord = coord_of("A")
    n = len(coord)
    mass = masses_of(n) if masses else None
    op = sc.PairOperator(coord, sc.InvariantForceField(7.0), masses=mass)
    h = dense_of(sc, coord, 3, mass)
    s = np.ones(3 * n) if mass is None else np.repeat(1.0 / np.sqrt(mass), 3)
    force = right_hand_sides(n, 3).reshape(7, n, 3)
    ref = (pinvh(h) @ (force.reshape(7, -1) * s).T).T * s   # the Cartesian response
    x, info = op.linear_response(force, tol=TOL, max_iter=MAX_ITER)
    assert tuple(x.shape) == (7, n, 3) and info["converged"]
    z, b = op.null_space().cpu().numpy(), op.spectral_bound()
    check_solution(x.cpu().numpy().reshape(7, -1) / s, info, h, z, b, force.reshape(7, -1) * s, label="linear response")
    fp = force.reshape(7, -1) * s
    fp = fp - (fp @ z) @ z.T
    lam_nz = np.linalg.eigvalsh(h)[6]
    err = np.linalg.norm(x.cpu().numpy().reshape(7, -1) - ref, axis=1)
    gate = s.max() * (TOL * np.linalg.norm(fp, axis=1) / lam_nz + 1e-12 * np.linalg.norm(ref / s, axis=1))
    print(f"Cartesian response vs pinvh: max err / gate {(err / gate).max():.3f}")
    assert np.all(err <= gate)
    # the other shapes, and the scale given explicitly
    one, _ = op.linear_response(force[3], tol=TOL, max_iter=MAX_ITER)
    flat, _ = op.linear_response(force[3].reshape(-1), tol=TOL, max_iter=MAX_ITER,
                                 atom_scale=None if mass is None else 1.0 / np.sqrt(mass))
    assert tuple(one.shape) == tuple(flat.shape) == (n, 3)
    assert np.array_equal(one.cpu().numpy(), x[3].cpu().numpy()) and np.array_equal(flat.cpu().numpy(), one.cpu().numpy())


def test_covariance_columns_are_rows_of_the_dense_pseudo_inverse(sc):
    case = case_of(sc, ("A", False, 3))
    op, h, z, b = case["op"], case["h"], case["z"], case["b"]
    atoms = [0, 57, 119]
    cols, info = op.covariance_columns(atoms, tol=TOL, max_iter=MAX_ITER)
    assert tuple(cols.shape) == (9, 360)
    rows = (3 * np.array(atoms)[:, None] + np.arange(3)).reshape(-1)
    unit = np.eye(360)[rows]
    check_solution(cols.cpu().numpy(), info, h, z, b, unit, label="covariance columns")
    lam, vec = np.linalg.eigh(h)
    cov = (vec[:, 6:] / lam[6:]) @ vec[:, 6:].T
    msf = np.array([np.trace(cov[3 * a: 3 * a + 3, 3 * a: 3 * a + 3]) for a in atoms])
    got = np.array([np.trace(cols.cpu().numpy()[3 * k: 3 * k + 3, 3 * a: 3 * a + 3]) for k, a in enumerate(atoms)])
    fp = unit - (unit @ z) @ z.T
    gate = 3 * (TOL * np.linalg.norm(fp, axis=1).max() / lam[6] + 1e-12 * np.linalg.norm(cov[rows], axis=1).max())
    print(f"exact MSF of atoms {atoms}: {got}, dense {msf}, max diff / gate {(np.abs(got - msf) / gate).max():.3f}")
    assert np.all(np.abs(got - msf) <= gate)


def test_rtb_exact_response_deflates_only_after_a_converged_refine(sc):
    coord = coord_of("B")
    n = len(coord)
    h = dense_of(sc, coord, 3, None)
    rtb = sc.RTB(coord, sc.InvariantForceField(7.0), np.arange(n) // 8)
    force = right_hand_sides(n, 3)[:3].reshape(3, n, 3)
    rtb.solve(subset_by_index=(0, 17))
    rtb.finish()
    z, b = rtb.operator.null_space().cpu().numpy(), rtb.operator.spectral_bound()
    x0, info0 = rtb.exact_response(force, tol=TOL, max_iter=MAX_ITER)   # block modes are not exact: undeflated
    check_solution(x0.cpu().numpy().reshape(3, -1), info0, h, z, b, force.reshape(3, -1), label="RTB, after solve")
    plain, _ = rtb.operator.solve(force.reshape(3, -1), tol=TOL, max_iter=MAX_ITER)
    assert np.array_equal(plain.cpu().numpy(), x0.cpu().numpy().reshape(3, -1))
    assert rtb.refine(tol=1e-10)["converged"]
    x1, info1 = rtb.exact_response(force, tol=TOL, max_iter=MAX_ITER)
    check_solution(x1.cpu().numpy().reshape(3, -1), info1, h, z, b, force.reshape(3, -1), label="RTB, after refine")
    print(f"iterations: {info0['iterations'].max()} after solve, {info1['iterations'].max()} after refine")
    assert info1["iterations"].max() < info0["iterations"].max()
    x2, info2 = rtb.exact_response(force, tol=TOL, max_iter=MAX_ITER, deflate=False)
    assert np.array_equal(info2["iterations"], info0["iterations"]) and np.array_equal(x2.cpu().numpy(), x0.cpu().numpy())
    with pytest.raises(ValueError, match="deflate"):
        rtb.operator.solve(force.reshape(3, -1), deflate=3)
    rtb.solve(subset_by_index=(0, 17))   # block modes again: undeflated again
    _, info3 = rtb.exact_response(force, tol=TOL, max_iter=MAX_ITER)
    assert np.array_equal(info3["iterations"], info0["iterations"])
