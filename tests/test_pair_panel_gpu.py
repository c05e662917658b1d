"""
GPU tests of the column-panel step ``Z <- alpha (T H T) X + beta X + gamma_c Z``: ``k_pairs_panel`` of csrc/pair_panel.hip
through ``sc_dev_pairs_panel_f64`` and :meth:`springcraft_amd.PairOperator.panel_step`.

Structures: A = ``lattice(4, 5, 6, 3)`` under ``InvariantForceField(7.0)`` (N = 120, 30 workgroups, 6 .. 26 pairs per atom)
and the operator tests' ``chain(40, 2)`` with atom 17 moved 100 A away (an atom without pairs); N = 1 (no pair at all).
Each in dim 3 and dim 1, with and without masses ``RandomState(5).uniform(50, 200, N)``.  Panels: q in {1, 3, 64, 65, 130}
(below one chunk of 64 columns, exactly one, one more, three chunks with a ragged last), ld in {q, q + 3}, and
(alpha, beta, gamma_c) in {(1, 0, 0), (0.7, -1.3, 0.4)}.  One panel of 130 standard-normal columns and one ``Z0`` serve all
of them per case: a column's result does not depend on the others, so one NumPy reference does.

Reference: :func:`panel_reference`, the operator tests' NumPy restatement of the three formulas on the transposed panel.
Tolerance, the one the operator tests derive: a float64 sum of fewer than 1000 terms of atom i errs by less than 1e-13 of
``B_i = sum_p gamma_p (|u_i|_1 + |u_j|_1)``; the scaled product by ``|alpha| 1e-12 t_i B_i``, and ``beta X + gamma_c Z`` add a
rounding each of their own size and of the sums': ``|alpha| 1e-12 t_i B_i + 4 eps (|beta| |X| + |gamma_c| |Z0|)`` elementwise.
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_iterative_host import lattice
from tests.test_pair_operator_gpu import ISOLATED, bits, masses_of, network, restate, structure

pytestmark = pytest.mark.gpu

QS = (1, 3, 64, 65, 130)
QMAX = 130
COEFS = ((1.0, 0.0, 0.0), (0.7, -1.3, 0.4))
SENTINEL = -7.25
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def sc():
    import springcraft_amd

    return springcraft_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def panel_reference(coord, pairs, gamma, scale, x, dim):
    """``H X`` (m, q) and the tolerance magnitude ``t_i B_i`` (m, q) for the columns of ``x`` (m, q), in NumPy."""
    ref = restate(coord, pairs, gamma, scale, np.ascontiguousarray(x.T), dim)
    return ref["Y"].T, np.repeat(ref["B"], dim, axis=1).T


CASES = [(name, masses, dim) for name in ("A", "n40iso") for dim in (3, 1) for masses in (False, True)]
CASE_IDS = [f"{name}-dim{dim}-{'mass' if masses else 'plain'}" for name, masses, dim in CASES]
_cache = {}


def case_of(sc, torch, key):
    if key not in _cache:
        name, masses, dim = key
        coord, ff = (lattice(4, 5, 6, 3), sc.InvariantForceField(7.0)) if name == "A" else structure(sc, name)
        n = len(coord)
        mass = masses_of(n) if masses else None
        scale = None if mass is None else 1.0 / np.sqrt(mass)
        pairs, gamma = network(sc, coord, ff)
        rng = np.random.RandomState(21)
        x, z0 = rng.standard_normal((dim * n, QMAX)), rng.standard_normal((dim * n, QMAX))
        hx, tb = panel_reference(coord, pairs, gamma, scale, x, dim)
        op = sc.PairOperator(coord, ff, dim=dim, masses=mass)
        _cache[key] = {"name": name, "n": n, "dim": dim, "m": dim * n, "pairs": pairs, "x": x, "z0": z0, "hx": hx, "tb": tb,
                       "op": op, "xd": torch.from_numpy(x).cuda(), "zd": torch.from_numpy(z0).cuda()}
    return _cache[key]


@pytest.fixture(params=CASES, ids=CASE_IDS)
def case(request, sc, torch):
    return case_of(sc, torch, request.param)


def run(torch, case, q, ld, coef, x=None, z0=None):
    """One panel step on the first q columns inside buffers of leading dimension ld: the whole (m, ld) result buffer."""
    x = case["xd"] if x is None else x
    z0 = case["zd"] if z0 is None else z0
    xbuf = torch.full((case["m"], ld), SENTINEL, dtype=torch.float64, device="cuda")
    zbuf = torch.full((case["m"], ld), SENTINEL, dtype=torch.float64, device="cuda")
    xbuf[:, :q] = x[:, :q]
    zbuf[:, :q] = z0[:, :q]
    out = case["op"].panel_step(xbuf[:, :q], zbuf[:, :q], *coef)
    assert out.data_ptr() == zbuf.data_ptr() and tuple(out.shape) == (case["m"], q)
    return zbuf


def test_panel_step_matches_the_restatement_and_leaves_the_padding(case, torch):
    worst = 0.0
    for q in QS:
        for ld in (q, q + 3):
            for alpha, beta, gamma_c in COEFS:
                z = run(torch, case, q, ld, (alpha, beta, gamma_c)).cpu().numpy()
                x, z0 = case["x"][:, :q], case["z0"][:, :q]
                ref = alpha * case["hx"][:, :q] + beta * x + gamma_c * z0
                tol = abs(alpha) * 1e-12 * case["tb"][:, :q] + 4 * EPS * (abs(beta) * np.abs(x) + abs(gamma_c) * np.abs(z0))
                err = np.abs(z[:, :q] - ref)
                worst = max(worst, float(np.max(err / np.where(tol > 0, tol, 1))))
                assert np.all(err <= tol), (q, ld, alpha)
                assert np.all(z[:, q:] == SENTINEL), (q, ld, alpha)   # columns q .. ld - 1 keep their bits
    print(f"panel vs restatement: max err / tol {worst:.3e}")


def test_panel_step_matches_apply(case, torch):
    z = run(torch, case, QMAX, QMAX, COEFS[0])
    y = case["op"].apply(case["xd"].T.contiguous()).T
    err = (z - y).abs().cpu().numpy()
    tol = 1e-12 * case["tb"]
    print(f"panel vs apply: max err / tol {np.max(err / np.where(tol > 0, tol, 1)):.3e}")
    assert np.all(err <= tol)


@pytest.mark.parametrize("coef", COEFS, ids=["plain", "recurrence"])
def test_a_column_has_the_same_bits_alone_and_at_another_ld(case, torch, coef):
    full = run(torch, case, QMAX, QMAX, coef)
    assert torch.equal(bits(run(torch, case, QMAX, QMAX, coef)), bits(full))   # two calls
    assert torch.equal(bits(run(torch, case, QMAX, QMAX + 3, coef)[:, :QMAX]), bits(full))
    for q in QS[:-1]:
        assert torch.equal(bits(run(torch, case, q, q + 3, coef)[:, :q]), bits(full[:, :q]))
    for r in (0, 63, 64, 77, 129):   # every chunk, first and last lane
        one = slice(r, r + 1)
        alone = run(torch, case, 1, 1, coef, x=case["xd"][:, one], z0=case["zd"][:, one])
        assert torch.equal(bits(alone[:, 0]), bits(full[:, r])), r
        wide = run(torch, case, 1, 4, coef, x=case["xd"][:, one], z0=case["zd"][:, one])
        assert torch.equal(bits(wide[:, 0]), bits(full[:, r])), r


def test_z_is_not_read_when_gamma_c_is_zero(case, torch):
    nan = torch.full_like(case["zd"], float("nan"))
    for q in (3, 65):
        z = run(torch, case, q, q + 3, (1.0, -0.5, 0.0), z0=nan)
        assert bool(torch.isfinite(z[:, :q]).all())
        assert torch.equal(bits(z[:, :q]), bits(run(torch, case, q, q + 3, (1.0, -0.5, 0.0))[:, :q]))


def test_a_nan_column_stays_alone(case, torch):
    coef = COEFS[1]
    clean = run(torch, case, QMAX, QMAX, coef)
    for r in (0, 64):   # (64: the first column of its chunk, which the lanes beyond q = 67 read in place of their own)
        bad = case["xd"].clone()
        bad[:, r] = float("nan")
        for q in (QMAX, 67):
            z = run(torch, case, q, q, coef, x=bad)
            keep = [c for c in range(q) if c != r]
            assert torch.equal(bits(z[:, keep]), bits(clean[:, keep]))
            assert bool(torch.isnan(z[:, r]).all())


def test_an_atom_without_pairs_gets_beta_x_plus_gamma_z(case):
    import torch

    n, dim = case["n"], case["dim"]
    lonely = np.nonzero(np.bincount(case["pairs"][:, 0], minlength=n) == 0)[0]
    assert list(lonely) == ([ISOLATED] if case["name"] == "n40iso" else [])
    rows = (dim * lonely[:, None] + np.arange(dim)[None, :]).reshape(-1)
    for alpha, beta, gamma_c in COEFS + ((2.0, 0.0, -0.3),):
        z = run(torch, case, QMAX, QMAX, (alpha, beta, gamma_c)).cpu().numpy()
        expect = beta * case["x"][rows] + (gamma_c * case["z0"][rows] if gamma_c != 0 else 0.0)
        assert np.array_equal(z[rows], expect)


@pytest.mark.parametrize("dim", [3, 1])
def test_a_single_atom_has_no_h_term(sc, torch, dim):
    coord, ff = structure(sc, "n1")
    op = sc.PairOperator(coord, ff, dim=dim)
    assert op.n_pairs == 0
    rng = np.random.RandomState(3)
    x, z0 = rng.standard_normal((dim, 65)), rng.standard_normal((dim, 65))
    for alpha, beta, gamma_c in COEFS:
        z = torch.from_numpy(z0).cuda()
        op.panel_step(torch.from_numpy(x).cuda(), z, alpha, beta, gamma_c)
        expect = beta * x + (gamma_c * z0 if gamma_c != 0 else 0.0)
        assert np.array_equal(z.cpu().numpy(), expect)


def test_invalid_arguments_are_refused_before_a_launch(sc, torch):
    from springcraft_amd import _hip

    case = case_of(sc, torch, ("A", False, 3))
    op, L = case["op"], _hip.lib()
    n, k, q, ld = op.n_atoms, op.n_pairs, 5, 8
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    x = case["xd"][:, :ld].contiguous()
    z = torch.full((3 * n, ld), SENTINEL, dtype=torch.float64, device="cuda")

    def panel(coord=op._coord, n_atoms=n, dim=3, pairs=op._pairs, kk=k, gamma=op._gamma, start=op._row_start, xx=x, zz=z,
              lead=ld, qq=q, coef=(1.0, 0.0, 0.0)):
        return L.sc_dev_pairs_panel_f64(op.ctx.handle, p(coord), n_atoms, dim, p(pairs), kk, p(gamma), p(start), None,
                                        p(xx), p(zz), lead, qq, *coef)

    bad = _hip.SC_ERR_INVALID_ARG
    assert panel(zz=x) == bad                                   # aliasing
    assert panel(lead=q - 1) == bad and panel(lead=-1, qq=0) == bad
    assert panel(dim=2) == bad and panel(dim=0) == bad
    assert panel(coord=None) == bad
    assert panel(n_atoms=0) == bad and panel(n_atoms=-3) == bad
    assert panel(kk=-1) == bad and panel(qq=-1) == bad
    assert panel(pairs=None) == bad and panel(gamma=None) == bad and panel(start=None) == bad
    assert panel(xx=None) == bad and panel(zz=None) == bad
    torch.cuda.synchronize()
    assert bool((z == SENTINEL).all()), "a refused call wrote to its result"
    assert bool((x == case["xd"][:, :ld]).all())
    # valid corner cases: no columns; no pairs with NULL pair arrays
    assert panel(qq=0) == _hip.SC_OK and panel(qq=0, xx=None, zz=None) == _hip.SC_OK
    torch.cuda.synchronize()
    assert bool((z == SENTINEL).all())
    assert panel(kk=0, pairs=None, gamma=None, start=None, coef=(1.0, 2.0, 0.0)) == _hip.SC_OK
    torch.cuda.synchronize()
    assert torch.equal(z[:, :q], 2.0 * x[:, :q]) and bool((z[:, q:] == SENTINEL).all())
    assert panel() == _hip.SC_OK
    torch.cuda.synchronize()
    assert torch.equal(bits(z[:, :q]), bits(run(torch, case, q, q, COEFS[0])))
    # the wrapper's own refusals
    with pytest.raises(ValueError, match="strides"):
        op.panel_step(case["xd"].T.contiguous().T, case["zd"].clone(), 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="columns"):
        op.panel_step(case["xd"], case["zd"][:, :5].contiguous(), 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="must not be the input"):
        op.panel_step(case["xd"], case["xd"], 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="Expected a panel"):
        op.panel_step(case["xd"][:-1], case["zd"][:-1], 1.0, 0.0, 0.0)
